// Launch wrappers of the layer kernels of swin_unet_v2.hip that waifu2x.wgmlp_4x (wgmlp.hip) runs as well: both nets are built from
// GLUConvMLP, the DCAE-style shortcut PatchDown / PatchUp and the SourceResidual head of the same reference modules.
#pragma once
#include "common.h"

namespace nunif {

// F.glu over the channels: out[t][c] = in[t][c] * sigmoid(in[t][m + c]), in [M][2 m], out [M][m]
int launch_v2_glu(const f16 *in, f16 *out, long M, int m, hipStream_t s);
// PatchDown shortcut: pixel_unshuffle(2) of x [B,H,W,C] + mean over groups of 4 C / C2 adjacent channels -> out [B,H/2,W/2,C2]
int launch_v2_down_shortcut(const f16 *x, f16 *out, int B, int H, int W, int C, int C2, hipStream_t s);
// PatchUp shortcut + U-Net skip: out = pixel_shuffle(2)(repeat_interleave(low [B,H/2,W/2,C2], 4 C / C2)) + skip, both [B,H,W,C]
int launch_v2_up_shortcut(const f16 *low, const f16 *skip, f16 *out, int B, int H, int W, int C, int C2, hipStream_t s);
// SourceResidual: z [B,3,O,O] = centre crop of pixel_shuffle(s)(conv3x3(replicate_pad(src [B,3,T,T]))) + r * scale_bias (+ clamp)
int launch_v2_source_residual(const float *src, const float *r, const float *w, const float *scale_bias, float *z, int B, int T, int s_,
                              int O, int clamp01, hipStream_t s);

}  // namespace nunif
