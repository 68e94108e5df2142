// The reference's WABlock on the device, shared by row_flow_v3, MLBW (rowflow.hip) and DepthAA (depth_aa.hip): window attention with a
// learned score bias in place (wmha_kernel / wmha8_kernel), conv_mlp[0] 1x1 + GELU(erf) (gemm_kernel), ReplicationPad2d(1) + 3x3 with
// the block's residual (conv_kernel).  wa_block_host.h builds a block's arrays, wa_block.hip uploads and runs them.
#pragma once
#include <string>

#include "packed_layers.h"

namespace nunif {

struct WaBlock {
    f16 *wfrag = nullptr; float *bqkv = nullptr, *bproj = nullptr, *btab = nullptr;
    PackedLinear mlp1;                               // conv_mlp[0] 1x1
    PackedConv mlp3;                                 // conv_mlp[3] 3x3
    int window = 4;
};

// what a handle of these nets owns besides its weights: the NHWC fp16 maps [tokens][C] of the block loop
struct WaMaps : DeviceOwner {
    DeviceBuf f, t1, t2;
    int ensure_maps(size_t tok, int C) {
        const size_t bytes = tok * C * sizeof(f16);
        int rc;
        if ((rc = f.ensure(bytes)) || (rc = t1.ensure(bytes))) return rc;
        return t2.ensure(bytes);
    }
    void release_maps() { f.release(); t1.release(); t2.release(); }
};

// window x window <= 16 tokens, C = 64 or 128 in heads of 32 (wmha_kernel), or window 8, C = 32 in heads of 16 (wmha8_kernel)
int make_wa_block(DeviceOwner *h, const TensorMap &m, const std::string &p, int window, int C, int hd, WaBlock *bk);

// n blocks on the map in h->f ([B,H,W,C]); block i zero-pads by (sy[i], sx[i]) for its windows (WindowMHA2d's shift).  act / slope:
// the 3x3 conv's activation, as in ConvArgs; tag: the profiler class of the 1x1.  *out: the buffer that holds the result, f or t2.
int run_wa_blocks(WaMaps *h, const WaBlock *blk, int n, const int *sy, const int *sx, int C, int B, int H, int W, int act, float slope,
                  const char *tag, hipStream_t s, f16 **out);

}  // namespace nunif
