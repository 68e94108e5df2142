// waifu2x.wgmlp_4x (window gMLP + GLU conv-MLP on a two-level U-Net with an IR / Overscan stem) on the HIP engine.
//
// Reference: waifu2x/models/wgmlp.py — GLUConvMLP :15-35, MLP :38-52, WGMLPBlock :75-101, WGMLPBlocks :104-123, Overscan :126-153,
// IR :156-173, PatchDown :176-200, PatchUp :203-226, ToImage :229-242, SourceResidual :245-286, get_shift_config :289-295,
// WGMLPBase :298-353 (_forward :339-353), WGMLP4x :441-470; nunif/modules/attention.py GMLP :621-651, WindowGMLP2d :654-693.
//
// New here: wgmlp_block_kernel, ONE launch per WindowGMLP2d call (LayerNorm 1, proj_in, GELU, LayerNorm 2 on v, the 64 x 64 token
// mixing, the gate, proj_out and the shortcut; a 64-token window with its 2 C hidden row lives in LDS, x is read and written in
// place), and wg_stem_conv_kernel, the direct fp32 convs of the IR stem.  The rest is the composition swin_unet_v2.hip runs on:
// gemm_kernel for every 1x1 / 2x2-s2 conv and the pixel-shuffle heads, conv_kernel for the 3x3 convs, and that file's GLU, shortcut
// and source-residual kernels (swin_unet_v2_kernels.h).  Maps are NHWC fp16, accumulation fp32.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "packed_layers.h"
#include "swin_unet_v2_kernels.h"
#include "wgmlp_host.h"

namespace nunif {

// ---- the fused window-gMLP block ------------------------------------------------------------------------------------------------------
// x: [B,H,W,C] fp16, updated in place (a window reads and writes its own tokens only).  w_in / w_out / w_sp: PackedLinear fragments in
// [n-tile][k-step] order, streamed from L2 per window (w_in, w_out) or held in registers for the whole launch (w_sp, 8 fragments).
// A token of a border window of a shifted block that lies in the zero padding is LayerNorm(0) = 0, so it enters the mixing as
// LayerNorm2(gelu(b_in)) like in the reference; it is computed and never stored.
// taps (debug launches): fp32 maps indexed like x — LayerNorm 1 [C], GELU [2 C], LayerNorm 2 [C], mixing [C], gate [C].
struct WgmlpArgs {
    f16 *x;
    const f16 *w_in, *w_out, *w_sp;
    const float *b_in, *b_out, *b_sp, *g1, *g2;
    int B, H, W, pad, nwy, nwx;
    long windows;
    float *taps[5];
};

template <int C, bool TAPS>
__global__ void __launch_bounds__(256) wgmlp_block_kernel(WgmlpArgs a) {
    constexpr int XS = C + kWgLdsPad;              // row stride of the LayerNorm-1 tile
    constexpr int VS = kWgTokens + kWgLdsPad;      // row stride of the transposed LayerNorm-2 tile
    constexpr int HS = wgmlp_lds_h_stride(C);
    constexpr int KS = C / 32;                     // k-steps of proj_in / proj_out
    constexpr int CP = C / 4;                      // channels of a token per LayerNorm thread
    __shared__ __attribute__((aligned(16))) f16 smem_wg[wgmlp_lds_a_halfs(C) + wgmlp_lds_h_halfs(C)];      // wgmlp_lds_bytes(C)
    f16 *xs = smem_wg;
    f16 *hs = xs + wgmlp_lds_a_halfs(C);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, g = lane >> 4;
    const int lt = tid >> 2, lp = tid & 3;         // LayerNorm passes: token, quarter (chunks of 8 channels, interleaved by 4)

    // the mixing matrix and its bias: stationary in registers
    f16x8 wsp[4][2];
    float bsp[4][4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) wsp[tt][ks] = *reinterpret_cast<const f16x8 *>(a.w_sp + ((size_t)(tt * 2 + ks) * 64 + lane) * 8);
#pragma unroll
        for (int i = 0; i < 4; ++i) bsp[tt][i] = a.b_sp[tt * 16 + 4 * g + i];
    }

    for (long wi = blockIdx.x; wi < a.windows; wi += gridDim.x) {
        const int wx = (int)(wi % a.nwx), wy = (int)((wi / a.nwx) % a.nwy), b = (int)(wi / ((long)a.nwx * a.nwy));
        const int y0 = wy * kWgWindow - a.pad, x0 = wx * kWgWindow - a.pad;
        auto inside = [&](int t) {
            const int y = y0 + (t >> 3), x = x0 + (t & 7);
            return y >= 0 && y < a.H && x >= 0 && x < a.W;
        };
        auto pixel = [&](int t) { return ((long)b * a.H + y0 + (t >> 3)) * a.W + x0 + (t & 7); };

        // ---- LayerNorm 1 -> xs [token][C] --------------------------------------------------------------------------------------
        {
            const bool in = inside(lt);
            const long p = in ? pixel(lt) : 0;
            float v[CP];
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < CP / 8; ++j) {
                f16x8 q = {};
                if (in) q = *reinterpret_cast<const f16x8 *>(a.x + p * C + (j * 4 + lp) * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) { v[j * 8 + e] = (float)q[e]; sum += v[j * 8 + e]; }
            }
            sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2);
            const float mean = sum * (1.0f / C);
            float var = 0.f;
#pragma unroll
            for (int j = 0; j < CP; ++j) { const float d = v[j] - mean; var = fmaf(d, d, var); }
            var += __shfl_xor(var, 1); var += __shfl_xor(var, 2);
            const float r = rsqrtf(var * (1.0f / C) + 1e-5f);
#pragma unroll
            for (int j = 0; j < CP / 8; ++j) {
                const int c0 = (j * 4 + lp) * 8;
                f16x8 q;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float o = in ? (v[j * 8 + e] - mean) * r * a.g1[c0 + e] : 0.f;
                    q[e] = (f16)o;
                    if (TAPS && in && a.taps[0]) a.taps[0][p * C + c0 + e] = o;
                }
                *reinterpret_cast<f16x8 *>(xs + lt * XS + c0) = q;
            }
        }
        __syncthreads();

        // ---- proj_in C -> 2 C + exact GELU -> hs [token][2 C]: a wave takes pairs of output tiles over all 64 tokens ----------------
        for (int nt = wave * 2; nt < 2 * C / 16; nt += 8) {
            f32x4 acc[2][4];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc[n][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const f16x8 w0 = *reinterpret_cast<const f16x8 *>(a.w_in + ((size_t)(nt * KS + ks) * 64 + lane) * 8);
                const f16x8 w1 = *reinterpret_cast<const f16x8 *>(a.w_in + ((size_t)((nt + 1) * KS + ks) * 64 + lane) * 8);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f16x8 xb = *reinterpret_cast<const f16x8 *>(xs + (tt * 16 + l16) * XS + ks * 32 + g * 8);
                    acc[0][tt] = MFMA_16x16x32(w0, xb, acc[0][tt]);
                    acc[1][tt] = MFMA_16x16x32(w1, xb, acc[1][tt]);
                }
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int c0 = (nt + n) * 16 + 4 * g;
                const f32x4 bi = *reinterpret_cast<const f32x4 *>(a.b_in + c0);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int t = tt * 16 + l16;
                    f16x4 q;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float z = acc[n][tt][i] + bi[i];
                        const float o = 0.5f * z * (1.0f + erff(z * 0.70710678118654752f));
                        q[i] = (f16)o;
                        if (TAPS && a.taps[1] && inside(t)) a.taps[1][pixel(t) * 2 * C + c0 + i] = o;
                    }
                    *reinterpret_cast<f16x4 *>(hs + t * HS + c0) = q;
                }
            }
        }
        __syncthreads();

        // ---- LayerNorm 2 on v = hs[:, C:2C] -> xs TRANSPOSED [channel][token] ----------------------------------------------------
        {
            float v[CP];
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < CP / 8; ++j) {
                const f16x8 q = *reinterpret_cast<const f16x8 *>(hs + lt * HS + C + (j * 4 + lp) * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) { v[j * 8 + e] = (float)q[e]; sum += v[j * 8 + e]; }
            }
            sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2);
            const float mean = sum * (1.0f / C);
            float var = 0.f;
#pragma unroll
            for (int j = 0; j < CP; ++j) { const float d = v[j] - mean; var = fmaf(d, d, var); }
            var += __shfl_xor(var, 1); var += __shfl_xor(var, 2);
            const float r = rsqrtf(var * (1.0f / C) + 1e-5f);
            const bool in = TAPS && inside(lt);
            const long p = in ? pixel(lt) : 0;
#pragma unroll
            for (int j = 0; j < CP / 8; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = (j * 4 + lp) * 8 + e;
                    const float o = (v[j * 8 + e] - mean) * r * a.g2[c];
                    xs[c * VS + lt] = (f16)o;
                    if (TAPS && in && a.taps[2]) a.taps[2][p * C + c] = o;
                }
        }
        __syncthreads();

        // ---- token mixing v'[t][c] = sum_s Ws[t][s] v[s][c] + bs[t] and the gate u * v' -> hs[:, 0:C] --------------------------------
        for (int ct = wave; ct < C / 16; ct += 4) {
            const int c = ct * 16 + l16;
            const f16x8 v0 = *reinterpret_cast<const f16x8 *>(xs + c * VS + g * 8);
            const f16x8 v1 = *reinterpret_cast<const f16x8 *>(xs + c * VS + 32 + g * 8);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
                acc = MFMA_16x16x32(wsp[tt][0], v0, acc);
                acc = MFMA_16x16x32(wsp[tt][1], v1, acc);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int t = tt * 16 + 4 * g + i;
                    const float m = acc[i] + bsp[tt][i];
                    const float o = (float)hs[t * HS + c] * m;
                    hs[t * HS + c] = (f16)o;
                    if (TAPS && inside(t)) {
                        if (a.taps[3]) a.taps[3][pixel(t) * C + c] = m;
                        if (a.taps[4]) a.taps[4][pixel(t) * C + c] = o;
                    }
                }
            }
        }
        __syncthreads();

        // ---- proj_out C -> C + shortcut -> x ----------------------------------------------------------------------------------------
        for (int nt = wave * 2; nt < C / 16; nt += 8) {
            f32x4 acc[2][4];
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) acc[n][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const f16x8 w0 = *reinterpret_cast<const f16x8 *>(a.w_out + ((size_t)(nt * KS + ks) * 64 + lane) * 8);
                const f16x8 w1 = *reinterpret_cast<const f16x8 *>(a.w_out + ((size_t)((nt + 1) * KS + ks) * 64 + lane) * 8);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f16x8 gb = *reinterpret_cast<const f16x8 *>(hs + (tt * 16 + l16) * HS + ks * 32 + g * 8);
                    acc[0][tt] = MFMA_16x16x32(w0, gb, acc[0][tt]);
                    acc[1][tt] = MFMA_16x16x32(w1, gb, acc[1][tt]);
                }
            }
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int t = tt * 16 + l16;
                if (!inside(t)) continue;
                f16 *row = a.x + pixel(t) * C;
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const int c0 = (nt + n) * 16 + 4 * g;
                    const f32x4 bo = *reinterpret_cast<const f32x4 *>(a.b_out + c0);
                    const f16x4 sc = *reinterpret_cast<const f16x4 *>(row + c0);
                    f16x4 q;
#pragma unroll
                    for (int i = 0; i < 4; ++i) q[i] = (f16)(acc[n][tt][i] + bo[i] + (float)sc[i]);
                    *reinterpret_cast<f16x4 *>(row + c0) = q;
                }
            }
        }
        // no barrier here: the next trip writes xs, last read before the barrier above, and hs only after its own first barrier
    }
}

// ---- IR stem: direct fp32 k x k convs on fp32 NHWC maps (8 / 16-channel maps; wgmlp.py:126-173) -----------------------------------
// The input is up to three maps concatenated along the channels (the torch.cat of Overscan); each is read at (y + off + dy * dil,
// x + off + dx * dil) CLAMPED to its own extent, which is ReplicationPad2d(-off) for off < 0, a crop by off for off > 0 and has no
// effect on a valid conv.  planar: the fp32 NCHW network input.  w: [tap][ci][COUT] fp32.
struct WgSeg { const float *p; int C, ld, S, off, planar; };
struct WgStemArgs {
    WgSeg seg[3];
    int nseg, cin;
    const float *w, *bias;
    float *out;            // fp32 NHWC [B,So,So,ldo], channels coff .. coff + COUT
    f16 *out16;            // or fp16 NHWC [B,So,So,ldo]: COUT channels, then zeros up to ldo
    int B, So, ldo, coff, k, dil, act;
};

template <int COUT>
__global__ void __launch_bounds__(256) wg_stem_conv_kernel(WgStemArgs a) {
    __shared__ float ws[9 * 32 * 16 + 16];
    const int nw = a.k * a.k * a.cin * COUT;
    for (int i = threadIdx.x; i < nw; i += 256) ws[i] = a.w[i];
    if (threadIdx.x < COUT) ws[9 * 32 * 16 + threadIdx.x] = a.bias[threadIdx.x];
    __syncthreads();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.B * a.So * a.So) return;
    const int px = (int)(i % a.So), py = (int)((i / a.So) % a.So), b = (int)(i / ((long)a.So * a.So));
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = ws[9 * 32 * 16 + co];
    int cbase = 0;
    for (int s = 0; s < a.nseg; ++s) {
        const WgSeg sg = a.seg[s];
        for (int tap = 0; tap < a.k * a.k; ++tap) {
            const int yy = min(max(py + sg.off + (tap / a.k) * a.dil, 0), sg.S - 1);
            const int xx = min(max(px + sg.off + (tap % a.k) * a.dil, 0), sg.S - 1);
            const float *wr = ws + (tap * a.cin + cbase) * COUT;
            if (sg.planar) {
                for (int c = 0; c < sg.C; ++c) {
                    const float v = sg.p[(((long)b * sg.C + c) * sg.S + yy) * sg.S + xx];
#pragma unroll
                    for (int co = 0; co < COUT; ++co) acc[co] = fmaf(wr[c * COUT + co], v, acc[co]);
                }
            } else {
                const f32x4 *src = reinterpret_cast<const f32x4 *>(sg.p + (((long)b * sg.S + yy) * sg.S + xx) * sg.ld);
                for (int c4 = 0; c4 < sg.C / 4; ++c4) {
                    const f32x4 v = src[c4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int co = 0; co < COUT; ++co) acc[co] = fmaf(wr[(c4 * 4 + e) * COUT + co], v[e], acc[co]);
                }
            }
        }
        cbase += sg.C;
    }
    if (a.act)
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[co] = acc[co] >= 0.f ? acc[co] : acc[co] * 0.2f;
    if (a.out16) {
        f16 *o = a.out16 + i * a.ldo;
#pragma unroll
        for (int co = 0; co < COUT; ++co) o[co] = (f16)acc[co];
        for (int co = COUT; co < a.ldo; ++co) o[co] = (f16)0.f;
    } else {
        float *o = a.out + i * a.ldo + a.coff;
#pragma unroll
        for (int co = 0; co < COUT; ++co) o[co] = acc[co];
    }
}

__global__ void __launch_bounds__(256) wg_f16_to_f32_kernel(const f16 *__restrict__ in, float *__restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
__global__ void __launch_bounds__(256) wg_f32_to_f16_kernel(const float *__restrict__ in, f16 *__restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (f16)in[i];
}

}  // namespace nunif

using namespace nunif;

// =====================================================================================================================
// host side
// =====================================================================================================================
namespace {

struct StemConv { float *w = nullptr, *bias = nullptr; int cin = 0, cout = 0, k = 3; };

struct WgBlock {
    PackedLinear proj_in, proj_out, spatial, w1, w2lin;
    PackedConv w2;
    float *g1 = nullptr, *g2 = nullptr;
    int C = 0, shift = 0, glu = 1;
};

}  // namespace

struct nunif_wgmlp : DeviceOwner {
    int C = 128, C2 = 256;
    StemConv ir_patch, ov1, ov2, ov3, fuse0, fuse2, fusion;
    PackedConv patch;
    std::vector<WgBlock> g1, g2, g3;
    PackedLinear down1, up1, to_image;
    float *res_w = nullptr, *scale_bias = nullptr;
    DeviceBuf ws, dbg;
};

namespace {

int make_stem_conv(nunif_wgmlp *h, const TensorMap &m, const std::string &key, int cin, int cout, int k, StemConv *c) {
    const HostTensor *w, *b;
    int rc;
    if ((rc = find(m, key + ".weight", &w)) || (rc = find(m, key + ".bias", &b))) return rc;
    NUNIF_REQUIRE(w->numel == (int64_t)cout * cin * k * k && b->numel == cout, "wgmlp: %s is not a %d x %d conv %d -> %d", key.c_str(), k, k,
                  cin, cout);
    std::vector<float> wv((size_t)k * k * cin * cout);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < k * k; ++tap) wv[((size_t)tap * cin + ci) * cout + co] = w->data[((size_t)co * cin + ci) * k * k + tap];
    c->cin = cin; c->cout = cout; c->k = k;
    if ((rc = h->upload(wv, &c->w))) return rc;
    return h->upload_f32(b, &c->bias);
}

int make_block(nunif_wgmlp *h, const TensorMap &m, const std::string &p, int C, int shift, bool glu, WgBlock *bk) {
    const HostTensor *n1, *n2, *sw, *sb;
    int rc;
    if ((rc = find(m, p + "norm1.weight", &n1)) || (rc = find(m, p + "norm2.weight", &n2)) ||
        (rc = find(m, p + "gmlp.gmlp.proj_spatial.weight", &sw)) || (rc = find(m, p + "gmlp.gmlp.proj_spatial.bias", &sb)))
        return rc;
    NUNIF_REQUIRE(n1->numel == C && n2->numel == C && sw->numel == kWgTokens * kWgTokens && sb->numel == kWgTokens,
                  "wgmlp: %s is not a window-gMLP block of %d channels with 8 x 8 windows", p.c_str(), C);
    bk->C = C; bk->shift = shift; bk->glu = glu;
    if ((rc = h->upload_f32(n1, &bk->g1)) || (rc = h->upload_f32(n2, &bk->g2))) return rc;
    if ((rc = linear_from(h, m, p + "gmlp.gmlp.proj_in", 2 * C, C, 16, &bk->proj_in)) ||
        (rc = linear_from(h, m, p + "gmlp.gmlp.proj_out", C, C, 16, &bk->proj_out)) ||
        (rc = linear_from(h, m, p + "gmlp.gmlp.proj_spatial", kWgTokens, kWgTokens, 16, &bk->spatial)) ||   // Conv1d(64, 64, 1): [t][s][1]
        (rc = linear_from(h, m, p + "conv_mlp.w1", 2 * C, C, 16, &bk->w1)))
        return rc;
    if (glu) return conv_from(h, m, p + "conv_mlp.w2", C, 16, C, C, 3, &bk->w2);
    return linear_from(h, m, p + "conv_mlp.w2", C, 2 * C, 16, &bk->w2lin);
}

template <int C, bool TAPS>
int launch_block_t(const WgmlpArgs &a, hipStream_t s) {
    wgmlp_block_kernel<C, TAPS><<<wgmlp_grid(a.windows, C), 256, 0, s>>>(a);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

// the WindowGMLP2d of block bk in place on x [B,H,W,C]; taps: nullptr or five fp32 maps (any of them nullptr)
int run_gmlp(const WgBlock &bk, f16 *x, int B, int H, int W, int shift, float *const *taps, hipStream_t s) {
    NUNIF_REQUIRE(wgmlp_channels_supported(bk.C) && wgmlp_map_supported(H, W), "wgmlp: a %d x %d map of %d channels is not windows of 8 x 8 at 128 / 256 channels",
                  H, W, bk.C);
    WgmlpArgs a{};
    a.x = x; a.w_in = bk.proj_in.w; a.w_out = bk.proj_out.w; a.w_sp = bk.spatial.w;
    a.b_in = bk.proj_in.bias; a.b_out = bk.proj_out.bias; a.b_sp = bk.spatial.bias; a.g1 = bk.g1; a.g2 = bk.g2;
    a.B = B; a.H = H; a.W = W; a.pad = wgmlp_pad(shift); a.nwy = wgmlp_windows_along(H, shift); a.nwx = wgmlp_windows_along(W, shift);
    a.windows = wgmlp_window_count(B, H, W, shift);
    for (int i = 0; i < 5; ++i) a.taps[i] = taps ? taps[i] : nullptr;
    const double M = (double)a.windows * kWgTokens, Cd = bk.C;
    ProfScope ps(bk.C == 128 ? "wgmlp_block_kernel<128>" : "wgmlp_block_kernel<256>", s, 2.0 * M * (3.0 * Cd * Cd + kWgTokens * Cd),
                 2.0 * (double)B * H * W * Cd * 2.0);
    if (bk.C == 128) return taps ? launch_block_t<128, true>(a, s) : launch_block_t<128, false>(a, s);
    return taps ? launch_block_t<256, true>(a, s) : launch_block_t<256, false>(a, s);
}

int run_lin(const PackedLinear &L, const f16 *a, int B, int S, int act, float slope, const f16 *res, f16 *out, hipStream_t s, const char *tag) {
    GemmArgs g = gemm_map_args(L, a, B, S, S, L.K, S, S, out);
    g.act = act; g.slope = slope; g.res = res;
    return launch_gemm(g, s, tag);
}

// one WGMLPBlock (:92-101) on *px [B,S,S,C]; the result ends up in *px again (the buffers swap for the 3x3 form)
int run_block(const WgBlock &bk, f16 **px, f16 **pother, f16 *tmpA, f16 *tmpB, int B, int S, hipStream_t s) {
    f16 *x = *px, *other = *pother;
    const long M = (long)B * S * S;
    int rc;
    if ((rc = run_gmlp(bk, x, B, S, S, bk.shift, nullptr, s))) return rc;
    if (bk.glu) {
        // x = x + leaky_relu(conv3x3(replicate_pad(glu(w1 x))), 0.2)      (GLUConvMLP :29-35)
        if ((rc = run_lin(bk.w1, x, B, S, 0, 0.f, nullptr, tmpB, s, "wgmlp_mlp_w1")) || (rc = launch_v2_glu(tmpB, tmpA, M, bk.C, s))) return rc;
        ConvArgs c = conv_args(bk.w2, tmpA, B, S, S, other, 1, 0, 1);
        c.act = 2; c.slope = 0.2f; c.res = x;
        if ((rc = launch_conv(c, s))) return rc;
        *px = other; *pother = x;
    } else {
        // x = x + w2(leaky_relu(w1 x, 0.1))                                (MLP :47-52)
        if ((rc = run_lin(bk.w1, x, B, S, 2, 0.1f, nullptr, tmpB, s, "wgmlp_mlp_w1")) ||
            (rc = run_lin(bk.w2lin, tmpB, B, S, 0, 0.f, x, x, s, "wgmlp_mlp_w2")))
            return rc;
    }
    return NUNIF_HIP_OK;
}

int run_stem_conv(const StemConv &c, const WgSeg *segs, int nseg, int B, int So, int dil, int act, float *out, int ldo, int coff, f16 *out16,
                  hipStream_t s) {
    WgStemArgs a{};
    int cin = 0;
    for (int i = 0; i < nseg; ++i) { a.seg[i] = segs[i]; cin += segs[i].C; }
    NUNIF_REQUIRE(cin == c.cin && cin <= 32 && (c.cout == 8 || c.cout == 16), "wgmlp: stem conv %d -> %d", cin, c.cout);
    a.nseg = nseg; a.cin = cin; a.w = c.w; a.bias = c.bias; a.out = out; a.out16 = out16; a.B = B; a.So = So; a.ldo = ldo; a.coff = coff;
    a.k = c.k; a.dil = dil; a.act = act;
    const long n = (long)B * So * So;
    ProfScope ps("wg_stem_conv_kernel", s, 2.0 * (double)n * c.k * c.k * cin * c.cout, (double)n * (cin + c.cout) * 4.0);
    if (c.cout == 16) wg_stem_conv_kernel<16><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a);
    else wg_stem_conv_kernel<8><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

int tap_out(const f16 *x, long n, float **tap, hipStream_t s) {
    if (!tap || !*tap) return NUNIF_HIP_OK;
    wg_f16_to_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(x, *tap, n);
    NUNIF_LAUNCH_CHECK();
    *tap += n;
    return NUNIF_HIP_OK;
}

// WGMLP4x.forward in eval mode (:457-467, _forward :339-353); taps: nullptr, or the nine block outputs in order as fp32 NHWC
int forward(nunif_wgmlp *h, const float *x, float *z, int B, int T, int clamp01, float *taps, hipStream_t s) {
    NUNIF_REQUIRE(h && x && z && B > 0, "wgmlp_forward: bad argument");
    NUNIF_REQUIRE(wgmlp_tile_supported(T), "tile_size %d is not valid for wgmlp_4x (T - 16 a positive multiple of 48)", T);
    const int S = T - 16, C = h->C, C2 = h->C2;
    const WgWorkspace w = wgmlp_workspace(B, T, C);
    int rc;
    if ((rc = h->ws.ensure(w.total))) return rc;
    auto at = [&](int r) { return (unsigned char *)h->ws.p + w.off[r]; };
    float *cat = (float *)at(WG_CAT), *x1 = (float *)at(WG_X1), *x2 = (float *)at(WG_X2), *x3 = (float *)at(WG_X3), *fu = (float *)at(WG_FU);
    f16 *ir = (f16 *)at(WG_IR), *tmpA = (f16 *)at(WG_TMPA), *tmpB = (f16 *)at(WG_TMPB);
    float *rimg = (float *)at(WG_RIMG);
    // ---- IR (:156-173) with Overscan (:126-153) ---------------------------------------------------------------------------------------
    {
        const WgSeg sx = {x, 3, 3, T, -1, 1};
        if ((rc = run_stem_conv(h->ir_patch, &sx, 1, B, T, 1, 1, cat, 32, 0, nullptr, s))) return rc;        // cat[..., 0:16]
        const WgSeg s0 = {cat, 16, 32, T, -7, 0};                                                             // ReplicationPad2d(7)
        if ((rc = run_stem_conv(h->ov1, &s0, 1, B, T + 12, 1, 1, x1, 16, 0, nullptr, s))) return rc;
        const WgSeg s1 = {x1, 16, 16, T + 12, 0, 0};
        if ((rc = run_stem_conv(h->ov2, &s1, 1, B, T + 8, 2, 1, x2, 8, 0, nullptr, s))) return rc;
        const WgSeg s2 = {x2, 8, 8, T + 8, 0, 0};
        if ((rc = run_stem_conv(h->ov3, &s2, 1, B, T + 2, 3, 1, x3, 8, 0, nullptr, s))) return rc;
        const WgSeg sc[3] = {{x1, 16, 16, T + 12, 5, 0}, {x2, 8, 8, T + 8, 3, 0}, {x3, 8, 8, T + 2, 0, 0}};     // crops 5, 3, cat
        if ((rc = run_stem_conv(h->fuse0, sc, 3, B, T, 1, 1, fu, 16, 0, nullptr, s))) return rc;
        const WgSeg sf = {fu, 16, 16, T, 0, 0};
        if ((rc = run_stem_conv(h->fuse2, &sf, 1, B, T, 1, 0, cat, 32, 16, nullptr, s))) return rc;           // cat[..., 16:32]
        const WgSeg sa = {cat, 32, 32, T, -1, 0};
        if ((rc = run_stem_conv(h->fusion, &sa, 1, B, T, 1, 0, nullptr, 32, 0, ir, s))) return rc;
    }
    // ---- patch: 3x3 VALID 16 -> C, crop 7, LeakyReLU(0.2) (:340-342): conv rows / cols [7, 7 + S) of the (T - 2)^2 result --------------
    f16 *l1[3] = {(f16 *)at(WG_L1A), (f16 *)at(WG_L1B), (f16 *)at(WG_L1C)};
    f16 *cur = l1[0], *other = l1[1];
    {
        ConvArgs c = conv_args(h->patch, ir + ((long)7 * T + 7) * 32, B, T, T, cur);
        c.Ho = S; c.Wo = S; c.act = 2; c.slope = 0.2f;
        if ((rc = launch_conv(c, s))) return rc;
    }
    const long M1 = (long)B * S * S;
    for (auto &bk : h->g1)
        if ((rc = run_block(bk, &cur, &other, tmpA, tmpB, B, S, s)) || (rc = tap_out(cur, M1 * C, &taps, s))) return rc;
    f16 *skip = cur, *dec = l1[2];
    // ---- down1 (:188-197): shortcut first, then the 2x2-s2 conv with LeakyReLU(0.2) accumulates onto it -----------------------------
    f16 *f2 = (f16 *)at(WG_L2A), *f2b = (f16 *)at(WG_L2B);
    if ((rc = launch_v2_down_shortcut(skip, f2, B, S, S, C, C2, s))) return rc;
    {
        GemmArgs g = gemm_map_args(h->down1, skip, B, S, S, C, S / 2, S / 2, f2, 2, 2);
        g.act = 2; g.slope = 0.2f; g.res = f2;
        if ((rc = launch_gemm(g, s, "wgmlp_down1"))) return rc;
    }
    for (auto &bk : h->g2)
        if ((rc = run_block(bk, &f2, &f2b, tmpA, tmpB, B, S / 2, s)) || (rc = tap_out(f2, M1 / 4 * C2, &taps, s))) return rc;
    // ---- up1 (:214-222) + skip (:348): shortcut + skip first, then proj + LeakyReLU(0.2) + pixel shuffle accumulates onto it ----------
    if ((rc = launch_v2_up_shortcut(f2, skip, dec, B, S, S, C, C2, s))) return rc;
    {
        GemmArgs g = gemm_map_args(h->up1, f2, B, S / 2, S / 2, C2, S / 2, S / 2, dec);
        g.mode = 1; g.act = 2; g.slope = 0.2f; g.res = dec; g.ldo = C;
        if ((rc = launch_gemm(g, s, "wgmlp_up1"))) return rc;
    }
    for (auto &bk : h->g3)
        if ((rc = run_block(bk, &dec, &other, tmpA, tmpB, B, S, s)) || (rc = tap_out(dec, M1 * C, &taps, s))) return rc;
    // ---- to_residual_image (:229-242): 1x1 conv, pixel shuffle, crop 4; then the source residual + clamp -----------------------------
    const int O = S * 4 - 8;
    {
        GemmArgs g = gemm_map_args(h->to_image, dec, B, S, S, C, S, S, rimg);
        g.mode = 2; g.ldo = 0; g.ps = 4; g.oshift = -4; g.OH = O; g.OW = O; g.no_clamp = 1;
        if ((rc = launch_gemm(g, s, "wgmlp_to_image"))) return rc;
    }
    return launch_v2_source_residual(x, rimg, h->res_w, h->scale_bias, z, B, T, 4, O, clamp01, s);
}

WgBlock *block_at(nunif_wgmlp *h, int i) {
    const int n1 = (int)h->g1.size(), n2 = (int)h->g2.size(), n3 = (int)h->g3.size();
    if (i < 0 || i >= n1 + n2 + n3) return nullptr;
    return i < n1 ? &h->g1[i] : i < n1 + n2 ? &h->g2[i - n1] : &h->g3[i - n1 - n2];
}

}  // namespace

extern "C" int nunif_hip_wgmlp_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_wgmlp **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "wgmlp_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_wgmlp *h = new nunif_wgmlp();
    const std::string P = "unet.";
    int rc = NUNIF_HIP_OK;
    do {
        const HostTensor *w, *b;
        if ((rc = make_stem_conv(h, m, P + "ir.patch", 3, 16, 3, &h->ir_patch)) ||
            (rc = make_stem_conv(h, m, P + "ir.overscan.conv1", 16, 16, 3, &h->ov1)) ||
            (rc = make_stem_conv(h, m, P + "ir.overscan.conv2", 16, 8, 3, &h->ov2)) ||
            (rc = make_stem_conv(h, m, P + "ir.overscan.conv3", 8, 8, 3, &h->ov3)) ||
            (rc = make_stem_conv(h, m, P + "ir.overscan.fuse.0", 32, 16, 3, &h->fuse0)) ||
            (rc = make_stem_conv(h, m, P + "ir.overscan.fuse.2", 16, 16, 1, &h->fuse2)) ||
            (rc = make_stem_conv(h, m, P + "ir.fusion", 32, 16, 3, &h->fusion)))
            break;
        if ((rc = find(m, P + "patch.weight", &w))) break;
        const int C = (int)w->shape[0], C2 = 2 * C;
        if (C != 128) { set_error("wgmlp: base_dim %d is not carried (the registered geometry: base_dim 128, mlp ratios 2)", C); rc = NUNIF_HIP_EUNSUPPORTED; break; }
        h->C = C; h->C2 = C2;
        if ((rc = conv_from(h, m, P + "patch", C, 16, 16, 32, 3, &h->patch))) break;
        if ((rc = find(m, P + "down1.conv.weight", &w)) || (rc = find(m, P + "down1.conv.bias", &b))) break;
        if (w->numel != (int64_t)C2 * C * 4 || b->numel != C2) { set_error("wgmlp: down1.conv shape"); rc = NUNIF_HIP_EINVAL; break; }
        {   // down1: 2x2 stride-2 conv as a gather GEMM, k = (dy*2 + dx) * C + ci
            const float *wd = w->data, *bd = b->data;
            if ((rc = make_linear(h, C2, 16, 4 * C, [=](int n, int k) { const int tap = k / C, ci = k % C; return wd[((size_t)n * C + ci) * 4 + tap]; },
                                  bias_at(bd), &h->down1)))
                break;
        }
        if ((rc = find(m, P + "up1.proj.weight", &w)) || (rc = find(m, P + "up1.proj.bias", &b))) break;
        if (w->numel != (int64_t)4 * C * C2 || b->numel != 4 * C) { set_error("wgmlp: up1.proj shape"); rc = NUNIF_HIP_EINVAL; break; }
        {   // up1: gemm mode 1 writes column n' = q * C + c to sub-pixel q: torch's pixel_shuffle takes channel c * 4 + q
            const float *wd = w->data, *bd = b->data;
            if ((rc = make_linear(h, 4 * C, 16, C2, [=](int n, int k) { const int q = n / C, c = n % C; return wd[(size_t)(c * 4 + q) * C2 + k]; },
                                  [=](int n) { const int q = n / C, c = n % C; return bd[c * 4 + q]; }, &h->up1)))
                break;
        }
        auto count_blocks = [&](const std::string &key) {
            int n = 0;
            while (m.find(key + "blocks." + std::to_string(n) + ".norm1.weight") != m.end()) ++n;
            return n;
        };
        const int n1 = count_blocks(P + "wgmlp1."), n2 = count_blocks(P + "wgmlp2."), n3 = count_blocks(P + "wgmlp3.");
        if (n1 < 1 || n2 < 1 || n3 < 1) { set_error("wgmlp: state_dict has no wgmlp1 / wgmlp2 / wgmlp3 blocks"); rc = NUNIF_HIP_EMISSING; break; }
        // get_shift_config(n) :289-295: reversed([i % 2 == 1]), i.e. block i is shifted iff (n - 1 - i) is odd
        auto shift_of = [](int n, int i) { return ((n - 1 - i) % 2) == 1 ? 1 : 0; };
        h->g1.resize(n1); h->g2.resize(n2); h->g3.resize(n3);
        for (int i = 0; i < n1 && !rc; ++i) rc = make_block(h, m, P + "wgmlp1.blocks." + std::to_string(i) + ".", C, shift_of(n1, i), true, &h->g1[i]);
        for (int i = 0; i < n2 && !rc; ++i) rc = make_block(h, m, P + "wgmlp2.blocks." + std::to_string(i) + ".", C2, shift_of(n2, i), true, &h->g2[i]);
        for (int i = 0; i < n3 && !rc; ++i)
            rc = make_block(h, m, P + "wgmlp3.blocks." + std::to_string(i) + ".", C, shift_of(n3, i), i < n3 - 1, &h->g3[i]);
        if (rc) break;
        if ((rc = linear_from(h, m, P + "to_residual_image.proj", 48, C, 16, &h->to_image))) break;
        if ((rc = find(m, P + "to_image.resampling.weight", &w)) || (rc = find(m, P + "to_image.scale_bias", &b))) break;
        if (w->numel != (int64_t)48 * 27 || b->numel != 1) { set_error("wgmlp: to_image shape"); rc = NUNIF_HIP_EINVAL; break; }
        if ((rc = h->upload_f32(w, &h->res_w)) || (rc = h->upload_f32(b, &h->scale_bias))) break;
    } while (0);
    if (rc) { nunif_hip_wgmlp_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_wgmlp_destroy(nunif_wgmlp *h) {
    if (!h) return;
    h->free_all();
    h->ws.release();
    h->dbg.release();
    delete h;
}

extern "C" int nunif_hip_wgmlp_forward(nunif_wgmlp *h, const float *x, float *z, int32_t B, int32_t T, int32_t clamp01, void *stream) {
    return forward(h, x, z, B, T, clamp01, nullptr, (hipStream_t)stream);
}

extern "C" int nunif_hip_wgmlp_debug_taps(nunif_wgmlp *h, const float *x, float *z, float *taps, int32_t B, int32_t T, int32_t clamp01,
                                          void *stream) {
    NUNIF_REQUIRE(taps, "wgmlp_debug_taps: NULL taps");
    return forward(h, x, z, B, T, clamp01, taps, (hipStream_t)stream);
}

extern "C" int nunif_hip_wgmlp_debug_gmlp(nunif_wgmlp *h, int32_t block, const float *x, float *out, int32_t B, int32_t H, int32_t W,
                                          int32_t shift, float *tap_ln1, float *tap_gelu, float *tap_ln2, float *tap_mix, float *tap_gate,
                                          void *stream) {
    NUNIF_REQUIRE(h && x && out && B > 0, "wgmlp_debug_gmlp: bad argument");
    const WgBlock *bk = block_at(h, block);
    NUNIF_REQUIRE(bk, "wgmlp_debug_gmlp: block %d of %d", block, (int)(h->g1.size() + h->g2.size() + h->g3.size()));
    NUNIF_REQUIRE(wgmlp_map_supported(H, W), "wgmlp_debug_gmlp: a %d x %d map is not whole 8 x 8 windows", H, W);
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)B * H * W * bk->C;
    int rc;
    if ((rc = h->dbg.ensure((size_t)n * sizeof(f16)))) return rc;
    f16 *m = (f16 *)h->dbg.p;
    wg_f32_to_f16_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(x, m, n);
    NUNIF_LAUNCH_CHECK();
    float *taps[5] = {tap_ln1, tap_gelu, tap_ln2, tap_mix, tap_gate};
    // without taps this is the launch of the forward (the instance without the tap stores)
    const bool any = tap_ln1 || tap_gelu || tap_ln2 || tap_mix || tap_gate;
    if ((rc = run_gmlp(*bk, m, B, H, W, shift ? 1 : 0, any ? taps : nullptr, s))) return rc;
    wg_f16_to_f32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(m, out, n);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
