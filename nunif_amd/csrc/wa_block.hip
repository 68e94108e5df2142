// Device half of the WABlock (wa_block.h): the two window-attention kernels, the upload of a block's arrays and the block loop.
//
// Reference: nunif/modules/attention.py — WindowMHA2d :118-161, MHA :94-115, sliced_sdp :61-77 (float score bias),
// WindowScoreBias :375-419; WABlock in iw3/models/row_flow_v3.py :14-30, mlbw.py, depth_aa.py :11-26.
//   wmha_kernel<WS,C>  per window of WS x WS <= 16 tokens: qkv GEMM, C/32 heads of 32 with the learned score bias, head_proj,
//                      residual — everything after the x gather in registers (same operand tricks as swin_qkv_attn_r.hip)
//   wmha8_kernel       one 8x8 window per wave, C = 32: qkv GEMM, 2 heads of 16 x (4x4 score tiles with the learned 64x64 bias as
//                      the MFMA C operand, softmax over 64 keys, PV), head_proj, residual — all in registers
#include <algorithm>
#include <cstring>

#include "swin_kernels.h"
#include "wa_block.h"
#include "wa_block_host.h"

namespace nunif {

struct WmhaArgs {
    f16 *x;                  // [B,H,W,C], updated in place: x += head_proj(attention(x))
    const f16 *wfrag;        // 3*NT*KS qkv fragments (part, nt, ks) + NT*KS head_proj fragments (nt, ks; chained k order)
    const float *bqkv;       // [3C] (q part pre-scaled by hd^-0.5 * log2e)
    const float *bproj;      // [C]
    const float *btab;       // [16][16] log2e * score bias [query][key]; -1e30 for keys beyond the window
    int B, H, W, n_windows;
    int sy, sx;              // WindowMHA2d shift: the map is ZERO-padded by (sy, sx) on both sides, windows tile the
                             // padded map, padded positions act as (all-zero input) tokens and are cropped away again
};

// One window (WS x WS <= 16 tokens = one MFMA tile) per wave; C channels = C/32 heads of 32; weights resident in LDS.
template <int WS, int C>
__global__ void __launch_bounds__(256) wmha_kernel(WmhaArgs a) {
    constexpr int N = WS * WS, KS = C / 32, NT = C / 16, HEADS = C / 32;
    constexpr int NF = 4 * NT * KS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_w[];
    f16x8 *wl = reinterpret_cast<f16x8 *>(smem_w);                                  // [NF][64]
    float *tb = reinterpret_cast<float *>(wl + NF * 64);                            // [256]
    float *bq = tb + 256;                                                           // [3C]
    float *bp = bq + 3 * C;                                                         // [C]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, grp = lane >> 4;
    for (int i = tid; i < NF * 64; i += 256) wl[i] = reinterpret_cast<const f16x8 *>(a.wfrag)[i];
    tb[tid] = a.btab[tid];
    for (int i = tid; i < 3 * C; i += 256) bq[i] = a.bqkv[i];
    for (int i = tid; i < C; i += 256) bp[i] = a.bproj[i];
    __syncthreads();
    const f16x4 zero4 = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
    const f16x8 zero8 = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
    const int nwx = (a.W + 2 * a.sx) / WS, nwy = (a.H + 2 * a.sy) / WS;
    const int tt = min(r16, N - 1);
    const int iy = tt / WS, ix = tt - iy * WS;
    const f16x8 *wq = wl + lane;

    for (int wi = blockIdx.x * 4 + wave; wi < a.n_windows; wi += gridDim.x * 4) {
        const int wx = wi % nwx, t2 = wi / nwx;
        const int wy = t2 % nwy, b = t2 / nwy;
        const int y = wy * WS + iy - a.sy, x = wx * WS + ix - a.sx;
        const bool inside = y >= 0 && y < a.H && x >= 0 && x < a.W;
        const long pix = ((long)b * a.H + min(max(y, 0), a.H - 1)) * a.W + min(max(x, 0), a.W - 1);
        f16x8 xf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            xf[ks] = inside ? *reinterpret_cast<const f16x8 *>(a.x + pix * C + ks * 32 + 8 * grp) : zero8;
        // q, k: [channel 4g+r of tile nt][token l&15];  v (operands swapped): [token 4g+r][channel l&15 of tile nt]
        f16x4 q4[NT], k4[NT], v4[NT];
#pragma unroll
        for (int part = 0; part < 3; ++part)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ch0 = part * C + nt * 16;
                f32x4 acc;
                if (part == 2) { const float bv = bq[ch0 + r16]; acc = (f32x4){bv, bv, bv, bv}; }
                else acc = *reinterpret_cast<const f32x4 *>(bq + ch0 + 4 * grp);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const f16x8 w = wq[((part * NT + nt) * KS + ks) * 64];
                    acc = part == 2 ? MFMA_16x16x32(xf[ks], w, acc) : MFMA_16x16x32(w, xf[ks], acc);
                }
                const f16x4 v = {(f16)acc[0], (f16)acc[1], (f16)acc[2], (f16)acc[3]};
                if (part == 0) q4[nt] = v; else if (part == 1) k4[nt] = v; else v4[nt] = v;
            }
        // heads of 32 channels: S^T[key][query] = K Q^T + bias; softmax over keys; O^T = V^T P^T
        f16x4 o4[NT];
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(tb + r16 * 16 + 4 * grp);          // [query l&15][keys 4g..]
#pragma unroll
        for (int hh = 0; hh < HEADS; ++hh) {
            f32x4 s = MFMA_16x16x32(cat8(k4[2 * hh], k4[2 * hh + 1]), cat8(q4[2 * hh], q4[2 * hh + 1]), bias);
            float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float p0 = __builtin_amdgcn_exp2f(s[0] - mx), p1 = __builtin_amdgcn_exp2f(s[1] - mx);
            const float p2 = __builtin_amdgcn_exp2f(s[2] - mx), p3 = __builtin_amdgcn_exp2f(s[3] - mx);
            float sum = (p0 + p1) + (p2 + p3);
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            const float inv = 1.0f / sum;
            const f16x8 pf = cat8((f16x4){(f16)p0, (f16)p1, (f16)p2, (f16)p3}, zero4);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                o = MFMA_16x16x32(cat8(v4[2 * hh + dt], zero4), pf, o);
                o4[2 * hh + dt] = (f16x4){(f16)(o[0] * inv), (f16)(o[1] * inv), (f16)(o[2] * inv), (f16)(o[3] * inv)};
            }
        }
        // head_proj (weights packed in the chained k order: two accumulator tiles = one 32-wide k-step) + residual
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f32x4 acc = *reinterpret_cast<const f32x4 *>(bp + nt * 16 + 4 * grp);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                acc = MFMA_16x16x32(wq[(3 * NT * KS + nt * KS + ks) * 64], cat8(o4[2 * ks], o4[2 * ks + 1]), acc);
            if (inside && r16 < N) {
                f16 *px = a.x + pix * C + nt * 16 + 4 * grp;
                const f16x4 xr = *reinterpret_cast<const f16x4 *>(px);
                const f16x4 ov = {(f16)(acc[0] + (float)xr[0]), (f16)(acc[1] + (float)xr[1]), (f16)(acc[2] + (float)xr[2]),
                                  (f16)(acc[3] + (float)xr[3])};
                *reinterpret_cast<f16x4 *>(px) = ov;
            }
        }
    }
}

struct Wmha8Args {
    f16 *x;                   // [B,H,W,32] in place
    const f16 *wfrag;         // 6 qkv fragments (part*2 + head) + 2 head_proj fragments (chained k order)
    const float *bqkv;        // [96]  (q pre-scaled by 16^-0.5 * log2e)
    const float *bproj;       // [32]
    const float *btab;        // [64][64] log2e * score bias [query][key]
    int B, H, W, n_windows, shift;   // shift: 0 or 4 (zero padding on all four sides)
};

__global__ void __launch_bounds__(256) wmha8_kernel(Wmha8Args a) {
    __shared__ __attribute__((aligned(16))) f16x8 wl[8 * 64];
    __shared__ __attribute__((aligned(16))) float tb[64 * 64], bq[96], bp[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, grp = lane >> 4;
    for (int i = tid; i < 8 * 64; i += 256) wl[i] = reinterpret_cast<const f16x8 *>(a.wfrag)[i];
    for (int i = tid; i < 64 * 64; i += 256) tb[i] = a.btab[i];
    if (tid < 96) bq[tid] = a.bqkv[tid];
    if (tid < 32) bp[tid] = a.bproj[tid];
    __syncthreads();
    const f16x4 zero4 = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
    const f16x8 zero8 = cat8(zero4, zero4);
    const int nwx = (a.W + 2 * a.shift) / 8, nwy = (a.H + 2 * a.shift) / 8;
    const f16x8 *wq = wl + lane;

    for (int wi = blockIdx.x * 4 + wave; wi < a.n_windows; wi += gridDim.x * 4) {
        const int wx = wi % nwx, t2 = wi / nwx;
        const int wy = t2 % nwy, b = t2 / nwy;
        // token tile mt holds window tokens 16 mt + r16 = rows 2 mt, 2 mt + 1 of the 8x8 window
        long pix[4];
        bool inside[4];
        f16x8 xf[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int t = 16 * mt + r16;
            const int y = wy * 8 + (t >> 3) - a.shift, x = wx * 8 + (t & 7) - a.shift;
            inside[mt] = y >= 0 && y < a.H && x >= 0 && x < a.W;
            pix[mt] = ((long)b * a.H + min(max(y, 0), a.H - 1)) * a.W + min(max(x, 0), a.W - 1);
            xf[mt] = inside[mt] ? *reinterpret_cast<const f16x8 *>(a.x + pix[mt] * 32 + 8 * grp) : zero8;
        }
        f16x4 o4[2][4];                                         // [head][query tile]: channels 4g+r of the head
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            // q, k: [channel 4g+r][token];  v (operands swapped): [token 4g+r][channel l&15]
            f16x4 q4[4], k4[4], v4[4];
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                const int ch0 = part * 32 + hh * 16;
                const f16x8 w = wq[(part * 2 + hh) * 64];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    f32x4 acc;
                    if (part == 2) { const float bv = bq[ch0 + r16]; acc = (f32x4){bv, bv, bv, bv}; }
                    else acc = *reinterpret_cast<const f32x4 *>(bq + ch0 + 4 * grp);
                    acc = part == 2 ? MFMA_16x16x32(xf[mt], w, acc) : MFMA_16x16x32(w, xf[mt], acc);
                    const f16x4 v = {(f16)acc[0], (f16)acc[1], (f16)acc[2], (f16)acc[3]};
                    if (part == 0) q4[mt] = v; else if (part == 1) k4[mt] = v; else v4[mt] = v;
                }
            }
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                // S^T[key][query] for the 4 key tiles; the learned bias [query][key] is the accumulator's initial value
                f32x4 s[4];
                float mx = -3.0e38f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const f32x4 bias = *reinterpret_cast<const f32x4 *>(tb + (16 * qt + r16) * 64 + 16 * kt + 4 * grp);
                    s[kt] = MFMA_16x16x32(cat8(k4[kt], zero4), cat8(q4[qt], zero4), bias);
                    mx = fmaxf(mx, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
                }
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                float sum = 0.f;
                f16x4 p[4];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const float p0 = __builtin_amdgcn_exp2f(s[kt][0] - mx), p1 = __builtin_amdgcn_exp2f(s[kt][1] - mx);
                    const float p2 = __builtin_amdgcn_exp2f(s[kt][2] - mx), p3 = __builtin_amdgcn_exp2f(s[kt][3] - mx);
                    sum += (p0 + p1) + (p2 + p3);
                    p[kt] = (f16x4){(f16)p0, (f16)p1, (f16)p2, (f16)p3};
                }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                o = MFMA_16x16x32(cat8(v4[0], v4[1]), cat8(p[0], p[1]), o);
                o = MFMA_16x16x32(cat8(v4[2], v4[3]), cat8(p[2], p[3]), o);
                o4[hh][qt] = (f16x4){(f16)(o[0] * inv), (f16)(o[1] * inv), (f16)(o[2] * inv), (f16)(o[3] * inv)};
            }
        }
        // head_proj: K = 32 = [head 0's 16 channels | head 1's 16 channels] in the chained slot order
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 acc = *reinterpret_cast<const f32x4 *>(bp + nt * 16 + 4 * grp);
                acc = MFMA_16x16x32(wq[(6 + nt) * 64], cat8(o4[0][mt], o4[1][mt]), acc);
                if (inside[mt]) {
                    f16 *px = a.x + pix[mt] * 32 + nt * 16 + 4 * grp;
                    const f16x4 xr = *reinterpret_cast<const f16x4 *>(px);
                    *reinterpret_cast<f16x4 *>(px) = (f16x4){(f16)(acc[0] + (float)xr[0]), (f16)(acc[1] + (float)xr[1]),
                                                             (f16)(acc[2] + (float)xr[2]), (f16)(acc[3] + (float)xr[3])};
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int WS, int C>
static int launch_wmha_t(const WmhaArgs &a, hipStream_t s) {
    constexpr size_t smem = (size_t)4 * (C / 16) * (C / 32) * 1024 + 256 * 4 + 4 * C * 4;
    static bool configured = false;
    if (!configured) {
        NUNIF_HIP_CHECK(hipFuncSetAttribute((const void *)wmha_kernel<WS, C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        configured = true;
    }
    const int grid = std::min((a.n_windows + 3) / 4, C == 64 ? 2048 : 256);
    wmha_kernel<WS, C><<<grid, 256, smem, s>>>(a);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

static int launch_wmha(WmhaArgs a, int window, int C, hipStream_t s) {
    NUNIF_REQUIRE((a.H + 2 * a.sy) % window == 0 && (a.W + 2 * a.sx) % window == 0, "window attention: %dx%d (+%d,%d) is not "
                  "a multiple of the %dx%d window", a.H, a.W, a.sy, a.sx, window, window);
    a.n_windows = a.B * ((a.H + 2 * a.sy) / window) * ((a.W + 2 * a.sx) / window);
    const double tok = (double)a.B * a.H * a.W, flops = tok * (8.0 * C * C + 4.0 * window * window * C), bytes = tok * C * 4.0;
    if (window == 4 && C == 64) { ProfScope ps("wmha_kernel<4,64>", s, flops, bytes); return launch_wmha_t<4, 64>(a, s); }
    if (window == 3 && C == 64) { ProfScope ps("wmha_kernel<3,64>", s, flops, bytes); return launch_wmha_t<3, 64>(a, s); }
    if (window == 4 && C == 128) { ProfScope ps("wmha_kernel<4,128>", s, flops, bytes); return launch_wmha_t<4, 128>(a, s); }
    if (window == 8 && C == 32 && a.sy == a.sx) {
        Wmha8Args a8;
        a8.x = a.x; a8.wfrag = a.wfrag; a8.bqkv = a.bqkv; a8.bproj = a.bproj; a8.btab = a.btab;
        a8.B = a.B; a8.H = a.H; a8.W = a.W; a8.n_windows = a.n_windows; a8.shift = a.sy;
        ProfScope ps("wmha8_kernel", s, flops, bytes);
        wmha8_kernel<<<std::min((a.n_windows + 3) / 4, 2048), 256, 0, s>>>(a8);
        NUNIF_LAUNCH_CHECK();
        return NUNIF_HIP_OK;
    }
    set_error("window attention: window %d / %d channels unsupported", window, C);
    return NUNIF_HIP_EUNSUPPORTED;
}

int make_wa_block(DeviceOwner *h, const TensorMap &m, const std::string &p, int window, int C, int hd, WaBlock *bk) {
    WaBlockHost b;
    int rc;
    if ((rc = wa_block_pack(m, p, window, C, hd, window == 8 ? 64 : 16, &b))) return rc;
    bk->window = window;
    if ((rc = h->upload(b.wfrag, &bk->wfrag)) || (rc = h->upload(b.bqkv, &bk->bqkv)) || (rc = h->upload(b.bproj, &bk->bproj)) ||
        (rc = h->upload(b.btab, &bk->btab)) || (rc = h->upload(b.w1, &bk->mlp1.w)) || (rc = h->upload(b.b1, &bk->mlp1.bias)) ||
        (rc = h->upload(b.w3, &bk->mlp3.stream)))
        return rc;
    bk->mlp1.N = bk->mlp1.n_real = bk->mlp1.K = C;
    bk->mlp3.N = bk->mlp3.n_real = bk->mlp3.Cin = C;
    return h->upload(b.b3, &bk->mlp3.bias);
}

int run_wa_blocks(WaMaps *h, const WaBlock *blk, int n, const int *sy, const int *sx, int C, int B, int H, int W, int act, float slope,
                  const char *tag, hipStream_t s, f16 **out) {
    f16 *cur = (f16 *)h->f.p, *t1 = (f16 *)h->t1.p, *other = (f16 *)h->t2.p;
    int rc;
    for (int bi = 0; bi < n; ++bi) {
        const WaBlock &bk = blk[bi];
        {
            WmhaArgs a;
            memset(&a, 0, sizeof(a));
            a.x = cur; a.wfrag = bk.wfrag; a.bqkv = bk.bqkv; a.bproj = bk.bproj; a.btab = bk.btab;
            a.B = B; a.H = H; a.W = W; a.sy = sy[bi]; a.sx = sx[bi];
            if ((rc = launch_wmha(a, bk.window, C, s))) return rc;
        }
        GemmArgs g = gemm_map_args(bk.mlp1, cur, B, H, W, C, H, W, t1);      // conv_mlp[0..1]: 1x1 + GELU(erf)
        g.act = 1;
        if ((rc = launch_gemm(g, s, tag))) return rc;
        // conv_mlp[2..4]: ReplicationPad2d(1) + 3x3 + the net's activation, then the block's residual
        ConvArgs c = conv_args(bk.mlp3, t1, B, H, W, other, 1, 0, 1);
        c.act = act; c.slope = slope; c.res = cur;
        if ((rc = launch_conv(c, s))) return rc;
        std::swap(cur, other);
    }
    *out = cur;
    return NUNIF_HIP_OK;
}

}  // namespace nunif
