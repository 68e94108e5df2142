// SOD v1 saliency estimator of iw3's auto convergence (iw3/models/sod_v1.py SODV1 = U2NETP(in_ch=6) of nunif/utils/u2netp.py,
// and iw3/convergence_estimator.py, reference) for gfx950, eval mode, BatchNorm folded, fp32 operands and accumulation.
//
// The maps are tiny (192^2 down to 6^2, 16 or 64 channels, ~115 convolutions per image): the net is bound by launch count and by
// how many lanes a 6^2 .. 24^2 map can fill, not by arithmetic, so every convolution is a direct fp32 form (one lane = one pixel x
// 8 output channels, the weights of those 8 channels uniform across the wave and read through the scalar cache) and everything
// between two convolutions is folded into the gather of the next one or the epilogue of the last one:
//   sod_entry_kernel   bilinear resize of rgb and depth to 192^2 (align_corners=False, no antialias), to_feature, the 6-channel cat
//   sod_conv_kernel    REBNCONV: 3x3, zero padding, dilation d, bias, ReLU.  Operand A is read plain, through MaxPool2d(2,2) or through
//                      the align_corners=False bilinear upsampling of _upsample_like; operand B (the second half of a torch.cat) plain;
//                      the RSU residual (hx1d + hxin) is the epilogue
//   sod_head_kernel    six side convolutions, their upsampling to 192^2, the 1x1 outconv and the sigmoid: one launch, the side values
//                      a 16x16 output tile needs staged in LDS
//   sod_depth_position_kernel   per image: radix select of the 0.1 / 0.9 quantiles of the depth under saliency > 0.5, the rule of
//                      convergence_estimator.py:41-59
//   sod_ema_kernel     the EMA across frames with resets (:69-82) on a device state
// Activations are planar [B][C][H][W] fp32.  Accumulation runs in chains of at most 16 input channels (144 products) that are then
// added to a running total: a blocked sum, like the reference's fp32 convolution, not one 1152-long chain.
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace nunif {
namespace {

constexpr int kNet = 192;            // SODV1.i2i_in_size
constexpr int kCoT = 8;              // output channels per lane
constexpr int kConvThreads = 128;
constexpr int kChain = 16;           // input channels per accumulation chain

enum { M_PLAIN = 0, M_POOL = 1, M_UP = 2 };

// ---- entry: iw3/models/sod_v1.py infer :49-56 + forward :39-41 -------------------------------------------------------------------
// source index of torch's upsample_bilinear2d, align_corners=False: src = scale * (dst + 0.5) - 0.5, clamped at 0.  Computed in
// double: for a 1080p source an fp32 coordinate carries 3e-5 of error into the interpolation weight.
__device__ __forceinline__ void bilinear_src(int dst, int in, int out, int &i0, int &i1, float &lam) {
    double s = ((double)in / (double)out) * ((double)dst + 0.5) - 0.5;
    if (s < 0.0) s = 0.0;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    lam = (float)(s - (double)i0);
}

__device__ __forceinline__ float bilerp(const float *p, int r0, int r1, int c0, int c1, float ly, float lx) {
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * p[r0 + c0] + lx * p[r0 + c1]) + ly * (hx * p[r1 + c0] + lx * p[r1 + c1]);
}

__global__ void __launch_bounds__(256) sod_entry_kernel(const float *__restrict__ rgb, const float *__restrict__ depth,
                                                        float *__restrict__ x6, float *__restrict__ depth_out, int B, int H, int W,
                                                        int h, int w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * kNet * kNet) return;
    const int b = i / (kNet * kNet), p = i - b * (kNet * kNet), y = p / kNet, x = p - y * kNet;
    int y0, y1, x0, x1;
    float ly, lx;
    bilinear_src(y, H, kNet, y0, y1, ly);
    bilinear_src(x, W, kNet, x0, x1, lx);
    float *o = x6 + (long)b * 6 * kNet * kNet + p;
    const long hw = (long)H * W;
    for (int c = 0; c < 3; ++c)
        o[(long)c * kNet * kNet] = bilerp(rgb + ((long)b * 3 + c) * hw, y0 * W, y1 * W, x0, x1, ly, lx);
    bilinear_src(y, h, kNet, y0, y1, ly);
    bilinear_src(x, w, kNet, x0, x1, lx);
    const float d = bilerp(depth + (long)b * h * w, y0 * w, y1 * w, x0, x1, ly, lx);
    o[3L * kNet * kNet] = d;                    // to_feature :31-35
    o[4L * kNet * kNet] = sqrtf(d);
    o[5L * kNet * kNet] = d * d;
    depth_out[i] = d;
}

// ---- REBNCONV (u2netp.py:11-35) ------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const float *a, *b;          // operand A [B][CA][aH][aW] (as MODE reads it), operand B [B][CB][H][W] or unused (CB = 0)
    const float *w, *bias;       // [cout/8][CA+CB][9][8], [cout]
    const float *res;            // [B][cout][H][W] added after the ReLU, or NULL
    float *out;                  // [B][cout][H][W]
    int B, H, W, CA, CB, aH, aW, dil, cout;
};

struct Taps {
    int r0[3], r1[3], c0[3], c1[3];
    float ly[3], lx[3];
    bool rok[3], cok[3];
};

template <int MODE>
__device__ __forceinline__ void make_taps(Taps &t, int y, int x, int H, int W, int aH, int aW, int dil) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int yy = y + (k - 1) * dil, xx = x + (k - 1) * dil;
        t.rok[k] = yy >= 0 && yy < H;
        t.cok[k] = xx >= 0 && xx < W;
        const int ys = t.rok[k] ? yy : 0, xs = t.cok[k] ? xx : 0;
        t.r1[k] = 0; t.c1[k] = 0; t.ly[k] = 0.f; t.lx[k] = 0.f;
        if (MODE == M_PLAIN) {
            t.r0[k] = ys * aW; t.c0[k] = xs;
        } else if (MODE == M_POOL) {                       // MaxPool2d(2, 2, ceil_mode=True) of an even map: aH = 2H, aW = 2W
            t.r0[k] = 2 * ys * aW; t.r1[k] = t.r0[k] + aW;
            t.c0[k] = 2 * xs; t.c1[k] = t.c0[k] + 1;
        } else {                                           // _upsample_like :39-41
            int i0, i1;
            bilinear_src(ys, aH, H, i0, i1, t.ly[k]);
            t.r0[k] = i0 * aW; t.r1[k] = i1 * aW;
            bilinear_src(xs, aW, W, i0, i1, t.lx[k]);
            t.c0[k] = i0; t.c1[k] = i1;
        }
    }
}

template <int MODE>
__device__ __forceinline__ float tap_value(const float *p, const Taps &t, int r, int c) {
    float v;
    if (MODE == M_PLAIN) {
        v = p[t.r0[r] + t.c0[c]];
    } else if (MODE == M_POOL) {
        v = fmaxf(fmaxf(p[t.r0[r] + t.c0[c]], p[t.r0[r] + t.c1[c]]), fmaxf(p[t.r1[r] + t.c0[c]], p[t.r1[r] + t.c1[c]]));
    } else {
        v = bilerp(p, t.r0[r], t.r1[r], t.c0[c], t.c1[c], t.ly[r], t.lx[c]);
    }
    return (t.rok[r] && t.cok[c]) ? v : 0.f;
}

// C input channels starting at plane `src` (plane stride `ps`), their weights at `w` ([ci][9][8])
template <int MODE>
__device__ __forceinline__ void accumulate(const float *src, long ps, int C, const float *w, const Taps &t, float (&tot)[kCoT]) {
    for (int c0 = 0; c0 < C; c0 += kChain) {
        float acc[kCoT];
#pragma unroll
        for (int j = 0; j < kCoT; ++j) acc[j] = 0.f;
        const int c1 = min(c0 + kChain, C);
        for (int ci = c0; ci < c1; ++ci) {
            const float *p = src + (long)ci * ps;
            const float *wc = w + (long)ci * 9 * kCoT;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = tap_value<MODE>(p, t, r, c);
#pragma unroll
                    for (int j = 0; j < kCoT; ++j) acc[j] = fmaf(v, wc[(r * 3 + c) * kCoT + j], acc[j]);
                }
        }
#pragma unroll
        for (int j = 0; j < kCoT; ++j) tot[j] += acc[j];
    }
}

template <int MODE>
__global__ void __launch_bounds__(kConvThreads) sod_conv_kernel(const ConvArgs g) {
    const int hw = g.H * g.W;
    const int i = blockIdx.x * kConvThreads + threadIdx.x;
    if (i >= g.B * hw) return;
    const int b = i / hw, p = i - b * hw, y = p / g.W, x = p - y * g.W;
    const int cog = blockIdx.y, ctot = g.CA + g.CB;
    const float *w = g.w + (long)cog * ctot * 9 * kCoT;
    float tot[kCoT];
#pragma unroll
    for (int j = 0; j < kCoT; ++j) tot[j] = g.bias[cog * kCoT + j];
    {
        Taps t;
        make_taps<MODE>(t, y, x, g.H, g.W, g.aH, g.aW, g.dil);
        const long ps = (long)g.aH * g.aW;
        accumulate<MODE>(g.a + (long)b * g.CA * ps, ps, g.CA, w, t, tot);
    }
    if (g.CB > 0) {
        Taps t;
        make_taps<M_PLAIN>(t, y, x, g.H, g.W, g.H, g.W, g.dil);
        accumulate<M_PLAIN>(g.b + (long)b * g.CB * hw, hw, g.CB, w + (long)g.CA * 9 * kCoT, t, tot);
    }
    const long o = ((long)b * g.cout + cog * kCoT) * hw + p;
#pragma unroll
    for (int j = 0; j < kCoT; ++j) {
        float v = fmaxf(tot[j], 0.f);
        if (g.res) v += g.res[o + (long)j * hw];
        g.out[o + (long)j * hw] = v;
    }
}

// ---- head: u2netp.py:406-430 ---------------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float *h[6];           // hx1d, hx2d, hx3d, hx4d, hx5d, hx6: [B][64][192>>l][192>>l]
    const float *sw, *sb;        // side weights [6][64][9], biases [6]
    const float *ow, *ob;        // outconv [6], [1]
    float *out;                  // [B][1][192][192]
};

constexpr int kHeadTile = 16;
__device__ __forceinline__ int head_n(int l) { return l == 0 ? kHeadTile : (kHeadTile >> l) + 2; }   // side values per axis and tile

__global__ void __launch_bounds__(256) sod_head_kernel(const HeadArgs g) {
    // level l of a 16x16 output tile reads side values lo_l .. lo_l + n_l - 1 per axis (n = 16, 10, 6, 4, 3, 2): 421 in all
    __shared__ float sd[421];
    __shared__ int lo[6][2];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int ty0 = blockIdx.y * kHeadTile, tx0 = blockIdx.x * kHeadTile;
    const int start[7] = {0, 256, 356, 392, 408, 417, 421};
    if (tid < 12) {
        const int l = tid >> 1, t0 = (tid & 1) ? tx0 : ty0;
        lo[l][tid & 1] = l == 0 ? t0 : (int)fmaxf(((float)t0 + 0.5f) / (float)(1 << l) - 0.5f, 0.f);
    }
    __syncthreads();
    for (int it = tid; it < 421; it += 256) {
        int l = 0;
        while (it >= start[l + 1]) ++l;
        const int n = head_n(l), e = it - start[l], S = kNet >> l;
        const int y = min(lo[l][0] + e / n, S - 1), x = min(lo[l][1] + e % n, S - 1);
        const float *src = g.h[l] + (long)b * 64 * S * S;
        const float *w = g.sw + l * 64 * 9;
        int off[9];
        bool ok[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            ok[k] = yy >= 0 && yy < S && xx >= 0 && xx < S;
            off[k] = ok[k] ? yy * S + xx : 0;
        }
        float tot = g.sb[l];
        for (int c0 = 0; c0 < 64; c0 += kChain) {
            float acc = 0.f;
            for (int ci = c0; ci < c0 + kChain; ++ci) {
                const float *p = src + (long)ci * S * S;
#pragma unroll
                for (int k = 0; k < 9; ++k) acc = fmaf(ok[k] ? p[off[k]] : 0.f, w[ci * 9 + k], acc);
            }
            tot += acc;
        }
        sd[it] = tot;
    }
    __syncthreads();
    const int ly = tid >> 4, lx = tid & 15, y = ty0 + ly, x = tx0 + lx;
    float d0 = g.ob[0] + g.ow[0] * sd[ly * kHeadTile + lx];
#pragma unroll
    for (int l = 1; l < 6; ++l) {
        const int n = head_n(l), S = kNet >> l;
        const float inv = 1.f / (float)(1 << l);
        const float sy = fmaxf(((float)y + 0.5f) * inv - 0.5f, 0.f), sx = fmaxf(((float)x + 0.5f) * inv - 0.5f, 0.f);
        const int y0 = (int)sy, x0 = (int)sx, y1 = min(y0 + 1, S - 1), x1 = min(x0 + 1, S - 1);
        const float wy = sy - (float)y0, wx = sx - (float)x0;
        const int a0 = min(y0 - lo[l][0], n - 1) * n, a1 = min(y1 - lo[l][0], n - 1) * n;
        const int b0 = min(x0 - lo[l][1], n - 1), b1 = min(x1 - lo[l][1], n - 1);
        d0 += g.ow[l] * bilerp(sd + start[l], a0, a1, b0, b1, wy, wx);
    }
    g.out[((long)b * kNet + y) * kNet + x] = 1.f / (1.f + expf(-d0));
}

// ---- depth_position_from_ratio (convergence_estimator.py:33-59) ----------------------------------------------------------------------

// One workgroup per image.  The four order statistics torch.quantile's linear interpolation needs (floor and ceil rank of q = 0.1
// and q = 0.9) are found together by a radix select over the ordered bit pattern: four passes of 8 bits, one 256-bin histogram per
// statistic in LDS.  Integer counts only: the result does not depend on the order in which lanes arrive.
__global__ void __launch_bounds__(1024) sod_depth_position_kernel(const float *__restrict__ sal, const float *__restrict__ depth,
                                                                  long n, float pos_m_half, float *__restrict__ out) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned prefix[4], krem[4], count;
    const int tid = threadIdx.x;
    const float *s = sal + (long)blockIdx.x * n, *d = depth + (long)blockIdx.x * n;
    if (tid == 0) count = 0;
    __syncthreads();
    unsigned mine = 0;
    for (long i = tid; i < n; i += 1024) mine += s[i] > 0.5f ? 1u : 0u;
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    const unsigned m = count;
    if (m == 0) {                                            // :41-45
        if (tid == 0) out[blockIdx.x] = 0.5f;
        return;
    }
    const double p1 = 0.1 * (double)(m - 1), p9 = 0.9 * (double)(m - 1);
    if (tid < 4) {
        const double pq = tid < 2 ? p1 : p9;
        krem[tid] = (unsigned)((tid & 1) ? ceil(pq) : floor(pq));
        prefix[tid] = 0;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 4 * 256; i += 1024) (&hist[0][0])[i] = 0;
        __syncthreads();
        unsigned pf[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pf[r] = prefix[r];
        // n rounded up to whole waves so that every lane of a wave takes part in the match below
        for (long i = tid; i < ((n + 63) / 64) * 64; i += 1024) {
            const bool in = i < n && s[i] > 0.5f;
            const unsigned key = in ? order_key(d[i]) : 0u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool hit = in && (shift == 24 || (key >> (shift + 8)) == (pf[r] >> (shift + 8)));
                const unsigned bin = (key >> shift) & 255u;
                // clustered depth puts a whole wave into one bin: when all its hits agree on the bin (checked against the first
                // hit lane's), one lane adds the wave's count instead of up to 64 same-address atomics
                const unsigned long long hits = __ballot(hit);
                if (hits == 0ull) continue;
                const int leader = __ffsll((long long)hits) - 1;
                const unsigned lbin = (unsigned)__shfl((int)bin, leader);
                const unsigned long long same = __ballot(hit && bin == lbin);
                if (same == hits) {
                    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[r][lbin], (unsigned)__popcll(hits));
                } else if (hit) {
                    atomicAdd(&hist[r][bin], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < 4) {
            unsigned cum = 0, k = krem[tid];
            for (int bin = 0; bin < 256; ++bin) {
                const unsigned c = hist[tid][bin];
                if (cum + c > k) {
                    prefix[tid] |= (unsigned)bin << shift;
                    krem[tid] = k - cum;
                    break;
                }
                cum += c;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float w1 = (float)(p1 - floor(p1)), w9 = (float)(p9 - floor(p9));
        const float a1 = key_value(prefix[0]), b1 = key_value(prefix[1]), a9 = key_value(prefix[2]), b9 = key_value(prefix[3]);
        const float q01 = a1 + (b1 - a1) * w1, q09 = a9 + (b9 - a9) * w9;
        const float range = q09 - q01;
        float q = q01;                                       // :50-51
        if (!(range < 1e-6f)) q = (q01 + q09) / 2.f + pos_m_half * (range * 3.0f);      // :55-57
        out[blockIdx.x] = fminf(fmaxf(q, 0.f), 1.f);
    }
}

// :69-82.  state[0] = the EMA, state[1] != 0 once it holds a value.  A reset takes effect after the frame that carries it.
__global__ void sod_ema_kernel(const float *__restrict__ z, float *__restrict__ out, int B, float *__restrict__ state, float decay,
                               float one_m_decay, unsigned long long reset_mask) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float ema = state[0];
    bool has = state[1] != 0.f;
    for (int i = 0; i < B; ++i) {
        const float p = z[i];
        ema = has ? __fadd_rn(__fmul_rn(decay, ema), __fmul_rn(one_m_decay, p)) : p;
        has = true;
        out[i] = ema;
        if ((reset_mask >> i) & 1ull) has = false;
    }
    state[0] = ema;
    state[1] = has ? 1.f : 0.f;
}

// ---- the network walk ------------------------------------------------------------------------------------------------------------------
struct Map { long off; int C, S; };                       // a [B][C][S][S] map at workspace offset `off` x B (off: floats per image)
struct Operand { Map m; int mode; };

}  // namespace
}  // namespace nunif

using namespace nunif;

// One REBNCONV launch of the plan: workspace offsets in floats per image (x B at launch), weight offsets into the device buffer.
struct Step { long a, b, res, out, w, bias; int mode, S, CA, CB, aS, dil, cout; };

struct nunif_sod_v1 {
    float *weights = nullptr;
    std::map<std::string, long> offset;
    std::map<std::string, long> count;
    // resolved once by create(): forward() issues the steps without touching a name
    std::vector<Step> steps;
    std::map<std::string, Map> taps;
    long head[6] = {0, 0, 0, 0, 0, 0};      // hx1d, hx2d, hx3d, hx4d, hx5d, hx6
    long side_w = 0, side_b = 0, out_w = 0, out_b = 0, peak = 0;
};

namespace {

// Walks U2NETP.forward once for ONE image and lays the workspace out (every offset is linear in B).  With a net it also resolves
// every tensor name and size the walk asks for and records the launches as the net's plan; without one it only measures.
struct Walk {
    nunif_sod_v1 *net;
    long top = 0, peak = 0;
    int status = NUNIF_HIP_OK;
    std::map<std::string, Map> taps;

    Map alloc(int C, int S) {
        Map m{top, C, S};
        top += (long)C * S * S;
        if (top > peak) peak = top;
        return m;
    }
    long weight(const std::string &name, long want) {
        auto it = net->offset.find(name);
        if (it == net->offset.end() || net->count.at(name) != want) {
            if (status == NUNIF_HIP_OK) set_error("sod_v1: tensor %s missing or not %ld floats", name.c_str(), want);
            status = NUNIF_HIP_EINVAL;
            return 0;
        }
        return it->second;
    }
    // REBNCONV `name` over cat(a, b) (b == nullptr: a alone) at S x S
    Map conv(const std::string &name, Operand a, const Map *b, int cout, int dil, int S, const Map *res) {
        Map o = alloc(cout, S);
        if (!net) return o;
        const int cb = b ? b->C : 0;
        Step st;
        st.w = weight(name + ".w", (long)cout * (a.m.C + cb) * 9);
        st.bias = weight(name + ".b", cout);
        st.a = a.m.off; st.b = b ? b->off : -1; st.res = res ? res->off : -1; st.out = o.off;
        st.mode = a.mode; st.S = S; st.CA = a.m.C; st.CB = cb; st.aS = a.m.S; st.dil = dil; st.cout = cout;
        const bool shape_ok = (a.mode == M_PLAIN && a.m.S == S) || (a.mode == M_POOL && a.m.S == 2 * S) || (a.mode == M_UP && a.m.S >= 1);
        if (!shape_ok || cout % kCoT != 0 || (b && b->S != S) || (res && (res->S != S || res->C != cout))) {
            if (status == NUNIF_HIP_OK) set_error("sod_v1: %s: operand geometry", name.c_str());
            status = NUNIF_HIP_EINVAL;
        }
        net->steps.push_back(st);
        return o;
    }
    // RSU7 / RSU6 / RSU5 / RSU4 (L = 7..4, u2netp.py:44-284) and RSU4F (L = 0, :287-318) at S x S.  The result is laid out first and
    // the maps inside the block after it, so that they are released on return and the result stays.
    Map rsu(const std::string &p, int L, Operand in, const Map *in_b, int S) {
        const Map result = alloc(64, S);
        const long mark = top;
        auto last = [&](Operand a, const Map *b, const Map *res) {       // rebnconv1d + hxin, written into `result`
            const long keep = top;
            top = result.off;
            conv(p + ".rebnconv1d", a, b, 64, 1, S, res);
            top = keep;
        };
        const Map hxin = conv(p + ".rebnconvin", in, in_b, 64, 1, S, nullptr);
        if (L == 0) {
            const Map h1 = conv(p + ".rebnconv1", {hxin, M_PLAIN}, nullptr, 16, 1, S, nullptr);
            const Map h2 = conv(p + ".rebnconv2", {h1, M_PLAIN}, nullptr, 16, 2, S, nullptr);
            const Map h3 = conv(p + ".rebnconv3", {h2, M_PLAIN}, nullptr, 16, 4, S, nullptr);
            const Map h4 = conv(p + ".rebnconv4", {h3, M_PLAIN}, nullptr, 16, 8, S, nullptr);
            const Map h3d = conv(p + ".rebnconv3d", {h4, M_PLAIN}, &h3, 16, 4, S, nullptr);
            const Map h2d = conv(p + ".rebnconv2d", {h3d, M_PLAIN}, &h2, 16, 2, S, nullptr);
            last({h2d, M_PLAIN}, &h1, &hxin);
        } else {
            std::vector<Map> h(L + 1);
            h[1] = conv(p + ".rebnconv1", {hxin, M_PLAIN}, nullptr, 16, 1, S, nullptr);
            for (int i = 2; i < L; ++i)
                h[i] = conv(p + ".rebnconv" + std::to_string(i), {h[i - 1], M_POOL}, nullptr, 16, 1, S >> (i - 1), nullptr);
            h[L] = conv(p + ".rebnconv" + std::to_string(L), {h[L - 1], M_PLAIN}, nullptr, 16, 2, S >> (L - 2), nullptr);
            Map d = conv(p + ".rebnconv" + std::to_string(L - 1) + "d", {h[L], M_PLAIN}, &h[L - 1], 16, 1, S >> (L - 2), nullptr);
            for (int i = L - 2; i >= 2; --i)
                d = conv(p + ".rebnconv" + std::to_string(i) + "d", {d, M_UP}, &h[i], 16, 1, S >> (i - 1), nullptr);
            last({d, M_UP}, &h[1], &hxin);
        }
        top = mark;
        return result;
    }

    // U2NETP.forward :364-430.  x6 / depth / saliency live outside the walk's own maps only in that the caller names them.
    Map x6, hx[7], hxd[6];
    void net_maps() {
        x6 = alloc(6, kNet);
        hx[1] = rsu("stage1", 7, {x6, M_PLAIN}, nullptr, 192);
        hx[2] = rsu("stage2", 6, {hx[1], M_POOL}, nullptr, 96);
        hx[3] = rsu("stage3", 5, {hx[2], M_POOL}, nullptr, 48);
        hx[4] = rsu("stage4", 4, {hx[3], M_POOL}, nullptr, 24);
        hx[5] = rsu("stage5", 0, {hx[4], M_POOL}, nullptr, 12);
        hx[6] = rsu("stage6", 0, {hx[5], M_POOL}, nullptr, 6);
        hxd[5] = rsu("stage5d", 0, {hx[6], M_UP}, &hx[5], 12);
        hxd[4] = rsu("stage4d", 4, {hxd[5], M_UP}, &hx[4], 24);
        hxd[3] = rsu("stage3d", 5, {hxd[4], M_UP}, &hx[3], 48);
        hxd[2] = rsu("stage2d", 6, {hxd[3], M_UP}, &hx[2], 96);
        hxd[1] = rsu("stage1d", 7, {hxd[2], M_UP}, &hx[1], 192);
        for (int i = 1; i <= 6; ++i) taps["hx" + std::to_string(i)] = hx[i];
        taps["hx1d"] = hxd[1];
    }
};

int launch_entry(const float *rgb, int H, int W, const float *depth, int h, int w, int B, float *x6, float *depth_scaled,
                 hipStream_t s) {
    NUNIF_REQUIRE(rgb && depth && x6 && depth_scaled, "sod_v1: NULL argument");
    NUNIF_REQUIRE(B > 0 && B <= 1024 && H > 0 && W > 0 && h > 0 && w > 0 && (long)H * W < (1L << 30) && (long)h * w < (1L << 30),
                  "sod_v1: bad shape B=%d rgb %dx%d depth %dx%d", B, H, W, h, w);
    sod_entry_kernel<<<cdiv(B * kNet * kNet, 256), 256, 0, s>>>(rgb, depth, x6, depth_scaled, B, H, W, h, w);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

}  // namespace

extern "C" int nunif_hip_sod_v1_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t net_size,
                                       nunif_sod_v1 **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "sod_v1_create: NULL argument");
    if (net_size != kNet) {
        // MaxPool2d(ceil_mode=True) is built for even maps only: 192 halves evenly down to 6
        set_error("sod_v1_create: net size %d is not built (only %d)", net_size, kNet);
        return NUNIF_HIP_EUNSUPPORTED;
    }
    nunif_sod_v1 *net = new nunif_sod_v1();
    long total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        long n = 1;
        for (int k = 0; k < tensors[i].ndim; ++k) n *= tensors[i].shape[k];
        net->offset[tensors[i].name] = total;
        net->count[tensors[i].name] = n;
        total += (n + 3) / 4 * 4;
    }
    std::vector<float> host(total, 0.f);
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].data) {
            delete net;
            set_error("sod_v1_create: tensor %s has no data", tensors[i].name);
            return NUNIF_HIP_EINVAL;
        }
        const float *src = static_cast<const float *>(tensors[i].data);
        std::copy(src, src + net->count[tensors[i].name], host.begin() + net->offset[tensors[i].name]);
    }
    // the plan: every tensor name and size the walk asks for is resolved here, so a wrong set of tensors fails in create()
    Walk wk{net};
    wk.net_maps();
    net->side_w = wk.weight("side.w", 6 * 64 * 9);
    net->side_b = wk.weight("side.b", 6);
    net->out_w = wk.weight("outconv.w", 6);
    net->out_b = wk.weight("outconv.b", 1);
    if (wk.status != NUNIF_HIP_OK) {
        delete net;
        return NUNIF_HIP_EINVAL;
    }
    for (int l = 0; l < 5; ++l) net->head[l] = wk.hxd[l + 1].off;
    net->head[5] = wk.hx[6].off;
    net->taps = wk.taps;
    net->peak = wk.peak;
    if (hipMalloc(&net->weights, (size_t)total * sizeof(float)) != hipSuccess ||
        hipMemcpy(net->weights, host.data(), (size_t)total * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        if (net->weights) (void)hipFree(net->weights);
        delete net;
        set_error("sod_v1_create: uploading the weights failed");
        return NUNIF_HIP_EHIP;
    }
    *handle = net;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_sod_v1_destroy(nunif_sod_v1 *handle) {
    if (!handle) return;
    if (handle->weights) (void)hipFree(handle->weights);
    delete handle;
}

extern "C" int64_t nunif_hip_sod_v1_workspace_floats(int32_t B) {
    if (B <= 0) return 0;
    // the walk releases an RSU's inner maps on return; its high-water mark per image is what a call needs, times B
    static const long peak = [] { Walk wk{nullptr}; wk.net_maps(); return wk.peak; }();
    return (int64_t)peak * B;
}

extern "C" int nunif_hip_sod_v1_entry(const float *rgb, int32_t H, int32_t W, const float *depth, int32_t h, int32_t w, int32_t B,
                                      float *x6, float *depth_scaled, void *stream) {
    return launch_entry(rgb, H, W, depth, h, w, B, x6, depth_scaled, (hipStream_t)stream);
}

extern "C" int nunif_hip_sod_v1_forward(nunif_sod_v1 *handle, const float *rgb, int32_t H, int32_t W, const float *depth,
                                        int32_t h, int32_t w, int32_t B, float *workspace, float *saliency, float *depth_scaled,
                                        void *stream) {
    NUNIF_REQUIRE(handle && workspace && saliency, "sod_v1_forward: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("sod_v1", s, 0.0, 0.0);
    const int st = launch_entry(rgb, H, W, depth, h, w, B, workspace, depth_scaled, s);      // x6 is the plan's first map
    if (st != NUNIF_HIP_OK) return st;
    const float *wt = handle->weights;
    for (const Step &p : handle->steps) {
        ConvArgs g;
        g.a = workspace + p.a * B; g.b = p.b >= 0 ? workspace + p.b * B : nullptr; g.res = p.res >= 0 ? workspace + p.res * B : nullptr;
        g.out = workspace + p.out * B; g.w = wt + p.w; g.bias = wt + p.bias;
        g.B = B; g.H = p.S; g.W = p.S; g.CA = p.CA; g.CB = p.CB; g.aH = p.aS; g.aW = p.aS; g.dil = p.dil; g.cout = p.cout;
        const dim3 grid(cdiv(B * p.S * p.S, kConvThreads), p.cout / kCoT);
        if (p.mode == M_PLAIN) sod_conv_kernel<M_PLAIN><<<grid, kConvThreads, 0, s>>>(g);
        else if (p.mode == M_POOL) sod_conv_kernel<M_POOL><<<grid, kConvThreads, 0, s>>>(g);
        else sod_conv_kernel<M_UP><<<grid, kConvThreads, 0, s>>>(g);
        NUNIF_LAUNCH_CHECK();
    }
    HeadArgs g;
    for (int l = 0; l < 6; ++l) g.h[l] = workspace + handle->head[l] * B;
    g.sw = wt + handle->side_w; g.sb = wt + handle->side_b; g.ow = wt + handle->out_w; g.ob = wt + handle->out_b;
    g.out = saliency;
    sod_head_kernel<<<dim3(kNet / kHeadTile, kNet / kHeadTile, B), 256, 0, s>>>(g);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_sod_v1_debug_taps(nunif_sod_v1 *handle, const float *workspace, int32_t B, const char *name, float *out,
                                           int64_t capacity, int64_t *shape4, void *stream) {
    NUNIF_REQUIRE(handle && workspace && name && out && shape4 && B > 0, "sod_v1_debug_taps: bad argument");
    auto it = handle->taps.find(name);
    NUNIF_REQUIRE(it != handle->taps.end(), "sod_v1_debug_taps: no tap named %s", name);
    const Map m = it->second;
    const int64_t n = (int64_t)B * m.C * m.S * m.S;
    NUNIF_REQUIRE(capacity >= n, "sod_v1_debug_taps: %s needs %lld floats", name, (long long)n);
    shape4[0] = B; shape4[1] = m.C; shape4[2] = m.S; shape4[3] = m.S;
    NUNIF_HIP_CHECK(hipMemcpyAsync(out, workspace + m.off * B, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_sod_v1_depth_position(const float *saliency, const float *depth, int32_t B, int64_t n, double pos,
                                               float *out, void *stream) {
    NUNIF_REQUIRE(saliency && depth && out && B > 0 && n > 0 && n < (1LL << 31), "sod_v1_depth_position: bad argument");
    sod_depth_position_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(saliency, depth, (long)n, (float)(pos - 0.5), out);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_sod_v1_ema(const float *z, float *out, int32_t B, float *state, double decay, uint64_t reset_mask,
                                    void *stream) {
    NUNIF_REQUIRE(z && out && state && B > 0 && B <= 64, "sod_v1_ema: bad argument (1 <= B <= 64)");
    sod_ema_kernel<<<1, 64, 0, (hipStream_t)stream>>>(z, out, B, state, (float)decay, (float)(1.0 - decay), reset_mask);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
