// cliqa's three image-quality nets (cliqa/models/jpeg_quality.py JPEGQuality :8-75, grain_noise_level.py GrainNoiseLevel :8-58,
// scale_factor.py ScaleFactor :10-63, reference) and the patch selection of cliqa/utils.py extract_patches :36-57 for gfx950.
// Eval mode, BatchNorm folded on the host (nunif_amd/cliqa/models pack_weights), fp16 operands on v_mfma_f32_16x16x32_f16 with
// fp32 accumulation (the reference runs these nets under fp16 autocast, cliqa/utils.py:65,78,91), NHWC fp16 maps in HBM.
//
// One forward of a group of images is eight launches:
//   cliqa_entry_kernel      preprocess (YCbCr + RGB concat for the JPEG net, x * 2 - 1) + conv Cin -> 64, REPLICATE pad, + ReLU
//   cliqa_conv_pool_kernel  conv 64 -> 128, zero pad, + ReLU + MaxPool2d(2) (floor: an odd row / column is dropped)
//   launch_conv             ResBlock conv 1, 128 -> 128 + ReLU: the library's 3x3 conv (cunet_kernels.hip / conv3_lds.hip), reused
//   cliqa_conv_pool_kernel  ResBlock conv 2 + shortcut + ReLU (res_block.py:76-77) + MaxPool2d(2)
//   (the last two once more for the second ResBlock)
//   cliqa_head_kernel       per head: conv 128 -> 256 + ReLU, reduced per tile and channel to a max or a sum; the two heads of the
//                           JPEG net share one staged input tile; no 256-channel map is written
//   cliqa_head_final_kernel the tiles' partials in tile order (no atomics), the mean's division, the 1x1 conv, ScaleFactor's clamp
// Operand orientation as in the cunet kernels: weights are MFMA operand A (host_weights.h fragments, [k-step][n-tile] stream,
// k = tap * Cin + ci), activations operand B, so an accumulator lane holds 4 consecutive output channels of one pixel.
// A workgroup (4 waves) owns an 8 x 16 tile of conv outputs and all output channels of a pass (128): wave w owns rows 2w, 2w + 1,
// which are exactly one pooled row, so the vertical half of the pool is lane-local and the horizontal half one lane exchange.
// The input tile with its halo is staged in LDS once; the weights of a k-step (8 fragments, 8 KiB) go through a two-slot LDS ring
// shared by the four waves, requested one k-step ahead into registers.
#include <vector>

#include "cliqa_host.h"
#include "swin_kernels.h"

namespace nunif {
namespace {

using cliqa_host::kTH;                           // conv outputs per workgroup: 8 rows x 16 columns (cliqa_host.h)
using cliqa_host::kTW;
constexpr int kHH = kTH + 2, kHW = kTW + 2;      // with the halo
constexpr int kChunk = 512;                      // f16x8 items of one k-step of 8 fragments
constexpr int kMaxPatches = 4096;                // patches of one image the selection ranks in LDS

enum { KIND_JPEG = 0, KIND_GRAIN = 1, KIND_SCALE = 2 };

// ---- entry ---------------------------------------------------------------------------------------------------------------------------
// K = 9 taps x 8 channel slots (6 or 3 used) = 72, padded to 96: k-step ks, lane group g read tap 4 ks + g, slots = channels.
struct EntryArgs {
    const float *x;            // [G][3][H][W]
    const f16 *w;              // 3 k-steps x 4 n-tiles
    const float *bias;         // [64]
    f16 *out;                  // [G][H][W][64]
    int H, W, tiles_x, jpeg;
};

__global__ void __launch_bounds__(256) cliqa_entry_kernel(const EntryArgs g) {
    __shared__ __attribute__((aligned(16))) f16 halo[kHH * kHW * 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, grp = lane >> 4;
    const int ty0 = ((int)blockIdx.x / g.tiles_x) * kTH, tx0 = ((int)blockIdx.x % g.tiles_x) * kTW;
    const long hw = (long)g.H * g.W;
    const float *img = g.x + (long)blockIdx.y * 3 * hw;
    if (tid < kHH * kHW) {
        const int hy = tid / kHW, hx = tid - hy * kHW;
        const int y = min(max(ty0 + hy - 1, 0), g.H - 1), x = min(max(tx0 + hx - 1, 0), g.W - 1);      // replicate
        const float r = img[(long)y * g.W + x], gg = img[hw + (long)y * g.W + x], b = img[2 * hw + (long)y * g.W + x];
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (g.jpeg) {                                          // jpeg_quality.py:57-68
            const float yy = r * 0.299f + gg * 0.587f + b * 0.114f;
            v[0] = yy; v[1] = (b - yy) * 0.564f + 0.5f; v[2] = (r - yy) * 0.713f + 0.5f;
            v[3] = r; v[4] = gg; v[5] = b;
#pragma unroll
            for (int c = 0; c < 6; ++c) v[c] = v[c] * 2.f - 1.f;
        } else {
            v[0] = r * 2.f - 1.f; v[1] = gg * 2.f - 1.f; v[2] = b * 2.f - 1.f;
        }
        f16x8 h;
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = (f16)v[c];
        *reinterpret_cast<f16x8 *>(halo + tid * 8) = h;
    }
    __syncthreads();
    f32x4 acc[4][2];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[nt][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f16x8 *wf = reinterpret_cast<const f16x8 *>(g.w);
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
        const int tap = min(ks * 4 + grp, 8);                  // taps 9 .. 11 carry zero weights: any finite value will do
        const int dy = tap / 3, dx = tap - dy * 3;
        f16x8 xv[2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
            xv[f] = *reinterpret_cast<const f16x8 *>(halo + ((2 * wave + f + dy) * kHW + r16 + dx) * 8);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const f16x8 w = wf[(ks * 4 + nt) * 64 + lane];
#pragma unroll
            for (int f = 0; f < 2; ++f) acc[nt][f] = MFMA_16x16x32(w, xv[f], acc[nt][f]);
        }
    }
    const int ox = tx0 + r16;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int oy = ty0 + 2 * wave + f;
        if (oy >= g.H || ox >= g.W) continue;
        f16 *o = g.out + (((long)blockIdx.y * g.H + oy) * g.W + ox) * 64 + grp * 4;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const float4 bv = *reinterpret_cast<const float4 *>(g.bias + nt * 16 + grp * 4);
            const f16x4 ov = {(f16)fmaxf(acc[nt][f][0] + bv.x, 0.f), (f16)fmaxf(acc[nt][f][1] + bv.y, 0.f),
                              (f16)fmaxf(acc[nt][f][2] + bv.z, 0.f), (f16)fmaxf(acc[nt][f][3] + bv.w, 0.f)};
            *reinterpret_cast<f16x4 *>(o + nt * 16) = ov;
        }
    }
}

// ---- the tile convolution shared by the pooled convs and the heads ---------------------------------------------------------------------
// halo: [kHH * kHW pixels][CIN halfs + 8 of padding] (the 16 bytes keep the 16 pixels of a row off the same LDS banks)
template <int CIN>
__device__ __forceinline__ void stage_halo(unsigned char *halo, const f16 *in, int b, int H, int W, int ty0, int tx0, int tid) {
    constexpr int PS = CIN * 2 + 16, SEGS = CIN / 8;
    const f16x8 z8 = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
    for (int i = tid; i < kHH * kHW * SEGS; i += 256) {
        const int p = i / SEGS, sg = i - p * SEGS;
        const int hy = p / kHW, hx = p - hy * kHW;
        const int y = ty0 + hy - 1, x = tx0 + hx - 1;
        f16x8 v = z8;                                          // zero padding
        if (y >= 0 && y < H && x >= 0 && x < W)
            v = *reinterpret_cast<const f16x8 *>(in + (((long)b * H + y) * W + x) * CIN + sg * 8);
        *reinterpret_cast<f16x8 *>(halo + p * PS + sg * 16) = v;
    }
}

// acc[nt][f] += conv of this wave's two rows with the 128 output channels of `wstream` (9 * CIN / 32 k-steps of 8 fragments,
// followed by at least one chunk of padding).  Every wave of the workgroup calls it; it ends on a barrier.
template <int CIN>
__device__ __forceinline__ void tile_conv(const unsigned char *halo, f16x8 *ring, const f16 *wstream, int tid, f32x4 (&acc)[8][2]) {
    constexpr int PS = CIN * 2 + 16, CPT = CIN / 32, KS = 9 * CPT;
    const int lane = tid & 63, wave = tid >> 6, r16 = lane & 15, grp = lane >> 4;
    const f16x8 *gsrc = reinterpret_cast<const f16x8 *>(wstream);
    f16x8 p0 = gsrc[tid], p1 = gsrc[tid + 256];
    ring[tid] = p0; ring[tid + 256] = p1;
    p0 = gsrc[kChunk + tid]; p1 = gsrc[kChunk + tid + 256];
    __syncthreads();                                           // the halo and chunk 0 are in LDS
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        const int tap = ks / CPT, c0 = (ks - tap * CPT) * 32;
        const int dy = tap / 3, dx = tap - dy * 3;
        const f16x8 *cur = ring + (ks & 1) * kChunk;
        f16x8 xv[2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
            xv[f] = *reinterpret_cast<const f16x8 *>(halo + ((2 * wave + f + dy) * kHW + r16 + dx) * PS + (c0 + 8 * grp) * 2);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const f16x8 w = cur[nt * 64 + lane];
#pragma unroll
            for (int f = 0; f < 2; ++f) acc[nt][f] = MFMA_16x16x32(w, xv[f], acc[nt][f]);
        }
        // the other slot was last read in step ks - 1, and every wave has passed that step's barrier
        f16x8 *nxt = ring + ((ks + 1) & 1) * kChunk;
        nxt[tid] = p0; nxt[tid + 256] = p1;
        const int cn = min(ks + 2, KS);                        // chunk KS is the host's zero padding
        p0 = gsrc[cn * kChunk + tid]; p1 = gsrc[cn * kChunk + tid + 256];
        __syncthreads();
    }
}

struct PoolArgs {
    const f16 *in;             // [G][H][W][CIN]
    const f16 *w;              // [9 CIN / 32][8] fragments + padding
    const float *bias;         // [128]
    const f16 *res;            // [G][H][W][128] added before the ReLU, or NULL
    f16 *out;                  // [G][H / 2][W / 2][128]
    int H, W, tiles_x;
};

template <int CIN>
__global__ void __launch_bounds__(256) cliqa_conv_pool_kernel(const PoolArgs g) {
    __shared__ __attribute__((aligned(16))) f16x8 ring[2 * kChunk];
    __shared__ __attribute__((aligned(16))) unsigned char halo[kHH * kHW * (CIN * 2 + 16)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, grp = lane >> 4;
    const int ty0 = ((int)blockIdx.x / g.tiles_x) * kTH, tx0 = ((int)blockIdx.x % g.tiles_x) * kTW;
    const int b = blockIdx.y;
    stage_halo<CIN>(halo, g.in, b, g.H, g.W, ty0, tx0, tid);
    f32x4 acc[8][2];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[nt][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    tile_conv<CIN>(halo, ring, g.w, tid, acc);

    const int Hp = g.H >> 1, Wp = g.W >> 1;
    const int py = (ty0 >> 1) + wave, px = (tx0 >> 1) + (r16 >> 1);
    const int ox = tx0 + r16;
    const bool store = (r16 & 1) == 0 && py < Hp && px < Wp;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const int n0 = nt * 16 + grp * 4;
        const float4 bv = *reinterpret_cast<const float4 *>(g.bias + n0);
        float m[4];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int oy = ty0 + 2 * wave + f;
            float v[4] = {acc[nt][f][0] + bv.x, acc[nt][f][1] + bv.y, acc[nt][f][2] + bv.z, acc[nt][f][3] + bv.w};
            if (g.res && oy < g.H && ox < g.W) {
                const f16x4 rv = *reinterpret_cast<const f16x4 *>(g.res + (((long)b * g.H + oy) * g.W + ox) * 128 + n0);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += (float)rv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = f == 0 ? v[i] : fmaxf(m[i], v[i]);
        }
        // a pooled pixel inside [Hp, Wp) reads only conv outputs inside the map; the others are never stored
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] = fmaxf(fmaxf(m[i], __shfl_xor(m[i], 1)), 0.f);      // ReLU commutes with the max
        if (store) {
            const f16x4 ov = {(f16)m[0], (f16)m[1], (f16)m[2], (f16)m[3]};
            *reinterpret_cast<f16x4 *>(g.out + (((long)b * Hp + py) * Wp + px) * 128 + n0) = ov;
        }
    }
}

// ---- heads ---------------------------------------------------------------------------------------------------------------------------
struct HeadArgs {
    const f16 *in;             // [G][mh][mw][128]
    const f16 *w;              // [heads * 2 passes] streams of 128 output channels, `pass_halfs` apart
    const float *bias;         // [heads][256]
    float *part;               // [G][heads][tiles][256]: max (mean_mask bit clear) or sum (bit set) over the tile's pixels
    float *map;                // tests only: [G][mh][mw][heads * 256] fp32, or NULL
    long pass_halfs;
    int mh, mw, tiles_x, tiles, heads, mean_mask;
};

__global__ void __launch_bounds__(256) cliqa_head_kernel(const HeadArgs g) {
    __shared__ __attribute__((aligned(16))) f16x8 ring[2 * kChunk];
    __shared__ __attribute__((aligned(16))) unsigned char halo[kHH * kHW * (128 * 2 + 16)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, grp = lane >> 4;
    const int ty0 = ((int)blockIdx.x / g.tiles_x) * kTH, tx0 = ((int)blockIdx.x % g.tiles_x) * kTW;
    const int b = blockIdx.y;
    stage_halo<128>(halo, g.in, b, g.mh, g.mw, ty0, tx0, tid);
    float (*red)[128] = reinterpret_cast<float (*)[128]>(ring);     // free between a pass's last barrier and the next pass
    const int ox = tx0 + r16;
    for (int pass = 0; pass < g.heads * 2; ++pass) {
        const int head = pass >> 1;
        const bool mean = (g.mean_mask >> head) & 1;
        f32x4 acc[8][2];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
#pragma unroll
            for (int f = 0; f < 2; ++f) acc[nt][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
        tile_conv<128>(halo, ring, g.w + pass * g.pass_halfs, tid, acc);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int n0 = nt * 16 + grp * 4;
            const float4 bv = *reinterpret_cast<const float4 *>(g.bias + pass * 128 + n0);
            float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const int oy = ty0 + 2 * wave + f;
                const bool in = oy < g.mh && ox < g.mw;
                // a pixel outside the map counts 0: neutral for the sum, and for the max of values that are >= 0 after the ReLU
                const float v[4] = {in ? fmaxf(acc[nt][f][0] + bv.x, 0.f) : 0.f, in ? fmaxf(acc[nt][f][1] + bv.y, 0.f) : 0.f,
                                    in ? fmaxf(acc[nt][f][2] + bv.z, 0.f) : 0.f, in ? fmaxf(acc[nt][f][3] + bv.w, 0.f) : 0.f};
                if (g.map && in) {
                    float *o = g.map + (((long)b * g.mh + oy) * g.mw + ox) * (g.heads * 256) + pass * 128 + n0;
                    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) m[i] = mean ? m[i] + v[i] : fmaxf(m[i], v[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    const float o = __shfl_xor(m[i], d);
                    m[i] = mean ? m[i] + o : fmaxf(m[i], o);
                }
            }
            if (r16 == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) red[wave][n0 + i] = m[i];
            }
        }
        __syncthreads();
        if (tid < 128) {
            float v = red[0][tid];
#pragma unroll
            for (int k = 1; k < 4; ++k) v = mean ? v + red[k][tid] : fmaxf(v, red[k][tid]);
            g.part[(((long)b * g.heads + head) * g.tiles + blockIdx.x) * 256 + (pass & 1) * 128 + tid] = v;
        }
        __syncthreads();
    }
}

struct FinalArgs {
    const float *part;         // [G][heads][tiles][256]
    const float *ow, *ob;      // 1x1 conv: [heads][256], [heads]
    float *out[2];             // per head: [G]
    int tiles, heads, mean_mask, clamp12;
    float inv_hw;
};

__global__ void __launch_bounds__(256) cliqa_head_final_kernel(const FinalArgs g) {
    __shared__ float s[256];
    const int tid = threadIdx.x, b = blockIdx.x / g.heads, head = blockIdx.x - b * g.heads;
    const bool mean = (g.mean_mask >> head) & 1;
    const float *p = g.part + (long)blockIdx.x * g.tiles * 256 + tid;
    float v = p[0];
    for (int t = 1; t < g.tiles; ++t) v = mean ? v + p[(long)t * 256] : fmaxf(v, p[(long)t * 256]);
    if (mean) v *= g.inv_hw;
    s[tid] = v * g.ow[head * 256 + tid];
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) s[tid] += s[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        float y = s[0] + g.ob[head];
        if (g.clamp12) y = fminf(fmaxf(y, 1.f), 2.f);           // scale_factor.py:63
        g.out[head][b] = y;
    }
}

// ---- patch selection (cliqa/utils.py:26-27, :36-57) ------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double *s, int tid) {
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) s[tid] += s[tid + d];
        __syncthreads();
    }
    return s[0];
}

// one workgroup per patch: the unbiased std over the patch per channel, two passes in double, the mean of the three, rounded once
__global__ void __launch_bounds__(256) cliqa_patch_score_kernel(const float *__restrict__ img, int H, int W, int P, int cols,
                                                                float *__restrict__ scores) {
    __shared__ double s[256];
    const int tid = threadIdx.x;
    const int y0 = ((int)blockIdx.x / cols) * P, x0 = ((int)blockIdx.x % cols) * P;
    const int n = P * P;
    double score = 0.0;
    for (int c = 0; c < 3; ++c) {
        const float *p = img + ((long)c * H + y0) * W + x0;
        double a = 0.0;
        for (int i = tid; i < n; i += 256) a += (double)p[(long)(i / P) * W + i % P];
        const double mu = block_sum(a, s, tid) / (double)n;
        a = 0.0;
        for (int i = tid; i < n; i += 256) {
            const double d = (double)p[(long)(i / P) * W + i % P] - mu;
            a += d * d;
        }
        score += sqrt(block_sum(a, s, tid) / (double)(n - 1));
    }
    if (tid == 0) scores[blockIdx.x] = (float)(score / 3.0);
}

// workgroup (k, c): finds the patch of rank k (descending score, the lower index first among equals) and copies its channel c
__global__ void __launch_bounds__(256) cliqa_patch_gather_kernel(const float *__restrict__ img, int H, int W, int P, int cols, int n,
                                                                 const float *__restrict__ scores, long long *__restrict__ indices,
                                                                 float *__restrict__ patches) {
    __shared__ float sc[kMaxPatches];
    __shared__ int pick;
    const int tid = threadIdx.x, k = blockIdx.x, c = blockIdx.y;
    if (tid == 0) pick = 0;                                    // a NaN score leaves a rank unclaimed
    for (int i = tid; i < n; i += 256) sc[i] = scores[i];
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const float si = sc[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (sc[j] > si || (sc[j] == si && j < i)) ? 1 : 0;
        if (rank == k) pick = i;                               // ranks are a permutation: exactly one lane writes
    }
    __syncthreads();
    const int idx = pick;
    if (c == 0 && tid == 0) indices[k] = idx;
    const float *src = img + ((long)c * H + (idx / cols) * P) * W + (idx % cols) * P;
    float *dst = patches + ((long)k * 3 + c) * P * P;
    for (int i = tid; i < P * P; i += 256) dst[i] = src[(long)(i / P) * W + i % P];
}

}  // namespace
}  // namespace nunif

using namespace nunif;
using cliqa_host::Geometry;

struct nunif_cliqa {
    DeviceOwner dev;
    int kind = 0, cin = 3, heads = 1, mean_mask = 0;
    f16 *w_entry = nullptr, *w_conv2 = nullptr, *w_rb[4] = {nullptr, nullptr, nullptr, nullptr}, *w_head = nullptr;
    float *b_entry = nullptr, *b_conv2 = nullptr, *b_rb[4] = {nullptr, nullptr, nullptr, nullptr}, *b_head = nullptr;
    float *ow = nullptr, *ob = nullptr;
    long pass_halfs = 0;
};

namespace {

int check_shape(const HostTensor *t, std::initializer_list<int64_t> shape, const char *name) {
    if (t->shape != std::vector<int64_t>(shape)) {
        set_error("cliqa_create: tensor %s has the wrong shape", name);
        return NUNIF_HIP_EINVAL;
    }
    return NUNIF_HIP_OK;
}

int build(nunif_cliqa *net, const TensorMap &tm) {
    const HostTensor *w, *b;
    int rc;
    if ((rc = find(tm, "conv1.w", &w)) || (rc = find(tm, "conv1.b", &b))) return rc;
    const int cin = net->cin;
    if ((rc = check_shape(w, {64, cin, 3, 3}, "conv1.w")) || (rc = check_shape(b, {64}, "conv1.b"))) return rc;
    if ((rc = net->dev.upload(cliqa_host::entry_stream(w->data, cin), &net->w_entry)) || (rc = net->dev.upload_f32(b, &net->b_entry)))
        return rc;
    if ((rc = find(tm, "conv2.w", &w)) || (rc = find(tm, "conv2.b", &b))) return rc;
    if ((rc = check_shape(w, {128, 64, 3, 3}, "conv2.w")) || (rc = check_shape(b, {128}, "conv2.b"))) return rc;
    if ((rc = net->dev.upload(cliqa_host::conv_stream(w->data, 64, 0), &net->w_conv2)) || (rc = net->dev.upload_f32(b, &net->b_conv2))) return rc;
    const char *rb[4] = {"rb1a", "rb1b", "rb2a", "rb2b"};
    for (int i = 0; i < 4; ++i) {
        const std::string n = rb[i];
        if ((rc = find(tm, n + ".w", &w)) || (rc = find(tm, n + ".b", &b))) return rc;
        if ((rc = check_shape(w, {128, 128, 3, 3}, rb[i])) || (rc = check_shape(b, {128}, rb[i]))) return rc;
        if ((rc = net->dev.upload(cliqa_host::conv_stream(w->data, 128, 0), &net->w_rb[i])) || (rc = net->dev.upload_f32(b, &net->b_rb[i]))) return rc;
    }
    std::vector<f16> hw;
    std::vector<float> hb, ow, ob;
    for (int h = 0; h < net->heads; ++h) {
        const std::string n = "head" + std::to_string(h);
        const HostTensor *o, *c;
        if ((rc = find(tm, n + ".w", &w)) || (rc = find(tm, n + ".b", &b)) || (rc = find(tm, n + ".ow", &o)) ||
            (rc = find(tm, n + ".ob", &c)))
            return rc;
        if ((rc = check_shape(w, {256, 128, 3, 3}, "head.w")) || (rc = check_shape(b, {256}, "head.b")) ||
            (rc = check_shape(o, {256}, "head.ow")) || (rc = check_shape(c, {1}, "head.ob")))
            return rc;
        for (int half = 0; half < 2; ++half) {
            const std::vector<f16> s = cliqa_host::conv_stream(w->data, 128, half * 128);
            net->pass_halfs = (long)s.size();
            hw.insert(hw.end(), s.begin(), s.end());
        }
        hb.insert(hb.end(), b->data, b->data + 256);
        ow.insert(ow.end(), o->data, o->data + 256);
        ob.push_back(c->data[0]);
    }
    if ((rc = net->dev.upload(hw, &net->w_head)) || (rc = net->dev.upload(hb, &net->b_head)) || (rc = net->dev.upload(ow, &net->ow)) ||
        (rc = net->dev.upload(ob, &net->ob)))
        return rc;
    return NUNIF_HIP_OK;
}

template <int CIN>
int launch_pool(const f16 *in, const f16 *w, const float *bias, const f16 *res, f16 *out, int G, int H, int W, hipStream_t s) {
    PoolArgs a;
    a.in = in; a.w = w; a.bias = bias; a.res = res; a.out = out; a.H = H; a.W = W; a.tiles_x = cdiv(W, kTW);
    cliqa_conv_pool_kernel<CIN><<<dim3(a.tiles_x * cdiv(H, kTH), G), 256, 0, s>>>(a);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

int launch_plain(const f16 *in, const f16 *w, const float *bias, f16 *out, int G, int H, int W, hipStream_t s) {
    ConvArgs c = {};
    c.a = in; c.B = G; c.Hi = H; c.Wi = W; c.Ho = H; c.Wo = W; c.Cin = 128; c.stride = 1; c.kh = 3; c.kw = 3;
    c.wstream = w; c.bias = bias; c.N = 128; c.n_real = 128; c.act = 3; c.out = out; c.zpad = 1;
    return launch_conv(c, s);
}

struct TapOut { f16 *t1, *t2, *t3; float *maps; };

int forward(nunif_cliqa *net, const float *x, int B, int H, int W, int group, void *workspace, int64_t workspace_bytes, float *out0,
            float *out1, const TapOut *taps, hipStream_t s) {
    NUNIF_REQUIRE(net && x && workspace && out0 && (net->heads == 1 || out1), "cliqa_forward: NULL argument");
    NUNIF_REQUIRE(cliqa_host::shape_ok(B, H, W), "cliqa_forward: bad shape B=%d H=%d W=%d (H, W >= 8)", B, H, W);
    const int G = cliqa_host::group_size(B, H, W, group);
    const Geometry q = cliqa_host::geometry(net->heads, G, H, W);
    NUNIF_REQUIRE(workspace_bytes >= q.total, "cliqa_forward: workspace of %lld bytes, %lld needed (nunif_hip_cliqa_workspace_bytes)",
                  (long long)workspace_bytes, (long long)q.total);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    f16 *a0 = (f16 *)(ws + q.a0), *a1 = (f16 *)(ws + q.a1), *t1 = (f16 *)(ws + q.t1), *a2 = (f16 *)(ws + q.a2);
    f16 *t2 = (f16 *)(ws + q.t2), *a3 = (f16 *)(ws + q.a3);
    float *part = (float *)(ws + q.part);
    int rc;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int n = std::min(G, B - b0);
        EntryArgs e;
        e.x = x + (long)b0 * 3 * H * W; e.w = net->w_entry; e.bias = net->b_entry; e.out = a0; e.H = H; e.W = W;
        e.tiles_x = cdiv(W, kTW); e.jpeg = net->kind == KIND_JPEG;
        cliqa_entry_kernel<<<dim3(e.tiles_x * cdiv(H, kTH), n), 256, 0, s>>>(e);
        NUNIF_LAUNCH_CHECK();
        if ((rc = launch_pool<64>(a0, net->w_conv2, net->b_conv2, nullptr, a1, n, H, W, s))) return rc;
        if ((rc = launch_plain(a1, net->w_rb[0], net->b_rb[0], t1, n, q.H1, q.W1, s))) return rc;
        if ((rc = launch_pool<128>(t1, net->w_rb[1], net->b_rb[1], a1, a2, n, q.H1, q.W1, s))) return rc;
        if ((rc = launch_plain(a2, net->w_rb[2], net->b_rb[2], t2, n, q.H2, q.W2, s))) return rc;
        if ((rc = launch_pool<128>(t2, net->w_rb[3], net->b_rb[3], a2, a3, n, q.H2, q.W2, s))) return rc;
        HeadArgs h;
        h.in = a3; h.w = net->w_head; h.bias = net->b_head; h.part = part; h.pass_halfs = net->pass_halfs;
        h.map = taps ? taps->maps + (long)b0 * q.H3 * q.W3 * net->heads * 256 : nullptr;
        h.mh = q.H3; h.mw = q.W3; h.tiles_x = cdiv(q.W3, kTW); h.tiles = q.tiles3; h.heads = net->heads; h.mean_mask = net->mean_mask;
        cliqa_head_kernel<<<dim3(q.tiles3, n), 256, 0, s>>>(h);
        NUNIF_LAUNCH_CHECK();
        FinalArgs f;
        f.part = part; f.ow = net->ow; f.ob = net->ob; f.out[0] = out0 + b0; f.out[1] = out1 ? out1 + b0 : nullptr;
        f.tiles = q.tiles3; f.heads = net->heads; f.mean_mask = net->mean_mask; f.clamp12 = net->kind == KIND_SCALE;
        f.inv_hw = 1.f / (float)(q.H3 * q.W3);
        cliqa_head_final_kernel<<<n * net->heads, 256, 0, s>>>(f);
        NUNIF_LAUNCH_CHECK();
        if (taps) {
            const size_t n1 = (size_t)q.H1 * q.W1 * 128, n2 = (size_t)q.H2 * q.W2 * 128, n3 = (size_t)q.H3 * q.W3 * 128;
            NUNIF_HIP_CHECK(hipMemcpyAsync(taps->t1 + b0 * n1, a1, n * n1 * 2, hipMemcpyDeviceToDevice, s));
            NUNIF_HIP_CHECK(hipMemcpyAsync(taps->t2 + b0 * n2, a2, n * n2 * 2, hipMemcpyDeviceToDevice, s));
            NUNIF_HIP_CHECK(hipMemcpyAsync(taps->t3 + b0 * n3, a3, n * n3 * 2, hipMemcpyDeviceToDevice, s));
        }
    }
    return NUNIF_HIP_OK;
}

}  // namespace

extern "C" int nunif_hip_cliqa_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t kind, nunif_cliqa **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "cliqa_create: NULL argument");
    NUNIF_REQUIRE(kind >= KIND_JPEG && kind <= KIND_SCALE, "cliqa_create: kind %d (0 jpeg_quality, 1 grain_noise_level, 2 scale_factor)",
                  kind);
    for (int i = 0; i < n_tensors; ++i) NUNIF_REQUIRE(tensors[i].data, "cliqa_create: tensor %s has no data", tensors[i].name);
    nunif_cliqa *net = new nunif_cliqa();
    net->kind = kind;
    net->cin = kind == KIND_JPEG ? 6 : 3;
    net->heads = kind == KIND_JPEG ? 2 : 1;
    net->mean_mask = kind == KIND_JPEG ? 2 : 0;                 // the subsampling head (head 1) pools by the mean
    const int rc = build(net, tensor_map(tensors, n_tensors));
    if (rc != NUNIF_HIP_OK) {
        net->dev.free_all();
        delete net;
        return rc;
    }
    *handle = net;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_cliqa_destroy(nunif_cliqa *handle) {
    if (!handle) return;
    handle->dev.free_all();
    delete handle;
}

extern "C" int64_t nunif_hip_cliqa_workspace_bytes(nunif_cliqa *handle, int32_t B, int32_t H, int32_t W, int32_t group) {
    if (!handle) return 0;
    return cliqa_host::workspace_bytes(handle->heads, B, H, W, group);
}

extern "C" int nunif_hip_cliqa_forward(nunif_cliqa *handle, const float *x, int32_t B, int32_t H, int32_t W, int32_t group,
                                       void *workspace, int64_t workspace_bytes, float *out0, float *out1, void *stream) {
    return forward(handle, x, B, H, W, group, workspace, workspace_bytes, out0, out1, nullptr, (hipStream_t)stream);
}

extern "C" int nunif_hip_cliqa_debug_taps(nunif_cliqa *handle, const float *x, int32_t B, int32_t H, int32_t W, int32_t group,
                                          void *workspace, int64_t workspace_bytes, float *out0, float *out1, void *tap1, void *tap2,
                                          void *tap3, float *head_maps, void *stream) {
    NUNIF_REQUIRE(tap1 && tap2 && tap3 && head_maps, "cliqa_debug_taps: NULL argument");
    const TapOut t{(f16 *)tap1, (f16 *)tap2, (f16 *)tap3, head_maps};
    return forward(handle, x, B, H, W, group, workspace, workspace_bytes, out0, out1, &t, (hipStream_t)stream);
}

extern "C" int nunif_hip_cliqa_select_patches(const float *image, int32_t H, int32_t W, int32_t patch_size, int32_t num_patches,
                                              float *scores, int64_t *indices, float *patches, void *stream) {
    NUNIF_REQUIRE(image && scores && indices && patches, "cliqa_select_patches: NULL argument");
    NUNIF_REQUIRE(patch_size >= 2 && patch_size <= 4096 && H >= patch_size && W >= patch_size && H <= 65536 && W <= 65536,
                  "cliqa_select_patches: image %dx%d is smaller than a patch of %d (pad on the host: safe_pad)", H, W, patch_size);
    const int rows = H / patch_size, cols = W / patch_size, n = rows * cols;
    NUNIF_REQUIRE(n <= kMaxPatches, "cliqa_select_patches: %d patches (at most %d)", n, kMaxPatches);
    NUNIF_REQUIRE(num_patches >= 1, "cliqa_select_patches: num_patches %d", num_patches);
    const int K = std::min(num_patches, n);
    hipStream_t s = (hipStream_t)stream;
    cliqa_patch_score_kernel<<<n, 256, 0, s>>>(image, H, W, patch_size, cols, scores);
    NUNIF_LAUNCH_CHECK();
    cliqa_patch_gather_kernel<<<dim3(K, 3), 256, 0, s>>>(image, H, W, patch_size, cols, n, scores, (long long *)indices, patches);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
