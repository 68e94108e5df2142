// iw3 --autocrop (nunif/utils/autocrop.py, reference) for gfx950: the letterbox detector's per-row and per-column statistics with
// their decisions (AutoCropDetector.detect_tb / detect_lr :140-170 and the accumulation of update :24-48), and the crop / uncrop
// copy (AutoCrop.crop :346-354, uncrop :356-360).  fp32 operands, no matrix instructions: every kernel is bound by memory or LDS.
//
//   autocrop_rows_kernel<FLAT>        one wave per image row (4 rows per workgroup), the frames of the batch one after another.
//                                     Black: sum, min and max of the clamped Y in one pass.  Flat: the row's Y staged in LDS, its
//                                     lower median by radix select, then the count of |y - median| < 16/255.
//   autocrop_cols_partial_kernel<V>   black, stage 1: sum / min / max of V adjacent columns over a band of kBand rows
//   autocrop_cols_final_kernel        black, stage 2: the bands of a column added in band order, the decision
//   autocrop_cols_flat_kernel<V>      flat: a tile of 8 columns x H rows of Y in LDS (one line per column), one wave per column
//   autocrop_crop_pad_kernel<VST>     dst = src shifted inside a window, pad_value outside it
//
// Y = r*0.299 + g*0.587 + b*0.114 is evaluated as torch evaluates it (three rounded products, two rounded sums: this file is
// built without FMA contraction), so the medians are the reference's bit for bit.  The sums run in double: the kernels wait for
// memory, and an fp32 chain over 2 160 rows would carry an error of its own into a statistic that is compared with a threshold.
// No float atomics and no atomics on global memory at all: one thread owns a row's or a column's counter, sums have a fixed order,
// the radix select counts integers.  Results are bit-identical from call to call and across streams.
//
// Limits of the tiling (refused on the host): W <= 8192 (4 row lines of W floats in LDS), H <= 4608 (8 column lines of H floats).
#include <algorithm>

#include "common.h"

namespace nunif {
namespace {

constexpr int kMaxW = 8192;
constexpr int kMaxH = 4608;
constexpr int kRowWaves = 4;         // rows per workgroup of the row pass
constexpr int kColLines = 8;         // columns per workgroup of the flat column pass
constexpr int kBand = 32;            // rows per band of the black column pass

// a Python scalar meets an fp32 tensor as fp32 (autocrop.py:133-136, :145-146, :152-153)
__device__ __forceinline__ float c_lo() { return (float)(16.0 / 255.0); }
__device__ __forceinline__ float c_hi() { return (float)(235.0 / 255.0); }
__device__ __forceinline__ float c_dark() { return (float)(32.0 / 255.0); }
__device__ __forceinline__ float c_dev() { return (float)(16.0 / 255.0); }
__device__ __forceinline__ float c_frac() { return (float)0.99; }

template <bool TV>
__device__ __forceinline__ float luma(float r, float g, float b) {           // rgb_to_y :118-138
    float y = r * 0.299f + g * 0.587f + b * 0.114f;
    if (TV) y = fminf(fmaxf(y, c_lo()), c_hi());
    return y;
}

struct Acc {                         // sum / min / max of one line
    double s;
    float lo, hi;
};
__device__ __forceinline__ void acc_init(Acc &a) { a.s = 0.0; a.lo = INFINITY; a.hi = -INFINITY; }
__device__ __forceinline__ void acc_add(Acc &a, float y) { a.s += (double)y; a.lo = fminf(a.lo, y); a.hi = fmaxf(a.hi, y); }

// mean, max |y - mean| and the decision of the black modes (:144-148).  x -> fl(x - mean) is monotonic, so the largest
// |y - mean| of a line is the larger of fl(max - mean) and fl(mean - min).
__device__ __forceinline__ int black_decide(double sum, float lo, float hi, int n, float &mean, float &dev) {
    mean = (float)(sum / (double)n);
    dev = fmaxf(hi - mean, mean - lo);
    return (mean <= c_dark() && dev < c_dev()) ? 1 : 0;
}

// ---- lower median of a line in LDS by one wave -----------------------------------------------------------------------------------
// Radix select over the ordered bit pattern, four passes of 8 bits, the scheme of sod_depth_position_kernel (sod_v1.hip) with one
// wave and one 256-bin histogram per line.  Every wave of the workgroup calls this with the same n: the barriers are uniform.

// the bin that holds rank k of `hist`: each lane owns four bins, an inclusive scan over the lanes finds the owner
__device__ __forceinline__ void wave_pick(const unsigned *hist, int lane, int shift, unsigned &k, unsigned &prefix) {
    const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
    const unsigned own = c0 + c1 + c2 + c3;
    unsigned inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, d);
        if (lane >= d) inc += t;
    }
    const unsigned exc = inc - own;
    const unsigned long long owner = __ballot(exc <= k && k < inc);
    const int leader = owner ? __ffsll((long long)owner) - 1 : 63;
    unsigned bin = 4u * lane, kk = k - exc;
    if (kk >= c0) {
        kk -= c0; ++bin;
        if (kk >= c1) {
            kk -= c1; ++bin;
            if (kk >= c2) { kk -= c2; ++bin; }
        }
    }
    bin = (unsigned)__shfl((int)bin, leader);
    kk = (unsigned)__shfl((int)kk, leader);
    prefix |= bin << shift;
    k = kk;
}

__device__ float wave_lower_median(const float *line, int n, unsigned *hist, int lane) {
    unsigned k = (unsigned)((n - 1) / 2), prefix = 0;       // torch.median: the lower of the two middle values
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = lane; i < 256; i += 64) hist[i] = 0;
        __syncthreads();
        for (int i = lane; i < ((n + 63) / 64) * 64; i += 64) {          // whole waves: every lane takes part in the ballots
            const bool in = i < n;
            const unsigned key = in ? order_key(line[i]) : 0u;
            const bool hit = in && (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8)));
            const unsigned bin = (key >> shift) & 255u;
            // a bar puts a whole wave into one bin: when all hits agree on the bin, one lane adds their number instead of up to
            // 64 atomics on one LDS word
            const unsigned long long hits = __ballot(hit);
            if (hits == 0ull) continue;
            const int leader = __ffsll((long long)hits) - 1;
            const unsigned lbin = (unsigned)__shfl((int)bin, leader);
            const unsigned long long same = __ballot(hit && bin == lbin);
            if (same == hits) {
                if (lane == leader) atomicAdd(&hist[lbin], (unsigned)__popcll(hits));
            } else if (hit) {
                atomicAdd(&hist[bin], 1u);
            }
        }
        __syncthreads();
        wave_pick(hist, lane, shift, k, prefix);
        __syncthreads();
    }
    return key_value(prefix);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// median, the fraction of the line within 16/255 of it, and the decision of the flat modes (:150-154)
__device__ int flat_decide(const float *line, int n, unsigned *hist, int lane, float &median, float &frac) {
    median = wave_lower_median(line, n, hist, lane);
    int cnt = 0;
    for (int i = lane; i < n; i += 64) cnt += fabsf(line[i] - median) < c_dev() ? 1 : 0;
    cnt = wave_sum_int(cnt);
    frac = (float)cnt / (float)n;
    return frac > c_frac() ? 1 : 0;
}

struct StatsArgs {
    const float *x;                  // [B][3][H][W]
    int B, H, W, vec4;               // vec4: W % 4 == 0 and x is 16-byte aligned
    int *count;                      // [H] (rows) or [W] (columns), or NULL
    float *stat_a, *stat_b;          // [B][H] or [B][W]: mean | median, maxdev | fraction; or NULL
};

// ---- rows (detect_tb) -----------------------------------------------------------------------------------------------------------------
template <bool FLAT>
__global__ void __launch_bounds__(kRowWaves * 64) autocrop_rows_kernel(const StatsArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wp = (g.W + 3) & ~3;
    unsigned *hist = reinterpret_cast<unsigned *>(smem) + wave * 256;
    float *line = smem + kRowWaves * 256 + (long)wave * wp;
    const int row_raw = blockIdx.x * kRowWaves + wave;
    const bool active = row_raw < g.H;
    const int row = active ? row_raw : g.H - 1;              // a wave past the last row repeats it and writes nothing
    const long hw = (long)g.H * g.W;
    int total = 0;
    for (int b = 0; b < g.B; ++b) {
        const float *r = g.x + (long)b * 3 * hw + (long)row * g.W, *gr = r + hw, *bl = gr + hw;
        Acc a;
        acc_init(a);
        if (g.vec4) {
            for (int i = lane * 4; i < g.W; i += 256) {
                const f32x4 vr = *reinterpret_cast<const f32x4 *>(r + i), vg = *reinterpret_cast<const f32x4 *>(gr + i),
                            vb = *reinterpret_cast<const f32x4 *>(bl + i);
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = luma<!FLAT>(vr[j], vg[j], vb[j]);
                if (FLAT) {
                    *reinterpret_cast<f32x4 *>(line + i) = y;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc_add(a, y[j]);
                }
            }
        } else {
            for (int i = lane; i < g.W; i += 64) {
                const float y = luma<!FLAT>(r[i], gr[i], bl[i]);
                if (FLAT) line[i] = y;
                else acc_add(a, y);
            }
        }
        float sa, sb;
        int dec;
        if (FLAT) {
            __syncthreads();
            dec = flat_decide(line, g.W, hist, lane, sa, sb);
            __syncthreads();                                  // the line is rewritten for the next frame
        } else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {               // a fixed butterfly: the same sum in every lane, every call
                a.s += __shfl_xor(a.s, d);
                a.lo = fminf(a.lo, __shfl_xor(a.lo, d));
                a.hi = fmaxf(a.hi, __shfl_xor(a.hi, d));
            }
            dec = black_decide(a.s, a.lo, a.hi, g.W, sa, sb);
        }
        total += dec;
        if (active && lane == 0 && g.stat_a) {
            g.stat_a[(long)b * g.H + row] = sa;
            g.stat_b[(long)b * g.H + row] = sb;
        }
    }
    if (active && lane == 0 && g.count) g.count[row] += total;          // the row's only writer (update :38)
}

// ---- columns, black (detect_lr :159-164) ---------------------------------------------------------------------------------------------
struct ColPartial {
    double s;
    float lo, hi;
};

template <int V>
__global__ void __launch_bounds__(256) autocrop_cols_partial_kernel(const StatsArgs g, ColPartial *__restrict__ part, int bands) {
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (x0 >= g.W) return;
    const int band = blockIdx.y, b = blockIdx.z;
    const int y0 = band * kBand, y1 = min(y0 + kBand, g.H);
    const long hw = (long)g.H * g.W;
    const float *r = g.x + (long)b * 3 * hw + x0, *gr = r + hw, *bl = gr + hw;
    Acc a[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc_init(a[j]);
    for (int y = y0; y < y1; ++y) {
        const long o = (long)y * g.W;
        if (V == 4) {
            const f32x4 vr = *reinterpret_cast<const f32x4 *>(r + o), vg = *reinterpret_cast<const f32x4 *>(gr + o),
                        vb = *reinterpret_cast<const f32x4 *>(bl + o);
#pragma unroll
            for (int j = 0; j < V; ++j) acc_add(a[j], luma<true>(vr[j], vg[j], vb[j]));
        } else {
            acc_add(a[0], luma<true>(r[o], gr[o], bl[o]));
        }
    }
    ColPartial *p = part + ((long)b * bands + band) * g.W + x0;
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = ColPartial{a[j].s, a[j].lo, a[j].hi};
}

__global__ void __launch_bounds__(256) autocrop_cols_final_kernel(const StatsArgs g, const ColPartial *__restrict__ part, int bands) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= g.W) return;
    int total = 0;
    for (int b = 0; b < g.B; ++b) {
        double s = 0.0;
        float lo = INFINITY, hi = -INFINITY;
        for (int k = 0; k < bands; ++k) {                     // band order: the sum does not depend on the launch
            const ColPartial p = part[((long)b * bands + k) * g.W + x];
            s += p.s;
            lo = fminf(lo, p.lo);
            hi = fmaxf(hi, p.hi);
        }
        float mean, dev;
        total += black_decide(s, lo, hi, g.H, mean, dev);
        if (g.stat_a) {
            g.stat_a[(long)b * g.W + x] = mean;
            g.stat_b[(long)b * g.W + x] = dev;
        }
    }
    if (g.count) g.count[x] += total;                          // the column's only writer (update :46)
}

// ---- columns, flat (detect_lr :165-170) ----------------------------------------------------------------------------------------------
// line stride: H rounded up to 8, plus 4.  The staging writes of a 32-lane group (16 rows x 2 column quads) then fall on 32
// different banks.
__host__ __device__ inline int col_line_stride(int H) { return ((H + 7) & ~7) + 4; }

template <int V>
__global__ void __launch_bounds__(kColLines * 64) autocrop_cols_flat_kernel(const StatsArgs g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hp = col_line_stride(g.H);
    unsigned *hist = reinterpret_cast<unsigned *>(smem) + wave * 256;
    float *tile = smem + kColLines * 256;
    const float *line = tile + (long)wave * hp;
    const int x0 = blockIdx.x * kColLines;
    const int col = x0 + wave;
    const bool active = col < g.W;
    const long hw = (long)g.H * g.W;
    int total = 0;
    for (int b = 0; b < g.B; ++b) {
        const float *r = g.x + (long)b * 3 * hw, *gr = r + hw, *bl = gr + hw;
        if (V == 4) {                                         // W % 4 == 0: a quad of columns is inside the frame or outside it
            const int q = tid & 1, xq = x0 + 4 * q;
            for (int y = tid >> 1; y < g.H; y += kColLines * 32) {
                f32x4 yv = {0.f, 0.f, 0.f, 0.f};
                if (xq < g.W) {
                    const long o = (long)y * g.W + xq;
                    const f32x4 vr = *reinterpret_cast<const f32x4 *>(r + o), vg = *reinterpret_cast<const f32x4 *>(gr + o),
                                vb = *reinterpret_cast<const f32x4 *>(bl + o);
#pragma unroll
                    for (int j = 0; j < 4; ++j) yv[j] = luma<false>(vr[j], vg[j], vb[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) tile[(long)(4 * q + j) * hp + y] = yv[j];
            }
        } else {
            const int c = tid & 7, xc = x0 + c;
            for (int y = tid >> 3; y < g.H; y += kColLines * 8) {
                float yv = 0.f;
                if (xc < g.W) {
                    const long o = (long)y * g.W + xc;
                    yv = luma<false>(r[o], gr[o], bl[o]);
                }
                tile[(long)c * hp + y] = yv;
            }
        }
        __syncthreads();
        float median, frac;
        const int dec = flat_decide(line, g.H, hist, lane, median, frac);      // a wave past the last column selects over zeros
        __syncthreads();                                      // the tile is rewritten for the next frame
        total += dec;
        if (active && lane == 0 && g.stat_a) {
            g.stat_a[(long)b * g.W + col] = median;
            g.stat_b[(long)b * g.W + col] = frac;
        }
    }
    if (active && lane == 0 && g.count) g.count[col] += total;
}

// ---- crop / uncrop ---------------------------------------------------------------------------------------------------------------------
struct CropArgs {
    const float *src;                // [N][sH][sW]
    float *dst;                      // [N][dH][dW]
    long quads;                      // N * dH * ceil(dW / 4)
    int sH, sW, dH, dW;
    int y0, x0;                      // the window's first row / column in src
    int pt, pl;                      // ... and in dst
    int wh, ww;                      // its size
    int src_vec;                     // src is 16-byte aligned and sW % 4 == 0
    float pad;
};

// One lane = four adjacent columns of dst.  VST: dW % 4 == 0 and dst is 16-byte aligned, the store is one 16-byte store.  The
// load is one 16-byte load where the four columns lie inside the window and their source address is 16-byte aligned.
template <bool VST>
__global__ void __launch_bounds__(256) autocrop_crop_pad_kernel(const CropArgs g) {
    const int qw = (g.dW + 3) >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < g.quads; i += (long)gridDim.x * 256) {
        const int xq = (int)(i % qw) * 4;
        const long ny = i / qw;
        const int y = (int)(ny % g.dH);
        const long n = ny / g.dH;
        const int wy = y - g.pt, wx = xq - g.pl;
        const bool row_in = wy >= 0 && wy < g.wh;
        const float *s = g.src + (n * g.sH + (row_in ? wy + g.y0 : 0)) * (long)g.sW + g.x0;      // + wx: the column in the window
        f32x4 v = {g.pad, g.pad, g.pad, g.pad};
        if (row_in) {
            if (wx >= 0 && wx + 3 < g.ww && g.src_vec && ((g.x0 + wx) & 3) == 0) {
                v = *reinterpret_cast<const f32x4 *>(s + wx);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (wx + j >= 0 && wx + j < g.ww) v[j] = s[wx + j];
            }
        }
        float *d = g.dst + (n * g.dH + y) * (long)g.dW + xq;
        if (VST) {
            *reinterpret_cast<f32x4 *>(d) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (xq + j < g.dW) d[j] = v[j];
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int launch_stats(const float *x, int B, int H, int W, int flat, int passes, int *count_tb, int *count_lr, void *work,
                 long work_bytes, float *row_a, float *row_b, float *col_a, float *col_b, hipStream_t s) {
    NUNIF_REQUIRE(x, "autocrop_stats: NULL frame");
    NUNIF_REQUIRE(B > 0 && B <= 4096 && H > 0 && W > 0, "autocrop_stats: bad shape B=%d H=%d W=%d", B, H, W);
    NUNIF_REQUIRE(H <= kMaxH && W <= kMaxW, "autocrop_stats: a %dx%d frame exceeds the built tiling (H <= %d, W <= %d)", H, W, kMaxH,
                  kMaxW);
    NUNIF_REQUIRE(passes >= 1 && passes <= 3, "autocrop_stats: passes must be 1 (tb), 2 (lr) or 3 (both)");
    NUNIF_REQUIRE((row_a == nullptr) == (row_b == nullptr) && (col_a == nullptr) == (col_b == nullptr),
                  "autocrop_stats: statistic outputs come in pairs");
    const int vec4 = (W % 4 == 0 && aligned16(x)) ? 1 : 0;
    if (passes & 1) {
        NUNIF_REQUIRE(count_tb || row_a, "autocrop_stats: the tb pass has no output");
        const StatsArgs g{x, B, H, W, vec4, count_tb, row_a, row_b};
        const int grid = cdiv(H, kRowWaves);
        if (flat) {
            NUNIF_HIP_CHECK(hipFuncSetAttribute((const void *)autocrop_rows_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                kRowWaves * (256 + kMaxW) * 4));
            const size_t smem = (size_t)kRowWaves * (256 + ((W + 3) & ~3)) * 4;
            autocrop_rows_kernel<true><<<grid, kRowWaves * 64, smem, s>>>(g);
        } else {
            autocrop_rows_kernel<false><<<grid, kRowWaves * 64, 0, s>>>(g);
        }
        NUNIF_LAUNCH_CHECK();
    }
    if (passes & 2) {
        NUNIF_REQUIRE(count_lr || col_a, "autocrop_stats: the lr pass has no output");
        const StatsArgs g{x, B, H, W, vec4, count_lr, col_a, col_b};
        if (flat) {
            const int max_smem = kColLines * (256 + col_line_stride(kMaxH)) * 4;
            NUNIF_HIP_CHECK(hipFuncSetAttribute((const void *)autocrop_cols_flat_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                max_smem));
            NUNIF_HIP_CHECK(hipFuncSetAttribute((const void *)autocrop_cols_flat_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                max_smem));
            const size_t smem = (size_t)kColLines * (256 + col_line_stride(H)) * 4;
            const int grid = cdiv(W, kColLines);
            if (vec4) autocrop_cols_flat_kernel<4><<<grid, kColLines * 64, smem, s>>>(g);
            else autocrop_cols_flat_kernel<1><<<grid, kColLines * 64, smem, s>>>(g);
            NUNIF_LAUNCH_CHECK();
        } else {
            const int bands = cdiv(H, kBand);
            const long need = (long)B * bands * W * (long)sizeof(ColPartial);
            NUNIF_REQUIRE(work && work_bytes >= need && aligned16(work),
                          "autocrop_stats: the black lr pass needs %ld bytes of 16-byte aligned workspace", need);
            ColPartial *part = static_cast<ColPartial *>(work);
            if (vec4) autocrop_cols_partial_kernel<4><<<dim3(cdiv(W / 4, 256), bands, B), 256, 0, s>>>(g, part, bands);
            else autocrop_cols_partial_kernel<1><<<dim3(cdiv(W, 256), bands, B), 256, 0, s>>>(g, part, bands);
            NUNIF_LAUNCH_CHECK();
            autocrop_cols_final_kernel<<<cdiv(W, 256), 256, 0, s>>>(g, part, bands);
            NUNIF_LAUNCH_CHECK();
        }
    }
    return NUNIF_HIP_OK;
}

}  // namespace
}  // namespace nunif

using namespace nunif;

extern "C" int nunif_hip_autocrop_stats(const float *x, int32_t B, int32_t H, int32_t W, int32_t flat, int32_t passes,
                                        int32_t *border_count_tb, int32_t *border_count_lr, void *work, int64_t work_bytes,
                                        void *stream) {
    NUNIF_REQUIRE(!(passes & 1) || border_count_tb, "autocrop_stats: border_count_tb is NULL");
    NUNIF_REQUIRE(!(passes & 2) || border_count_lr, "autocrop_stats: border_count_lr is NULL");
    return launch_stats(x, B, H, W, flat, passes, border_count_tb, border_count_lr, work, (long)work_bytes, nullptr, nullptr,
                        nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int nunif_hip_autocrop_debug_stats(const float *x, int32_t B, int32_t H, int32_t W, int32_t flat, int32_t passes,
                                              int32_t *border_count_tb, int32_t *border_count_lr, void *work, int64_t work_bytes,
                                              float *row_a, float *row_b, float *col_a, float *col_b, void *stream) {
    NUNIF_REQUIRE(!(passes & 1) || (row_a && row_b), "autocrop_debug_stats: the row statistics are NULL");
    NUNIF_REQUIRE(!(passes & 2) || (col_a && col_b), "autocrop_debug_stats: the column statistics are NULL");
    return launch_stats(x, B, H, W, flat, passes, border_count_tb, border_count_lr, work, (long)work_bytes, row_a, row_b, col_a,
                        col_b, (hipStream_t)stream);
}

extern "C" int nunif_hip_autocrop_crop_pad(const float *src, float *dst, int64_t N, int32_t sH, int32_t sW, int32_t dH, int32_t dW,
                                           int32_t y0, int32_t x0, int32_t pad_top, int32_t pad_left, int32_t win_h, int32_t win_w,
                                           float pad_value, void *stream) {
    NUNIF_REQUIRE(src && dst && src != dst, "autocrop_crop_pad: NULL or aliased argument");
    NUNIF_REQUIRE(N > 0 && sH > 0 && sW > 0 && dH > 0 && dW > 0 && win_h > 0 && win_w > 0, "autocrop_crop_pad: empty shape");
    NUNIF_REQUIRE(sH <= (1 << 20) && sW <= (1 << 20) && dH <= (1 << 20) && dW <= (1 << 20) && N <= (1 << 20) &&
                      N * (int64_t)sH * sW < (1LL << 40) && N * (int64_t)dH * dW < (1LL << 40),
                  "autocrop_crop_pad: shape out of range");
    NUNIF_REQUIRE(y0 >= 0 && x0 >= 0 && (int64_t)y0 + win_h <= sH && (int64_t)x0 + win_w <= sW,
                  "autocrop_crop_pad: the window (%d, %d) + %dx%d leaves the %dx%d source", y0, x0, win_h, win_w, sH, sW);
    NUNIF_REQUIRE(pad_top >= 0 && pad_left >= 0 && (int64_t)pad_top + win_h <= dH && (int64_t)pad_left + win_w <= dW,
                  "autocrop_crop_pad: the window (%d, %d) + %dx%d leaves the %dx%d destination", pad_top, pad_left, win_h, win_w, dH,
                  dW);
    CropArgs g;
    g.src = src; g.dst = dst; g.sH = sH; g.sW = sW; g.dH = dH; g.dW = dW; g.y0 = y0; g.x0 = x0; g.pt = pad_top; g.pl = pad_left;
    g.wh = win_h; g.ww = win_w; g.pad = pad_value;
    g.src_vec = (sW % 4 == 0 && aligned16(src)) ? 1 : 0;
    g.quads = (long)N * dH * ((dW + 3) / 4);
    const int grid = (int)std::min<long>((g.quads + 255) / 256, 8192);
    if (dW % 4 == 0 && aligned16(dst)) autocrop_crop_pad_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(g);
    else autocrop_crop_pad_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(g);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
