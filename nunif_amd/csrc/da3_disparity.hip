// Everything iw3 wraps around the Depth-Anything-3 mono backbone (iw3/depth_anything_v3_model.py _forward :33-56, reference) and the
// DA3MonoDisparity model that is to replace its fixed shift (iw3/models/da3mono_disparity.py forward :29-50, extract_features
// :53-73) for gfx950, fp32, batched, without a host synchronisation.
//
// Both need order statistics of a whole depth map: the 0.99 quantile of the non-sky depths (two of them, torch.quantile's linear
// interpolation) and the 64 features (min, 62 ranks, max) the reference reads out of a full torch.sort.  One radix selection over
// the order-preserving keys of common.h serves every rank of an image together: four levels of 8 bits, and per level
//   da3_hist_kernel   many workgroups per image; a pixel is matched against the distinct key prefixes the ranks have reached so far
//                     (at most one per rank, binary search in LDS) and counted in that prefix's 256-bin histogram: packed 16-bit
//                     counters in LDS per 16 Ki pixel chunk, non-zero bins flushed with integer atomics
//   da3_step_kernel   one workgroup per image, one wave per rank in turn: a wave-wide prefix sum over the 256 bins of the rank's
//                     histogram picks the digit and the rank inside it
// Ranks that share a prefix share one histogram, so a constant or two-valued map keeps one or two histograms through all four
// levels; the work is bounded by 4 passes whatever the values are.  Only integer counts are accumulated: the result does not depend
// on the order in which workgroups arrive, and is the same on every call and stream.
//   da3_count_kernel      the non-sky count of _forward :40 (an integer atomic per workgroup)
//   da3_disparity_kernel  :41-52 per pixel, 16 bytes per lane where the image size allows
//   da3mono_mlp_kernel    the 64 -> 128 -> 128 -> 2 MLP, one workgroup per image.  25 k multiply-adds per image: far below what an
//                         MFMA tile pays for, so it is a plain dot product per lane; fp32 operands and activations, the sums kept in
//                         double because every pixel of the image depends on the two scalars it returns
//   da3mono_apply_kernel  :34-48 per pixel
// The file is built without FMA contraction: the pixel formulas round once per operation, in the reference's order.
#include "common.h"
#include "host_weights.h"

namespace nunif {
namespace {

constexpr int kRanks = 64;             // FEAT_DIM
constexpr int kThreads = 1024;
constexpr int kChunk = 16384;          // pixels per histogram workgroup: its counts fit 16 bits
constexpr int kStateWords = 136;       // per image: prefix[64], krem[64], count, q bits, 6 spare
constexpr int kMaxSide = 8192;
constexpr int kMaxBatch = 4096;

struct SelState {
    unsigned prefix[kRanks];           // key bits found so far (high bits first)
    unsigned krem[kRanks];             // rank inside the set of keys that share `prefix`
    unsigned count;                    // non-sky pixels (disparity stage)
    unsigned q_bits;                   // the interpolated quantile of the last raw call (debug_stats)
    unsigned spare[6];
};
static_assert(sizeof(SelState) == kStateWords * 4, "state layout");

enum { MODE_RANKS = 0, MODE_QUANTILE = 1 };

// words of the histograms of one image: one histogram at the first level (no prefix yet), up to R at the three others
__host__ __device__ inline long level_offset(int level, int R) { return level == 0 ? 0 : 256L * (1 + (long)(level - 1) * R); }
inline long hist_words(int R) { return 256L * (1 + 3L * R); }

// The distinct prefixes of the R ranks at this level, sorted: s_groups[0 .. G), and each rank's index into them in s_gid.  Every
// thread of the block calls it.  O(R^2) compares on R lanes; R <= 64.
__device__ __forceinline__ void build_groups(const unsigned *prefix, int R, int shift, unsigned *s_hi, unsigned *s_groups, int *s_first,
                                             int *s_gid, int *s_G) {
    const int tid = threadIdx.x;
    if (tid < R) s_hi[tid] = shift == 24 ? 0u : prefix[tid] >> (shift + 8);
    __syncthreads();
    if (tid < R) {
        int first = 1;
        for (int j = 0; j < tid; ++j) first &= s_hi[j] != s_hi[tid];
        s_first[tid] = first;
    }
    __syncthreads();
    if (tid < R) {
        int below = 0, total = 0;
        for (int j = 0; j < R; ++j) {
            below += s_first[j] && s_hi[j] < s_hi[tid];
            total += s_first[j];
        }
        s_gid[tid] = below;
        if (s_first[tid]) s_groups[below] = s_hi[tid];
        if (tid == 0) *s_G = total;
    }
    __syncthreads();
}

// One count into a packed 16-bit LDS histogram.  Depth maps cluster: whole waves fall into one or two bins (a constant map, the sky
// plateau, the exponent byte of values in [0, 1)), and 64 same-address LDS atomics serialise.  The first two distinct slots of the
// wave are added once each by a leader lane with the number of lanes that agree; whoever is left adds for itself.
__device__ __forceinline__ void wave_hist_add(unsigned *s_hist, bool hit, unsigned slot) {
    unsigned long long rem = __ballot(hit);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (rem == 0ull) break;
        const int leader = __ffsll((long long)rem) - 1;
        const unsigned ls = (unsigned)__shfl((int)slot, leader);
        const unsigned long long same = __ballot(hit && slot == ls);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&s_hist[ls >> 1], (unsigned)__popcll(same) << (16 * (ls & 1)));
        hit = hit && slot != ls;
        rem &= ~same;
    }
    if (hit) atomicAdd(&s_hist[slot >> 1], 1u << (16 * (slot & 1)));
}

__device__ __forceinline__ void hist_one(unsigned *s_hist, const unsigned *s_groups, int G, int shift, bool valid, float v) {
    const unsigned key = order_key(v);
    const unsigned hi = shift == 24 ? 0u : key >> (shift + 8);
    int lo = 0, up = G;
    while (lo < up) {
        const int mid = (lo + up) >> 1;
        if (s_groups[mid] < hi) lo = mid + 1; else up = mid;
    }
    const bool hit = valid && lo < G && s_groups[lo] == hi;
    wave_hist_add(s_hist, hit, (unsigned)lo * 256u + ((key >> shift) & 255u));
}

// grid (chunks of the image, B).  MASKED: only pixels with !(sky > t) count (depth[~sky_mask], _forward :51).  VEC: 4 pixels per lane
// and load; the image size is a multiple of 4 and the base pointers are 16-byte aligned.
template <bool MASKED, bool VEC>
__global__ void __launch_bounds__(kThreads) da3_hist_kernel(const float *__restrict__ depth, const float *__restrict__ sky, float t,
                                                            long n, int R, int shift, unsigned *__restrict__ hist, long hist_image,
                                                            const SelState *__restrict__ state) {
    __shared__ unsigned s_hist[kRanks * 128];
    __shared__ unsigned s_hi[kRanks], s_groups[kRanks];
    __shared__ int s_first[kRanks], s_gid[kRanks], s_G;
    const int tid = threadIdx.x, b = blockIdx.y;
    if (MASKED && state[b].count == 0u) return;                  // all sky: no rank to find (block-uniform)
    build_groups(state[b].prefix, R, shift, s_hi, s_groups, s_first, s_gid, &s_G);
    const int G = s_G;
    for (int i = tid; i < G * 128; i += kThreads) s_hist[i] = 0u;
    __syncthreads();
    const float *d = depth + (long)b * n, *s = MASKED ? sky + (long)b * n : nullptr;
    const long start = (long)blockIdx.x * kChunk, end = min(n, start + (long)kChunk);
    constexpr int V = VEC ? 4 : 1;
    // every lane makes the same number of trips: the ballots inside need whole waves
    for (long base = start; base < end; base += (long)kThreads * V) {
        const long i = base + (long)tid * V;
        if (VEC) {
            const bool in = i < end;                               // n % 4 == 0: a group of four is inside or outside as a whole
            f32x4 dv = {0.f, 0.f, 0.f, 0.f}, sv = {0.f, 0.f, 0.f, 0.f};
            if (in) {
                dv = *reinterpret_cast<const f32x4 *>(d + i);
                if (MASKED) sv = *reinterpret_cast<const f32x4 *>(s + i);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) hist_one(s_hist, s_groups, G, shift, in && !(MASKED && sv[e] > t), dv[e]);
        } else {
            const bool in = i < end;
            const float dv = in ? d[i] : 0.f;
            const bool skyp = MASKED && in && s[i] > t;
            hist_one(s_hist, s_groups, G, shift, in && !skyp, dv);
        }
    }
    __syncthreads();
    unsigned *gh = hist + (long)b * hist_image;
    for (int i = tid; i < G * 128; i += kThreads) {
        const unsigned v = s_hist[i];
        if (v & 0xffffu) atomicAdd(&gh[2 * i], v & 0xffffu);
        if (v >> 16) atomicAdd(&gh[2 * i + 1], v >> 16);
    }
}

// grid (B).  Wave w takes ranks 4w .. 4w + 3.  MODE_RANKS: rank 0 is the minimum, rank 63 the maximum, ranks 1 .. 62 come from
// `ranks` (extract_features :65, computed on the host by the reference's own expression).  MODE_QUANTILE: the two order statistics
// around position 0.99 * (m - 1) of the m non-sky pixels.
template <int MODE>
__global__ void __launch_bounds__(kThreads) da3_step_kernel(const unsigned *__restrict__ hist, long hist_image, SelState *__restrict__ state,
                                                            int R, int shift, long n, const long long *__restrict__ ranks,
                                                            float *__restrict__ out) {
    __shared__ unsigned s_hi[kRanks], s_groups[kRanks];
    __shared__ int s_first[kRanks], s_gid[kRanks], s_G;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SelState *st = state + b;
    const unsigned m = MODE == MODE_QUANTILE ? st->count : 0u;
    if (MODE == MODE_QUANTILE && m == 0u) return;
    build_groups(st->prefix, R, shift, s_hi, s_groups, s_first, s_gid, &s_G);
    const unsigned *gh = hist + (long)b * hist_image;
    for (int r = wave * 4; r < min(wave * 4 + 4, R); ++r) {
        unsigned k;
        if (shift != 24) {
            k = st->krem[r];
        } else if (MODE == MODE_QUANTILE) {
            const double p = 0.99 * (double)(m - 1u);
            k = (unsigned)(r == 0 ? floor(p) : ceil(p));
        } else {
            long long want = r == 0 ? 0 : (r == kRanks - 1 ? n - 1 : ranks[r - 1]);
            want = want < 0 ? 0 : (want > n - 1 ? n - 1 : want);
            k = (unsigned)want;
        }
        const u32x4 c = reinterpret_cast<const u32x4 *>(gh + (long)s_gid[r] * 256)[lane];
        const unsigned mine = c[0] + c[1] + c[2] + c[3];
        unsigned incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = (unsigned)__shfl_up((int)incl, off);
            if (lane >= off) incl += up;
        }
        const unsigned long long over = __ballot(incl > k);
        const int L = over ? __ffsll((long long)over) - 1 : 63;      // the counts of a group always exceed its ranks
        unsigned cum = (unsigned)__shfl((int)(incl - mine), L);
        const unsigned c0 = (unsigned)__shfl((int)c[0], L), c1 = (unsigned)__shfl((int)c[1], L), c2 = (unsigned)__shfl((int)c[2], L);
        int j = 0;
        if (cum + c0 <= k) { cum += c0; j = 1;
            if (cum + c1 <= k) { cum += c1; j = 2;
                if (cum + c2 <= k) { cum += c2; j = 3; } } }
        if (lane == 0) {
            const unsigned prefix = (shift == 24 ? 0u : st->prefix[r]) | ((unsigned)(4 * L + j) << shift);
            st->prefix[r] = prefix;
            st->krem[r] = k - cum;
            if (MODE == MODE_RANKS && shift == 0) out[(long)b * kRanks + r] = key_value(prefix);
        }
    }
}

// grid (chunks, B): count of pixels with !(sky > t)
template <bool VEC>
__global__ void __launch_bounds__(256) da3_count_kernel(const float *__restrict__ sky, float t, long n, SelState *__restrict__ state) {
    __shared__ unsigned s_count;
    const int b = blockIdx.y;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    const float *s = sky + (long)b * n;
    unsigned mine = 0;
    constexpr int V = VEC ? 4 : 1;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (long)gridDim.x * 256 * V) {
        if (VEC) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(s + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) mine += v[e] > t ? 0u : 1u;
        } else {
            mine += s[i] > t ? 0u : 1u;
        }
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(&state[b].count, s_count);
}

// _forward :35, :41-52 for one pixel.  Not raw: (1 / (depth + shift)) * (1 - w).  Raw: min(depth * (1 - w) + w * q, q).
__device__ __forceinline__ float disparity_pixel(float d, float s, float t, float one_m_t, float shift, bool raw, float q) {
    const float w = (fminf(fmaxf(s, t), 1.f) - t) / one_m_t;
    const float keep = 1.f - w;
    if (!raw) return (1.f / (d + shift)) * keep;
    return fminf(d * keep + w * q, q);
}

template <bool VEC>
__global__ void __launch_bounds__(256) da3_disparity_kernel(const float *__restrict__ depth, const float *__restrict__ sky,
                                                            float *__restrict__ out, long n, float t, float one_m_t, float shift, int raw,
                                                            SelState *__restrict__ state) {
    const int b = blockIdx.y;
    const unsigned m = state[b].count;
    // raw: torch.quantile raises on an empty selection; the engine cannot stop the host and answers zeros
    const bool zeros = raw ? m == 0u : m < 10u;                  // :41-43
    float q = 0.f;
    if (raw && !zeros) {
        const double p = 0.99 * (double)(m - 1u), wgt = p - floor(p);
        const double lo = (double)key_value(state[b].prefix[0]), hi = (double)key_value(state[b].prefix[1]);
        q = (float)(lo + (hi - lo) * wgt);
        if (blockIdx.x == 0 && threadIdx.x == 0) state[b].q_bits = __float_as_uint(q);
    }
    const float *d = depth + (long)b * n, *s = sky + (long)b * n;
    float *o = out + (long)b * n;
    constexpr int V = VEC ? 4 : 1;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (long)gridDim.x * 256 * V) {
        if (VEC) {
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            if (!zeros) {
                const f32x4 dv = *reinterpret_cast<const f32x4 *>(d + i), sv = *reinterpret_cast<const f32x4 *>(s + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = disparity_pixel(dv[e], sv[e], t, one_m_t, shift, raw != 0, q);
            }
            *reinterpret_cast<f32x4 *>(o + i) = r;
        } else {
            o[i] = zeros ? 0.f : disparity_pixel(d[i], s[i], t, one_m_t, shift, raw != 0, q);
        }
    }
}

__global__ void da3_debug_stats_kernel(const SelState *__restrict__ state, int B, float *__restrict__ stats, int *__restrict__ counts) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    stats[3 * b + 0] = key_value(state[b].prefix[0]);
    stats[3 * b + 1] = key_value(state[b].prefix[1]);
    stats[3 * b + 2] = __uint_as_float(state[b].q_bits);
    counts[b] = (int)state[b].count;
}

// forward :32.  w0t [64][128] and w1t [128][128] are the transposed Linear weights (lane j reads column j: coalesced), w2 [2][128].
__device__ __forceinline__ float silu(double x) { return (float)(x / (1.0 + exp(-x))); }

__global__ void __launch_bounds__(128) da3mono_mlp_kernel(const float *__restrict__ feat, const float *__restrict__ w0t,
                                                          const float *__restrict__ b0, const float *__restrict__ w1t,
                                                          const float *__restrict__ b1, const float *__restrict__ w2,
                                                          const float *__restrict__ b2, float *__restrict__ out) {
    __shared__ float s_x[kRanks], s_h1[128], s_h2[128];
    const int j = threadIdx.x, b = blockIdx.x;
    if (j < kRanks) s_x[j] = feat[(long)b * kRanks + j];
    __syncthreads();
    double acc = (double)b0[j];
    for (int i = 0; i < kRanks; ++i) acc += (double)w0t[i * 128 + j] * (double)s_x[i];
    s_h1[j] = silu(acc);
    __syncthreads();
    acc = (double)b1[j];
    for (int i = 0; i < 128; ++i) acc += (double)w1t[i * 128 + j] * (double)s_h1[i];
    s_h2[j] = silu(acc);
    __syncthreads();
    if (j < 2) {
        acc = (double)b2[j];
        for (int i = 0; i < 128; ++i) acc += (double)w2[j * 128 + i] * (double)s_h2[i];
        out[2 * b + j] = fmaxf((float)acc, 0.f);
    }
}

// forward :34-48: the sky is where the depth equals its maximum (feature 63, exact); sky_shift is added there, then 1 / (depth + shift)
__device__ __forceinline__ float apply_pixel(float d, float maxv, float shift, float sky_shift) {
    const float moved = d == maxv ? d + sky_shift : d;
    return 1.f / (moved + shift);
}

template <bool VEC>
__global__ void __launch_bounds__(256) da3mono_apply_kernel(const float *__restrict__ depth, float *__restrict__ out, long n,
                                                            const float *__restrict__ feat, const float *__restrict__ mlp) {
    const int b = blockIdx.y;
    const float maxv = feat[(long)b * kRanks + kRanks - 1], shift = mlp[2 * b], sky_shift = mlp[2 * b + 1];
    const float *d = depth + (long)b * n;
    float *o = out + (long)b * n;
    constexpr int V = VEC ? 4 : 1;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * V; i < n; i += (long)gridDim.x * 256 * V) {
        if (VEC) {
            const f32x4 dv = *reinterpret_cast<const f32x4 *>(d + i);
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = apply_pixel(dv[e], maxv, shift, sky_shift);
            *reinterpret_cast<f32x4 *>(o + i) = r;
        } else {
            o[i] = apply_pixel(d[i], maxv, shift, sky_shift);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
inline long select_bytes(int B, int R) { return (long)B * (hist_words(R) + kStateWords) * 4; }
inline bool shape_ok(int B, int H, int W) {
    return B > 0 && B <= kMaxBatch && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide && (long)H * W >= 3;
}
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int pixel_blocks(long n, int V) { return (int)std::min<long>((n + 256L * V - 1) / (256L * V), 2048L); }

// The four histogram / step pairs of one selection.  ws: [B][hist_words(R)] histograms (zeroed here), then [B] SelState.
template <int MODE>
int launch_select(const float *depth, const float *sky, float t, int B, long n, int R, const long long *ranks, float *out,
                  unsigned *hist, SelState *state, bool vec, hipStream_t s) {
    const long hist_image = hist_words(R);
    const dim3 grid((unsigned)((n + kChunk - 1) / kChunk), (unsigned)B);
    for (int level = 0; level < 4; ++level) {
        const int shift = 24 - 8 * level;
        unsigned *h = hist + level_offset(level, R);
        if (MODE == MODE_QUANTILE) {
            if (vec) da3_hist_kernel<true, true><<<grid, kThreads, 0, s>>>(depth, sky, t, n, R, shift, h, hist_image, state);
            else da3_hist_kernel<true, false><<<grid, kThreads, 0, s>>>(depth, sky, t, n, R, shift, h, hist_image, state);
        } else {
            if (vec) da3_hist_kernel<false, true><<<grid, kThreads, 0, s>>>(depth, nullptr, 0.f, n, R, shift, h, hist_image, state);
            else da3_hist_kernel<false, false><<<grid, kThreads, 0, s>>>(depth, nullptr, 0.f, n, R, shift, h, hist_image, state);
        }
        NUNIF_LAUNCH_CHECK();
        da3_step_kernel<MODE><<<B, kThreads, 0, s>>>(h, hist_image, state, R, shift, n, ranks, out);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}

int launch_features(const float *depth, int B, long n, const long long *ranks, float *out, void *workspace, hipStream_t s) {
    unsigned *hist = static_cast<unsigned *>(workspace);
    SelState *state = reinterpret_cast<SelState *>(hist + (long)B * hist_words(kRanks));
    NUNIF_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)select_bytes(B, kRanks), s));
    return launch_select<MODE_RANKS>(depth, nullptr, 0.f, B, n, kRanks, ranks, out, hist, state, n % 4 == 0 && aligned16(depth), s);
}

}  // namespace
}  // namespace nunif

using namespace nunif;

struct nunif_da3mono {
    DeviceOwner mem;
    float *w0t = nullptr, *b0 = nullptr, *w1t = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
};

extern "C" int64_t nunif_hip_da3_disparity_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (!shape_ok(B, H, W)) return -1;
    return select_bytes(B, 2);
}

extern "C" int nunif_hip_da3_disparity(const float *depth, const float *sky, int32_t B, int32_t H, int32_t W, double sky_thresh,
                                       double shift, int32_t raw_output, float *out, void *workspace, int64_t workspace_bytes,
                                       void *stream) {
    NUNIF_REQUIRE(depth && sky && out && workspace, "da3_disparity: NULL argument");
    NUNIF_REQUIRE(shape_ok(B, H, W), "da3_disparity: bad shape B=%d H=%d W=%d (1 <= H, W <= %d, H * W >= 3)", B, H, W, kMaxSide);
    NUNIF_REQUIRE(sky_thresh < 1.0, "da3_disparity: sky_thresh %g must be below 1", sky_thresh);
    NUNIF_REQUIRE(aligned16(workspace) && workspace_bytes >= select_bytes(B, 2),
                  "da3_disparity: workspace of %lld bytes (need %ld, 16-byte aligned)", (long long)workspace_bytes, select_bytes(B, 2));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long n = (long)H * W;
    const float t = (float)sky_thresh, one_m_t = (float)(1.0 - sky_thresh);
    unsigned *hist = static_cast<unsigned *>(workspace);
    SelState *state = reinterpret_cast<SelState *>(hist + (long)B * hist_words(2));
    const bool vec = n % 4 == 0 && aligned16(depth) && aligned16(sky) && aligned16(out);
    const int V = vec ? 4 : 1;
    ProfScope prof("da3_disparity", s, 0.0, (double)B * n * 12.0);
    NUNIF_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)select_bytes(B, 2), s));
    const dim3 grid((unsigned)pixel_blocks(n, V), (unsigned)B);
    if (vec) da3_count_kernel<true><<<grid, 256, 0, s>>>(sky, t, n, state);
    else da3_count_kernel<false><<<grid, 256, 0, s>>>(sky, t, n, state);
    NUNIF_LAUNCH_CHECK();
    if (raw_output) {
        const int st = launch_select<MODE_QUANTILE>(depth, sky, t, B, n, 2, nullptr, nullptr, hist, state, vec, s);
        if (st != NUNIF_HIP_OK) return st;
    }
    if (vec) da3_disparity_kernel<true><<<grid, 256, 0, s>>>(depth, sky, out, n, t, one_m_t, (float)shift, raw_output ? 1 : 0, state);
    else da3_disparity_kernel<false><<<grid, 256, 0, s>>>(depth, sky, out, n, t, one_m_t, (float)shift, raw_output ? 1 : 0, state);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_da3_disparity_debug_stats(const void *workspace, int32_t B, float *stats, int32_t *counts, void *stream) {
    NUNIF_REQUIRE(workspace && stats && counts && B > 0 && B <= kMaxBatch, "da3_disparity_debug_stats: bad argument");
    const SelState *state = reinterpret_cast<const SelState *>(static_cast<const unsigned *>(workspace) + (long)B * hist_words(2));
    da3_debug_stats_kernel<<<cdiv(B, 64), 64, 0, static_cast<hipStream_t>(stream)>>>(state, B, stats, counts);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int64_t nunif_hip_da3mono_features_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (!shape_ok(B, H, W)) return -1;
    return select_bytes(B, kRanks);
}

extern "C" int nunif_hip_da3mono_features(const float *depth, int32_t B, int32_t H, int32_t W, const int64_t *ranks, float *out,
                                          void *workspace, int64_t workspace_bytes, void *stream) {
    NUNIF_REQUIRE(depth && ranks && out && workspace, "da3mono_features: NULL argument");
    NUNIF_REQUIRE(shape_ok(B, H, W), "da3mono_features: bad shape B=%d H=%d W=%d (1 <= H, W <= %d, H * W >= 3)", B, H, W, kMaxSide);
    NUNIF_REQUIRE(aligned16(workspace) && workspace_bytes >= select_bytes(B, kRanks),
                  "da3mono_features: workspace of %lld bytes (need %ld, 16-byte aligned)", (long long)workspace_bytes,
                  select_bytes(B, kRanks));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ProfScope prof("da3mono_features", s, 0.0, (double)B * H * W * 16.0);
    return launch_features(depth, B, (long)H * W, reinterpret_cast<const long long *>(ranks), out, workspace, s);
}

extern "C" int nunif_hip_da3mono_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_da3mono **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "da3mono_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_da3mono *net = new nunif_da3mono();
    const struct { const char *name; long count; float **dev; } want[6] = {
        {"mlp.0.wt", 64 * 128, &net->w0t}, {"mlp.0.bias", 128, &net->b0}, {"mlp.2.wt", 128 * 128, &net->w1t},
        {"mlp.2.bias", 128, &net->b1}, {"mlp.4.weight", 2 * 128, &net->w2}, {"mlp.4.bias", 2, &net->b2}};
    int rc = NUNIF_HIP_OK;
    for (int k = 0; k < 6 && rc == NUNIF_HIP_OK; ++k) {
        const HostTensor *t = nullptr;
        rc = find(m, want[k].name, &t);
        if (rc == NUNIF_HIP_OK && t->numel != want[k].count) {
            set_error("da3mono_create: tensor %s has %lld floats, not %ld", want[k].name, (long long)t->numel, want[k].count);
            rc = NUNIF_HIP_EINVAL;
        }
        if (rc == NUNIF_HIP_OK) rc = net->mem.upload_f32(t, want[k].dev);
    }
    if (rc != NUNIF_HIP_OK) {
        net->mem.free_all();
        delete net;
        return rc;
    }
    *handle = net;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_da3mono_destroy(nunif_da3mono *handle) {
    if (!handle) return;
    handle->mem.free_all();
    delete handle;
}

extern "C" int64_t nunif_hip_da3mono_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (!shape_ok(B, H, W)) return -1;
    return select_bytes(B, kRanks) + (long)B * (kRanks + 4) * 4;
}

extern "C" int nunif_hip_da3mono_forward(nunif_da3mono *handle, const float *depth, int32_t B, int32_t H, int32_t W,
                                         const int64_t *ranks, float *out, void *workspace, int64_t workspace_bytes, void *stream) {
    NUNIF_REQUIRE(handle && depth && ranks && out && workspace, "da3mono_forward: NULL argument");
    NUNIF_REQUIRE(shape_ok(B, H, W), "da3mono_forward: bad shape B=%d H=%d W=%d (1 <= H, W <= %d, H * W >= 3)", B, H, W, kMaxSide);
    const long need = select_bytes(B, kRanks) + (long)B * (kRanks + 4) * 4;
    NUNIF_REQUIRE(aligned16(workspace) && workspace_bytes >= need, "da3mono_forward: workspace of %lld bytes (need %ld, 16-byte aligned)",
                  (long long)workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long n = (long)H * W;
    float *feat = reinterpret_cast<float *>(static_cast<char *>(workspace) + select_bytes(B, kRanks));
    float *mlp = feat + (long)B * kRanks;
    ProfScope prof("da3mono_forward", s, 0.0, (double)B * n * 24.0);
    const int st = launch_features(depth, B, n, reinterpret_cast<const long long *>(ranks), feat, workspace, s);
    if (st != NUNIF_HIP_OK) return st;
    da3mono_mlp_kernel<<<B, 128, 0, s>>>(feat, handle->w0t, handle->b0, handle->w1t, handle->b1, handle->w2, handle->b2, mlp);
    NUNIF_LAUNCH_CHECK();
    const bool vec = n % 4 == 0 && aligned16(depth) && aligned16(out);
    const dim3 grid((unsigned)pixel_blocks(n, vec ? 4 : 1), (unsigned)B);
    if (vec) da3mono_apply_kernel<true><<<grid, 256, 0, s>>>(depth, out, n, feat, mlp);
    else da3mono_apply_kernel<false><<<grid, 256, 0, s>>>(depth, out, n, feat, mlp);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
