// stlizer pass 2 for gfx950: the batch form of find_transform (nunif/utils/superpoint.py:233-327, reference), a torch autograd loop
// of `iteration` Adam steps over a few KB per pair, as iteration + 1 launches of one kernel, one workgroup per pair, no host
// synchronisation and no waiting of one workgroup on another: the order between steps is the kernel boundary.
//
// The reference's loss is a mean over the WHOLE batch (:305, :309), so a pair's gradient is its own sum of signs divided by the
// batch's selected-element count of that step.  That count is only known when every workgroup of the step has finished, hence the
// Adam step is deferred: launch s leaves the pair's four gradient sums in its state and adds its integer count to slot s of the
// workspace (the only atomics), and launch s + 1 divides, steps Adam and goes on with the next forward.  Nothing else couples the
// pairs, and an integer sum has no order: the result is bit-equal across calls and streams and under any permutation of the pairs.
//
//   launch 0            centre, norm_scale (a block maximum), normalise into the workspace, initialise, forward 0
//   launch 1 .. it - 1  Adam step s - 1 (thread 0; four parameters), forward s
//   launch it           Adam step it - 1, outputs
//
// A forward is up to three passes over the pair's normalised points (N <= 8192: 64 KB, L2-resident): the masked mean of the
// element losses, their population deviation about it, and the selection with the four gradient sums.  Every sum is a double, taken
// by each lane over its own strided points in index order and then over the lanes by a fixed shuffle tree: the same bits whatever
// else runs.  The point arithmetic itself is fp32 in the reference's order, one rounding per operation (built without contraction).
// 8 bytes per lane and load; the kernel is latency bound (a few hundred points per pair is the common case), not bandwidth bound.
#include "common.h"

#include <cfloat>
#include <cmath>

namespace nunif {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBatch = 4096;
constexpr int kMaxPoints = 8192;
constexpr int kMaxIteration = 1024;
constexpr float kBeta2 = 0.9f, kOneMinusBeta2 = 0.1f, kEps = 1e-8f;      // betas (0.5, 0.9) :267; 1 - beta1 = 0.5 is the lerp weight

struct PairState {
    float p[4];                    // tx, ty, scale, rotation
    float m[4], v[4];              // Adam exp_avg, exp_avg_sq
    float norm_scale;
    float pad[3];
    double g[4];                   // gradient sums of the last forward, before the division by the batch's count
};
static_assert(sizeof(PairState) == 96, "state layout");

struct StepArgs {
    int s, iteration, flags, outliers;      // outliers: this forward rejects them (sigma given and s > 0)
    float step_t, step_sr;                  // lr / bias_correction1 of Adam step s - 1, translation and scale / rotation
    float bc2_sqrt;                         // sqrt(bias_correction2) of that step
    float sigma;                            // of forward s
};

struct Layout {
    long counts, state, xy1n, xy2n, total;
};
inline long align256(long v) { return (v + 255) / 256 * 256; }
inline Layout layout(int B, int N, int iteration) {
    Layout l;
    l.counts = 0;
    l.state = align256(4L * iteration);
    l.xy1n = l.state + align256((long)sizeof(PairState) * B);
    l.xy2n = l.xy1n + align256(8L * B * N);
    l.total = l.xy2n + align256(8L * B * N);
    return l;
}
inline bool shape_ok(int B, int N, int iteration) {
    return B >= 1 && B <= kMaxBatch && N >= 1 && N <= kMaxPoints && iteration >= 1 && iteration <= kMaxIteration;
}

__device__ __forceinline__ float nan_to_num(float v) { return v != v ? 0.f : fminf(fmaxf(v, -FLT_MAX), FLT_MAX); }
__device__ __forceinline__ float sign0(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Sums of K doubles and one int over the block, the same in every thread: lanes by a shuffle tree, then the four waves in order.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], int &n, double (*s_red)[8], int *s_n) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_down(v[k], o);
        n += __shfl_down(n, o);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_red[wave][k] = v[k];
        s_n[wave] = n;
    }
    __syncthreads();
    n = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += s_red[w][k];
        n += s_n[w];
    }
}

struct Elem {
    float rx, ry, dx, dy, lx, ly;
    bool mx, my;
};

// rotate, scale, translate, |xy' - xy2| of one point (:282-297), and its two mask bytes
__device__ __forceinline__ Elem forward_point(const float2 *__restrict__ xy1n, const float2 *__restrict__ xy2n,
                                              const uchar2 *__restrict__ mask, long at, float tx, float ty, float sc, float rc, float rs) {
    const float2 p = xy1n[at], q = xy2n[at];
    Elem e;
    e.rx = p.x * rc - p.y * rs;
    e.ry = p.x * rs + p.y * rc;
    e.dx = (e.rx * sc + tx) - q.x;
    e.dy = (e.ry * sc + ty) - q.y;
    e.lx = fabsf(e.dx);
    e.ly = fabsf(e.dy);
    e.mx = e.my = true;
    if (mask) {
        const uchar2 m = mask[at];
        e.mx = m.x != 0;
        e.my = m.y != 0;
    }
    return e;
}

// grid B.  All pointers are indexed by the pair; `counts` is the only memory the workgroups share.
__global__ void __launch_bounds__(kThreads)
find_transform_step_kernel(const float2 *__restrict__ xy1, const float2 *__restrict__ xy2, const uchar2 *__restrict__ mask,
                           const float2 *__restrict__ center, int B, int N, StepArgs a, int *__restrict__ counts,
                           PairState *__restrict__ state, float2 *__restrict__ xy1n, float2 *__restrict__ xy2n,
                           float *__restrict__ shift_out, float *__restrict__ scale_out, float *__restrict__ angle_out,
                           float *__restrict__ trace) {
    __shared__ double s_red[kWaves][8];
    __shared__ int s_n[kWaves];
    __shared__ float s_max[kWaves];
    __shared__ float s_par[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long base = (long)b * N;
    PairState *st = state + b;

    if (a.s == 0) {
        const float2 c = center[b];
        float amax = 0.f;
        for (int i = tid; i < N; i += kThreads) {
            const float2 p = xy1[base + i];
            amax = fmaxf(amax, fmaxf(fabsf(nan_to_num(p.x - c.x)), fabsf(nan_to_num(p.y - c.y))));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_down(amax, o));
        if ((tid & 63) == 0) s_max[tid >> 6] = amax;
        __syncthreads();
        amax = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
        // every lane reads back below exactly the points it writes here
        for (int i = tid; i < N; i += kThreads) {
            const float2 p = xy1[base + i], q = xy2[base + i];
            xy1n[base + i] = make_float2((p.x - c.x) / amax, (p.y - c.y) / amax);
            xy2n[base + i] = make_float2((q.x - c.x) / amax, (q.y - c.y) / amax);
        }
        if (tid == 0) {
            for (int k = 0; k < 4; ++k) {
                st->p[k] = k == 2 ? 1.f : 0.f;
                st->m[k] = st->v[k] = 0.f;
                s_par[k] = st->p[k];
            }
            st->norm_scale = amax;
        }
    } else if (tid == 0) {
        // torch.optim.Adam (single tensor form) step s - 1, operation by operation
        const int total = counts[a.s - 1];
        for (int k = 0; k < 4; ++k) {
            float p = st->p[k];
            const int frozen = k < 2 ? (a.flags & NUNIF_FIND_TRANSFORM_DISABLE_SHIFT)
                                     : (k == 2 ? (a.flags & NUNIF_FIND_TRANSFORM_DISABLE_SCALE) : (a.flags & NUNIF_FIND_TRANSFORM_DISABLE_ROTATE));
            if (!frozen) {
                const float g = total > 0 ? (float)(st->g[k] / (double)total) : 0.f;
                float m = st->m[k], v = st->v[k];
                m = g - (g - m) * 0.5f;                                   // exp_avg.lerp_(grad, 1 - beta1), weight >= 0.5 form
                v = v * kBeta2 + (kOneMinusBeta2 * g) * g;                // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
                const float denom = sqrtf(v) / a.bc2_sqrt + kEps;
                p = p + ((k < 2 ? -a.step_t : -a.step_sr) * m) / denom;   // param.addcdiv_(exp_avg, denom, value=-step_size)
                st->m[k] = m;
                st->v[k] = v;
                st->p[k] = p;
            }
            s_par[k] = p;
            if (trace) trace[((long)(a.s - 1) * B + b) * 4 + k] = p;
        }
    }
    __syncthreads();
    const float tx = s_par[0], ty = s_par[1], sc = s_par[2], rot = s_par[3];

    if (a.s == a.iteration) {
        if (tid == 0) {
            const float ns = st->norm_scale;
            shift_out[2 * b] = tx * ns;
            shift_out[2 * b + 1] = ty * ns;
            scale_out[b] = sc;
            angle_out[b] = atan2f(sinf(rot), cosf(rot)) * (180.f / 3.14159265358979323846f);
        }
        return;
    }

    const float rc = cosf(rot), rs = sinf(rot);
    float mean = 0.f, stdv = 0.f;
    if (a.outliers) {
        double sum[1] = {0.0};
        int cnt = 0;
        for (int i = tid; i < N; i += kThreads) {
            const Elem e = forward_point(xy1n, xy2n, mask, base + i, tx, ty, sc, rc, rs);
            if (e.mx) { sum[0] += (double)e.lx; ++cnt; }
            if (e.my) { sum[0] += (double)e.ly; ++cnt; }
        }
        block_sum<1>(sum, cnt, s_red, s_n);
        mean = (float)(sum[0] / (double)cnt);                              // no masked element: NaN, nothing is selected
        double sq[1] = {0.0};
        int unused = 0;
        for (int i = tid; i < N; i += kThreads) {
            const Elem e = forward_point(xy1n, xy2n, mask, base + i, tx, ty, sc, rc, rs);
            const double ex = (double)(e.lx - mean), ey = (double)(e.ly - mean);
            if (e.mx) sq[0] += ex * ex;
            if (e.my) sq[0] += ey * ey;
        }
        block_sum<1>(sq, unused, s_red, s_n);
        stdv = (float)sqrt(sq[0] / (double)cnt);
    }

    double g[4] = {0.0, 0.0, 0.0, 0.0};
    int sel = 0;
    for (int i = tid; i < N; i += kThreads) {
        const Elem e = forward_point(xy1n, xy2n, mask, base + i, tx, ty, sc, rc, rs);
        bool kx = e.mx, ky = e.my;
        if (a.outliers) {                                                  // one-sided; a zero deviation gives NaN or inf: false
            kx = kx && (e.lx - mean) / stdv < a.sigma;
            ky = ky && (e.ly - mean) / stdv < a.sigma;
        }
        const float sx = kx ? sign0(e.dx) : 0.f, sy = ky ? sign0(e.dy) : 0.f;
        g[0] += (double)sx;
        g[1] += (double)sy;
        g[2] += (double)(sx * e.rx) + (double)(sy * e.ry);
        g[3] += (double)(sy * e.rx) - (double)(sx * e.ry);
        sel += (kx ? 1 : 0) + (ky ? 1 : 0);
    }
    block_sum<4>(g, sel, s_red, s_n);
    if (tid == 0) {
        st->g[0] = g[0];
        st->g[1] = g[1];
        st->g[2] = g[2];
        st->g[3] = g[3] * (double)sc;
        if (sel > 0) atomicAdd(&counts[a.s], sel);
    }
}

inline bool aligned(const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace
}  // namespace nunif

using namespace nunif;

extern "C" int64_t nunif_hip_find_transform_workspace_bytes(int32_t B, int32_t N, int32_t iteration) {
    if (!shape_ok(B, N, iteration)) return -1;
    return layout(B, N, iteration).total;
}

extern "C" int nunif_hip_find_transform(const float *xy1, const float *xy2, const uint8_t *mask_or_null, const float *center,
                                        int32_t B, int32_t N, int32_t iteration, double lr_translation, double lr_scale_rotation,
                                        double sigma, double sigma_min, double sigma_max, int32_t flags, float *shift_out,
                                        float *scale_out, float *angle_out, void *workspace, int64_t workspace_bytes,
                                        float *trace_or_null, void *stream) {
    NUNIF_REQUIRE(shape_ok(B, N, iteration), "find_transform: bad shape B=%d N=%d iteration=%d (1 <= B <= %d, 1 <= N <= %d, 1 <= iteration <= %d)",
                  B, N, iteration, kMaxBatch, kMaxPoints, kMaxIteration);
    NUNIF_REQUIRE(xy1 && xy2 && center && shift_out && scale_out && angle_out && workspace, "find_transform: NULL argument");
    NUNIF_REQUIRE((flags & ~31) == 0, "find_transform: unknown flags 0x%x", flags);
    NUNIF_REQUIRE(aligned(xy1, 8) && aligned(xy2, 8) && aligned(center, 8) && aligned(mask_or_null, 2),
                  "find_transform: xy1, xy2, center must be 8-byte and mask 2-byte aligned");
    const Layout l = layout(B, N, iteration);
    NUNIF_REQUIRE(aligned(workspace, 256) && workspace_bytes >= l.total, "find_transform: workspace of %lld bytes (need %ld, 256-byte aligned)",
                  (long long)workspace_bytes, l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    int *counts = reinterpret_cast<int *>(ws + l.counts);
    PairState *state = reinterpret_cast<PairState *>(ws + l.state);
    float2 *xy1n = reinterpret_cast<float2 *>(ws + l.xy1n), *xy2n = reinterpret_cast<float2 *>(ws + l.xy2n);
    const bool has_sigma = (flags & (NUNIF_FIND_TRANSFORM_SIGMA | NUNIF_FIND_TRANSFORM_SIGMA_MIN)) != 0;
    const double eta_min = lr_scale_rotation * 1e-3;
    ProfScope prof("find_transform", s, 0.0, (double)B * N * 16.0 * (iteration + 1));
    NUNIF_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)l.state, s));
    for (int step = 0; step <= iteration; ++step) {
        StepArgs a = {};
        a.s = step;
        a.iteration = iteration;
        a.flags = flags;
        a.outliers = has_sigma && step > 0 && step < iteration;
        if (step > 0) {
            // CosineAnnealingWarmRestarts at T_cur = step - 1 and Adam's bias corrections of its step `step`, in double as Python has them
            const int t = step - 1;
            const double w = (1.0 + std::cos(M_PI * (double)t / (double)iteration)) / 2.0;
            const double bc1 = 1.0 - std::pow(0.5, (double)step), bc2 = 1.0 - std::pow(0.9, (double)step);
            a.step_t = (float)((eta_min + (lr_translation - eta_min) * w) / bc1);
            a.step_sr = (float)((eta_min + (lr_scale_rotation - eta_min) * w) / bc1);
            a.bc2_sqrt = (float)std::sqrt(bc2);
        }
        if (a.outliers) {
            double sg = sigma;
            if (flags & NUNIF_FIND_TRANSFORM_SIGMA_MIN)                    // cosine_annealing(sigma_min, sigma_max, step, iteration) :226-230
                sg = sigma_min + 0.5 * (sigma_max - sigma_min) * (1.0 + std::cos(((double)step / (double)iteration) * M_PI));
            a.sigma = (float)sg;
        }
        find_transform_step_kernel<<<B, kThreads, 0, s>>>(reinterpret_cast<const float2 *>(xy1), reinterpret_cast<const float2 *>(xy2),
                                                          reinterpret_cast<const uchar2 *>(mask_or_null),
                                                          reinterpret_cast<const float2 *>(center), B, N, a, counts, state, xy1n, xy2n,
                                                          shift_out, scale_out, angle_out, trace_or_null);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}
