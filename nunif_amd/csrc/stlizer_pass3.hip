// stlizer pass 3 for gfx950 (stlizer/multipass_pipeline.py:86-105, :272-366, reference): the scene weights, the weighted prefix
// sums of a video's path, the two smoothing filters, and grad_opt, the reference's torch.optim.LBFGS(history_size=10, max_iter=4)
// loop of `iteration` steps over three float64 vectors of N + 3 elements, restated decision for decision.
//
// grad_opt never reads anything back.  The host enqueues 1 + iteration * 4 * 22 + 1 launches whatever the data (the schedule is in
// stlizer_pass3_host.h); every data-dependent decision is taken by the begin launch of a slot (the gtd exit by its move launch),
// the same in every workgroup because each finishes the same per-workgroup partials in the same order, and workgroup (0, 0) writes
// it into the slot's record for the launches that follow.  A launch whose iteration does not run returns at once.  No workgroup
// waits on another, there are no float atomics, and every loop bound is a launch argument: the result is bit-equal across calls,
// streams and workspaces.
//
// The closure is the closed form: the objective is quadratic (stlizer_pass3_host.h has the schedule, tests/stlizer_pass3_ref.py the
// formula), its gradient a 7-point stencil that the move launch evaluates from a tile of x with a 3-element halo.  The file is
// built without contraction: every multiply and add is one rounding, as in the float64 restatement the tests compare with.
#include "common.h"
#include "stlizer_pass3_host.h"

#include <cmath>

namespace nunif {
namespace {

using namespace pass3;

constexpr int kThreads = kTile;
constexpr int kWaves = kThreads / 64;
// quantities of the move launch's partials
enum { Q_LOSS = 0, Q_MAXG, Q_SUMABS, Q_MAXDT, Q_YS, Q_YY };
constexpr unsigned kMoveMax = (1u << Q_MAXG) | (1u << Q_MAXDT);
constexpr int kMoveLaunch = kLaunchesPerSlot - 1, kGtdLaunch = kLaunchesPerSlot - 2, kMidLaunch = kHistory;

struct Ws {
    double *rec, *ro, *x, *t, *w, *g, *q, *S, *Y, *partials;
    int M, Mp, nparts;
    long vec;                                   // doubles of one [3][Mp] vector
};

struct EvalConsts {
    double c[3], h[3];                          // 2 gw / (M - k) and gw / (M - k), k = 1..3
    double cp, hp;                              // 2 pw / M and pw / M
    double rw;                                  // resolution / 320
};

// x is held as an unevaluated sum hi + lo of two doubles.  The differences of the closure cancel most of x (a path of magnitude 10
// to 100 against frame-to-frame steps of 1), so the rounding of a float64 x is what the gradient amplifies: with x in one double
// the iterates between the steps carry ten times the error of the result.  hi is what the trace and the decisions see.
struct dd {
    double h, l;
};
__device__ __forceinline__ dd dd_renorm(double s, double e) {
    dd r;
    r.h = s + e;
    r.l = e - (r.h - s);
    return r;
}
__device__ __forceinline__ dd dd_sub(dd a, dd b) {                         // TwoSum of the high words, then the low words
    const double s = a.h - b.h, bb = s - a.h;
    const double e = (a.h - (s - bb)) + (-b.h - bb);
    return dd_renorm(s, e + (a.l - b.l));
}
__device__ __forceinline__ dd dd_axpy(dd x, double t, double d) {            // x + t * d, the product exact by fma
    const double ph = t * d, pl = fma(t, d, -ph);
    const double s = x.h + ph, bb = s - x.h;
    const double e = (x.h - (s - bb)) + (ph - bb);
    return dd_renorm(s, e + (x.l + pl));
}

// NaN wins, as in torch's max
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }

// K sums (bits of `maxes`: maxima) over the block, the same in every thread: lanes by a shuffle tree, then the waves in order.
template <int K>
__device__ __forceinline__ void block_reduce(double (&v)[K], unsigned maxes, double (*s_red)[kQuantities]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double other = __shfl_down(v[k], o);
            v[k] = (maxes >> k) & 1 ? max_nan(v[k], other) : v[k] + other;
        }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double r = s_red[0][k];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) r = (maxes >> k) & 1 ? max_nan(r, s_red[w][k]) : r + s_red[w][k];
        v[k] = r;
    }
}

// Finishes the K quantities of one launch's partials: each thread its strided share in index order, then the block.
template <int K>
__device__ __forceinline__ void finish(const Ws &ws, int launch, unsigned maxes, double (&v)[K], double (*s_red)[kQuantities]) {
    const double *buf = ws.partials + (long)launch * kQuantities * ws.nparts;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double r = 0.0;
        for (int p = threadIdx.x; p < ws.nparts; p += kThreads) {
            const double o = buf[(long)k * ws.nparts + p];
            r = (maxes >> k) & 1 ? max_nan(r, o) : r + o;
        }
        v[k] = r;
    }
    block_reduce<K>(v, maxes, s_red);
}

__device__ __forceinline__ bool is_writer() { return threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0; }
__device__ __forceinline__ double *partial(const Ws &ws, int launch, int quantity) {
    return ws.partials + ((long)launch * kQuantities + quantity) * ws.nparts + blockIdx.y * gridDim.x + blockIdx.x;
}

// ---------------------------------------------------------------------------------------------------------------- begin
// grid (tiles, 3).  Every decision of slot j but the gtd exit; then q = -g and the first dot of the two-loop recursion.
__global__ void __launch_bounds__(kThreads) pass3_begin_kernel(Ws ws, int j) {
    __shared__ double s_red[kWaves][kQuantities];
    double v[kQuantities];
    finish<kQuantities>(ws, kMoveLaunch, kMoveMax, v, s_red);
    const double loss = v[Q_LOSS], maxg = v[Q_MAXG];
    double *cur = ws.rec + (long)j * kRecDoubles;
    double *prev = ws.rec + (long)(j > 0 ? j - 1 : 0) * kRecDoubles;
    const int k = j % kMaxIter;
    const bool writer = is_writer();

    double t = 1.0, hdiag = 1.0;
    int head = 0, num_old = 0, niter = 0, stale = 1, xbuf = 0;
    bool ran_prev = false;
    if (j > 0) {
        t = prev[R_T];
        hdiag = prev[R_HDIAG];
        head = (int)prev[R_HEAD];
        num_old = (int)prev[R_NUM_OLD];
        niter = (int)prev[R_NITER];
        const bool gtd_exit = prev[R_EXIT_GTD] != 0.0;
        ran_prev = prev[R_ACTIVE] != 0.0 && !gtd_exit;                       // the previous slot moved x
        stale = gtd_exit ? 1 : (prev[R_ACTIVE] != 0.0 ? 0 : (int)prev[R_STALE]);
        xbuf = ran_prev ? 1 - (int)prev[R_XBUF] : (int)prev[R_XBUF];
    }
    // the three exits after the re-evaluation of the previous iteration; its 4th iteration of a step has none (lbfgs.py:493-526)
    int exit_after = 0;
    if (k != 0 && ran_prev) {
        const double dloss = fabs(loss - prev[R_LOSS]);
        exit_after = exit_after_code(maxg, v[Q_MAXDT], dloss);
        if (writer) {
            prev[R_EXIT_AFTER] = exit_after;
            prev[R_MAXG_NEW] = maxg;
            prev[R_MAXDT] = v[Q_MAXDT];
            prev[R_DLOSS] = dloss;
        }
    }
    bool active = k == 0 ? true : (ran_prev && exit_after == 0);
    int exit_begin = 0;
    if (k == 0 && maxg <= kTolGrad) {                                        // opt_cond at step entry (:370-374)
        active = false;
        exit_begin = 1;
    } else if (!active) {
        exit_begin = 6;
    }
    int accepted = -1;
    if (active) {
        ++niter;
        if (niter > 1) {                                                     // the memory update (:404-421)
            const double ys = stale ? 0.0 : v[Q_YS];
            accepted = ys > kYsMin ? 1 : 0;
            if (accepted) {
                head = (head + 1) % kRing;
                num_old = num_old < kHistory ? num_old + 1 : kHistory;
                hdiag = ys / v[Q_YY];
                if (writer) ws.ro[head] = 1.0 / ys;
            }
        }
        t = niter == 1 ? fmin(1.0, 1.0 / v[Q_SUMABS]) : 1.0;                 // :454-457
    }
    if (writer) {
        const double nan = __builtin_nan("");
        for (int f = 0; f < kRecDoubles; ++f) cur[f] = 0.0;
        cur[R_ACTIVE] = active;
        cur[R_EXIT_BEGIN] = exit_begin;
        cur[R_ACCEPTED] = accepted;
        cur[R_LOSS] = loss;
        cur[R_MAXG] = maxg;
        cur[R_GTD] = cur[R_MAXG_NEW] = cur[R_MAXDT] = cur[R_DLOSS] = nan;
        cur[R_YS] = accepted >= 0 ? (stale ? 0.0 : v[Q_YS]) : nan;
        cur[R_T] = t;
        cur[R_HDIAG] = hdiag;
        cur[R_HEAD] = head;
        cur[R_NUM_OLD] = num_old;
        cur[R_NITER] = niter;
        cur[R_STALE] = stale;
        cur[R_XBUF] = xbuf;
    }
    if (!active) return;

    const int m = blockIdx.x * kTile + threadIdx.x;
    const long at = (long)blockIdx.y * ws.Mp + m;
    double dot[1] = {0.0};
    if (m < ws.M) {
        const double qv = -ws.g[at];
        ws.q[at] = qv;
        if (num_old > 0) dot[0] = ws.S[(long)head * ws.vec + at] * qv;
    }
    if (num_old == 0) return;
    block_reduce<1>(dot, 0, s_red);
    if (threadIdx.x == 0) *partial(ws, 0, 0) = dot[0];
}

// ---------------------------------------------------------------------------------------------------------------- recursion
// grid (tiles, 3).  One stage of the two-loop recursion (:432-442): the axpy that the previous stage's dot allows, fused with the
// next dot.  Pair i is the i-th newest; the first loop runs from the newest to the oldest, the second back.
__global__ void __launch_bounds__(kThreads) pass3_recursion_kernel(Ws ws, int j, int stage) {
    __shared__ double s_red[kWaves][kQuantities];
    double *cur = ws.rec + (long)j * kRecDoubles;
    if (cur[R_ACTIVE] == 0.0) return;
    const int num_old = (int)cur[R_NUM_OLD], head = (int)cur[R_HEAD];
    const int m = blockIdx.x * kTile + threadIdx.x;
    const long at = (long)blockIdx.y * ws.Mp + m;
    const bool in = m < ws.M;
    double dot[1];
    double out[1] = {0.0};

    if (stage < kMidLaunch) {                                               // first loop, stage 1 .. 9
        if (stage >= num_old) return;
        const int i = stage - 1;
        finish<1>(ws, stage - 1, 0, dot, s_red);
        const double al = dot[0] * ws.ro[ring_slot(head, i)];
        if (is_writer()) cur[R_AL + i] = al;
        if (in) {
            const double qv = ws.q[at] - al * ws.Y[(long)ring_slot(head, i) * ws.vec + at];
            ws.q[at] = qv;
            out[0] = ws.S[(long)ring_slot(head, stage) * ws.vec + at] * qv;
        }
    } else if (stage == kMidLaunch) {                                       // the oldest pair, r = q * H_diag
        const double hdiag = cur[R_HDIAG];
        if (num_old == 0) {
            if (in) ws.q[at] = ws.q[at] * hdiag;
            return;
        }
        const int i = num_old - 1;
        finish<1>(ws, i, 0, dot, s_red);
        const double al = dot[0] * ws.ro[ring_slot(head, i)];
        if (is_writer()) cur[R_AL + i] = al;
        if (in) {
            const double yv = ws.Y[(long)ring_slot(head, i) * ws.vec + at];
            const double r = (ws.q[at] - al * yv) * hdiag;
            ws.q[at] = r;
            out[0] = yv * r;
        }
    } else if (stage < kGtdLaunch) {                                        // second loop, stage 11 .. 19
        const int c = stage - kMidLaunch;
        if (c >= num_old) return;
        const int i_prev = num_old - c, i = i_prev - 1;
        finish<1>(ws, stage - 1, 0, dot, s_red);
        const double be = dot[0] * ws.ro[ring_slot(head, i_prev)];
        const double coef = cur[R_AL + i_prev] - be;
        if (in) {
            const double r = ws.q[at] + coef * ws.S[(long)ring_slot(head, i_prev) * ws.vec + at];
            ws.q[at] = r;
            out[0] = ws.Y[(long)ring_slot(head, i) * ws.vec + at] * r;
        }
    } else {                                                                // the newest pair: r is d; g . d
        double r = in ? ws.q[at] : 0.0;
        if (num_old > 0) {
            finish<1>(ws, kMidLaunch + num_old - 1, 0, dot, s_red);
            const double be = dot[0] * ws.ro[ring_slot(head, 0)];
            const double coef = cur[R_AL] - be;
            if (in) {
                r = r + coef * ws.S[(long)ring_slot(head, 0) * ws.vec + at];
                ws.q[at] = r;
            }
        }
        if (in) out[0] = ws.g[at] * r;
    }
    block_reduce<1>(out, 0, s_red);
    if (threadIdx.x == 0) *partial(ws, stage, 0) = out[0];
}

// ---------------------------------------------------------------------------------------------------------------- move
// grid (tiles, 3).  j < 0: the first evaluation, at x = the padded target (:299-306).  Otherwise the gtd exit (:460-464), x += t d
// (:492) in two doubles into the other x buffer, loss and gradient at the new x, and y, s of the next memory update.
__global__ void __launch_bounds__(kThreads)
pass3_move_kernel(Ws ws, int j, EvalConsts ec, const double *__restrict__ paths, const float *__restrict__ weight, int N,
                  double *__restrict__ trace) {
    __shared__ double s_red[kWaves][kQuantities];
    __shared__ double s_x[kTile + 2 * kHalo], s_xl[kTile + 2 * kHalo];
    __shared__ double s_w[kTile + kHalo];
    const int tid = threadIdx.x, a = blockIdx.y, m0 = blockIdx.x * kTile, m = m0 + tid;
    const long base = (long)a * ws.Mp, at = base + m;
    const bool init = j < 0, in = m < ws.M;
    double t = 0.0;
    int cand = 0, xbuf = 0;
    double *trace_row = trace && !init ? trace + ((long)j * 3 + a) * ws.M : nullptr;
    if (!init) {
        double *cur = ws.rec + (long)j * kRecDoubles;
        xbuf = (int)cur[R_XBUF];
        bool moves = cur[R_ACTIVE] != 0.0;
        if (moves) {
            double gtd[1];
            finish<1>(ws, kGtdLaunch, 0, gtd, s_red);
            moves = !(gtd[0] > -kTolChange);
            if (is_writer()) {
                cur[R_GTD] = gtd[0];
                if (!moves) cur[R_EXIT_GTD] = 2.0;
            }
        }
        if (!moves) {
            if (trace_row && in) trace_row[m] = ws.x[(long)xbuf * ws.vec + at];
            return;
        }
        t = cur[R_T];
        cand = ((int)cur[R_HEAD] + 1) % kRing;
    }
    const double *x_old = ws.x + (long)xbuf * ws.vec, *x_old_lo = x_old + 2 * ws.vec;
    double *x_new = ws.x + (long)(init ? 0 : 1 - xbuf) * ws.vec, *x_new_lo = x_new + 2 * ws.vec;

    for (int l = tid; l < kTile + 2 * kHalo; l += kThreads) {
        const int gm = m0 - kHalo + l;
        dd xv = {0.0, 0.0};
        if (gm >= 0 && gm < ws.M) {
            if (init) {
                const double p = paths[(long)a * N + (gm < N ? gm : N - 1)];
                xv.h = a < 2 ? p * ec.rw : p;
            } else {
                const dd xo = {x_old[base + gm], x_old_lo[base + gm]};
                xv = dd_axpy(xo, t, ws.q[base + gm]);
            }
        }
        s_x[l] = xv.h;
        s_xl[l] = xv.l;
        if (l < kTile + kHalo) {
            double wv = 0.0;
            if (gm >= 0 && gm < ws.M) wv = init ? (gm < N ? (double)weight[gm] : 0.0) : ws.w[gm];
            s_w[l] = wv;
        }
    }
    __syncthreads();

    double part[kQuantities] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (in) {
        // differences D^k at i = m - 3 + jj; D^k_i exists for 0 <= i < M - k and is weighted by w_i
        // in two doubles down to the third difference; its high word is what the weights multiply
        dd xv[7], e1[6], e2[5], e3[4];
        double d1[4], d2[4], d3[4];
#pragma unroll
        for (int jj = 0; jj < 7; ++jj) xv[jj] = dd{s_x[tid + jj], s_xl[tid + jj]};
#pragma unroll
        for (int jj = 0; jj < 6; ++jj) e1[jj] = dd_sub(xv[jj + 1], xv[jj]);
#pragma unroll
        for (int jj = 0; jj < 5; ++jj) e2[jj] = dd_sub(e1[jj + 1], e1[jj]);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) e3[jj] = dd_sub(e2[jj + 1], e2[jj]);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            d1[jj] = e1[jj].h;
            d2[jj] = e2[jj].h;
            d3[jj] = e3[jj].h;
        }
        double a1[4], a2[4], a3[4];                                        // c_k w_i D^k_i at i = m - 3 .. m, zero outside
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int i = m - 3 + jj;
            const double wv = s_w[tid + jj];
            a1[jj] = i >= 0 && i < ws.M - 1 ? ec.c[0] * wv * d1[jj] : 0.0;
            a2[jj] = i >= 0 && i < ws.M - 2 ? ec.c[1] * wv * d2[jj] : 0.0;
            a3[jj] = i >= 0 && i < ws.M - 3 ? ec.c[2] * wv * d3[jj] : 0.0;
        }
        // the adjoint of a difference is a'_p = a_{p-1} - a_p, applied k times
        const double g1 = a1[2] - a1[3];
        const double g2 = (a2[1] - a2[2]) - (a2[2] - a2[3]);
        const double g3 = ((a3[0] - a3[1]) - (a3[1] - a3[2])) - ((a3[1] - a3[2]) - (a3[2] - a3[3]));
        const double xm = xv[3].h;
        const double tv = init ? xm : ws.t[at];
        const double res = dd_sub(xv[3], dd{tv, 0.0}).h;
        const double gv = ((g1 + g2) + g3) + ec.cp * res;
        const double wm = s_w[tid + 3];
        double lossv = ec.hp * (res * res);
        if (m < ws.M - 1) lossv += ec.h[0] * (wm * (d1[3] * d1[3]));
        if (m < ws.M - 2) lossv += ec.h[1] * (wm * (d2[3] * d2[3]));
        if (m < ws.M - 3) lossv += ec.h[2] * (wm * (d3[3] * d3[3]));
        part[Q_LOSS] = lossv;
        part[Q_MAXG] = part[Q_SUMABS] = fabs(gv);
        x_new[at] = xm;
        x_new_lo[at] = xv[3].l;
        if (init) {
            ws.t[at] = xm;
            if (a == 0) ws.w[m] = wm;
        } else {
            const double sv = ws.q[at] * t, yv = gv - ws.g[at];            // s = d.mul(t), y = flat_grad.sub(prev_flat_grad)
            ws.S[(long)cand * ws.vec + at] = sv;
            ws.Y[(long)cand * ws.vec + at] = yv;
            part[Q_MAXDT] = fabs(sv);
            part[Q_YS] = yv * sv;
            part[Q_YY] = yv * yv;
            if (trace_row) trace_row[m] = xm;
        }
        ws.g[at] = gv;
    }
    block_reduce<kQuantities>(part, kMoveMax, s_red);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < kQuantities; ++k) *partial(ws, kMoveLaunch, k) = part[k];
    }
}

// grid (tiles, 3): the fixes (:330-332) from the x buffer the last record names.
__global__ void __launch_bounds__(kThreads)
pass3_output_kernel(Ws ws, int last, double rw, int N, double *__restrict__ out) {
    const double *rec = ws.rec + (long)last * kRecDoubles;
    const bool moved = rec[R_ACTIVE] != 0.0 && rec[R_EXIT_GTD] == 0.0;
    const int xbuf = moved ? 1 - (int)rec[R_XBUF] : (int)rec[R_XBUF];
    const int m = blockIdx.x * kTile + threadIdx.x, a = blockIdx.y;
    if (m >= N) return;
    const long at = (long)a * ws.Mp + m;
    const dd x = {ws.x[(long)xbuf * ws.vec + at], ws.x[(long)(2 + xbuf) * ws.vec + at]};
    const double fix = dd_sub(x, dd{ws.t[at], 0.0}).h;
    out[(long)a * N + m] = a < 2 ? fix / rw : fix;
}

// ------------------------------------------------------------------------------------------------ weights, paths, filters
// calc_scene_weight (:86-105), fp32, every operation exactly rounded
__global__ void __launch_bounds__(kThreads) pass3_scene_weight_kernel(const float *__restrict__ score, int N, float *__restrict__ weight) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    float w = (score[i] - 0.5f) / 0.25f;
    w = w != w ? w : fminf(fmaxf(w, 0.f), 1.f);
    if (w < 0.65f) w = w * w;
    if (i == 0 || i == N - 1) w = 0.f;
    weight[i] = w;
}

__device__ __forceinline__ double path_value(const double *__restrict__ sx, const double *__restrict__ sy, const double *__restrict__ an,
                                             const float *__restrict__ weight, int a, int i) {
    double v = a == 0 ? sx[i] : (a == 1 ? sy[i] : an[i]);
    if (a == 2 && v == v) v = fmin(fmax(v, -90.0), 90.0);                   // ANGLE_MAX_HARD :359
    return v * (double)weight[i];
}

// grid (tiles of N, 3).  pass 0: the tile's sum into sums[a * tiles + tile].  pass 1: the sums of the tiles before it in index
// order, then the running sum through the tile.
__global__ void __launch_bounds__(kThreads)
pass3_prefix_kernel(const double *__restrict__ sx, const double *__restrict__ sy, const double *__restrict__ an,
                    const float *__restrict__ weight, int N, int pass, double *__restrict__ sums, double *__restrict__ paths) {
    __shared__ double s_red[kWaves][kQuantities];
    __shared__ double s_scan[kTile];
    const int tid = threadIdx.x, a = blockIdx.y, i = blockIdx.x * kTile + tid;
    const double v = i < N ? path_value(sx, sy, an, weight, a, i) : 0.0;
    if (pass == 0) {
        double s[1] = {v};
        block_reduce<1>(s, 0, s_red);
        if (tid == 0) sums[a * gridDim.x + blockIdx.x] = s[0];
        return;
    }
    double before[1] = {0.0};
    for (int p = tid; p < (int)blockIdx.x; p += kThreads) before[0] += sums[a * gridDim.x + p];
    block_reduce<1>(before, 0, s_red);
    // inside the tile in index order, as the reference's cumsum adds: the first tile is bit-equal to it
    s_scan[tid] = v;
    __syncthreads();
    if (tid == 0) {
        double run = before[0];
        for (int l = 0; l < kTile; ++l) {
            run = blockIdx.x == 0 && l == 0 ? s_scan[0] : run + s_scan[l];
            s_scan[l] = run;
        }
    }
    __syncthreads();
    if (i < N) paths[(long)a * N + i] = s_scan[tid];
}

// grid (tiles of N, 3): replicate pad, K-tap correlation, minus the input (:78-83, :281-287)
__global__ void __launch_bounds__(kThreads)
pass3_conv_kernel(const double *__restrict__ paths, int N, const double *__restrict__ taps, int K, double *__restrict__ fix) {
    __shared__ double s_win[kTile + kMaxTaps - 1];
    const int tid = threadIdx.x, a = blockIdx.y, i0 = blockIdx.x * kTile, pad = (K - 1) / 2;
    const double *row = paths + (long)a * N;
    for (int l = tid; l < kTile + K - 1; l += kThreads) {
        int src = i0 - pad + l;
        src = src < 0 ? 0 : (src > N - 1 ? N - 1 : src);
        s_win[l] = row[src];
    }
    __syncthreads();
    const int i = i0 + tid;
    if (i >= N) return;
    // a compensated sum (TwoSum of every product into acc, the rounding errors gathered in comp): at K = 4097 a plain running sum
    // carries several times the error of a pairwise one
    double acc = 0.0, comp = 0.0;
    for (int k = 0; k < K; ++k) {
        const double p = taps[k] * s_win[tid + k];
        const double t = acc + p, bb = t - acc;
        comp += (acc - (t - bb)) + (p - bb);
        acc = t;
    }
    fix[(long)a * N + i] = (acc + comp) - s_win[tid + pad];
}

inline bool aligned(const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

inline Ws bind(void *workspace, const Layout &l) {
    char *b = static_cast<char *>(workspace);
    Ws ws;
    ws.rec = reinterpret_cast<double *>(b + l.rec);
    ws.ro = reinterpret_cast<double *>(b + l.ro);
    ws.x = reinterpret_cast<double *>(b + l.x);
    ws.t = reinterpret_cast<double *>(b + l.t);
    ws.w = reinterpret_cast<double *>(b + l.w);
    ws.g = reinterpret_cast<double *>(b + l.g);
    ws.q = reinterpret_cast<double *>(b + l.q);
    ws.S = reinterpret_cast<double *>(b + l.S);
    ws.Y = reinterpret_cast<double *>(b + l.Y);
    ws.partials = reinterpret_cast<double *>(b + l.partials);
    ws.M = (int)l.M;
    ws.Mp = (int)l.Mp;
    ws.nparts = (int)l.nparts;
    ws.vec = 3 * l.Mp;
    return ws;
}

}  // namespace
}  // namespace nunif

using namespace nunif;

extern "C" int nunif_hip_stlizer_scene_weight(const float *scores, int32_t N, float *weight, void *stream) {
    NUNIF_REQUIRE(N >= 1 && N <= kMaxN, "stlizer_scene_weight: N=%d is outside 1 <= N <= %d", N, kMaxN);
    NUNIF_REQUIRE(scores && weight, "stlizer_scene_weight: NULL argument");
    pass3_scene_weight_kernel<<<(N + kThreads - 1) / kThreads, kThreads, 0, static_cast<hipStream_t>(stream)>>>(scores, N, weight);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int64_t nunif_hip_stlizer_pass3_workspace_bytes(int32_t N, int32_t iteration) {
    if (!shape_ok(N, iteration)) return -1;
    return layout(N, iteration).total;
}

extern "C" int nunif_hip_stlizer_pass3_prepare(const double *shift_x, const double *shift_y, const double *angle, const float *weight,
                                               int32_t N, double *paths, void *workspace, int64_t workspace_bytes, void *stream) {
    NUNIF_REQUIRE(N >= 1 && N <= kMaxN, "stlizer_pass3_prepare: N=%d is outside 1 <= N <= %d", N, kMaxN);
    NUNIF_REQUIRE(shift_x && shift_y && angle && weight && paths && workspace, "stlizer_pass3_prepare: NULL argument");
    const Layout l = layout(N, 1);
    NUNIF_REQUIRE(aligned(workspace, 256) && workspace_bytes >= l.total,
                  "stlizer_pass3_prepare: workspace of %lld bytes (need %lld, 256-byte aligned)", (long long)workspace_bytes, (long long)l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *sums = bind(workspace, l).partials;                              // 3 * ceil(N / 256) <= nparts doubles
    const dim3 grid((N + kTile - 1) / kTile, 3);
    for (int pass = 0; pass < 2; ++pass) {
        pass3_prefix_kernel<<<grid, kThreads, 0, s>>>(shift_x, shift_y, angle, weight, N, pass, sums, paths);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_stlizer_pass3_conv(const double *paths, int32_t N, const double *taps, int32_t K, double *fix, void *stream) {
    NUNIF_REQUIRE(N >= 1 && N <= kMaxN, "stlizer_pass3_conv: N=%d is outside 1 <= N <= %d", N, kMaxN);
    NUNIF_REQUIRE(K >= 1 && K <= kMaxTaps && (K & 1), "stlizer_pass3_conv: K=%d taps (odd, 1 <= K <= %d)", K, kMaxTaps);
    NUNIF_REQUIRE(paths && taps && fix && paths != fix, "stlizer_pass3_conv: NULL argument or fix aliases paths");
    const dim3 grid((N + kTile - 1) / kTile, 3);
    pass3_conv_kernel<<<grid, kThreads, 0, static_cast<hipStream_t>(stream)>>>(paths, N, taps, K, fix);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_stlizer_pass3_grad_opt(const double *paths, const float *weight, int32_t N, double resolution_weight,
                                                int32_t iteration, double penalty_weight, double *out, void *workspace,
                                                int64_t workspace_bytes, double *trace_or_null, double *log_or_null, void *stream) {
    NUNIF_REQUIRE(shape_ok(N, iteration), "stlizer_pass3_grad_opt: bad shape N=%d iteration=%d (1 <= N <= %d, 1 <= iteration <= %d)",
                  N, iteration, kMaxN, kMaxIteration);
    NUNIF_REQUIRE(paths && weight && out && workspace, "stlizer_pass3_grad_opt: NULL argument");
    NUNIF_REQUIRE(resolution_weight > 0.0 && penalty_weight == penalty_weight, "stlizer_pass3_grad_opt: resolution weight %g, penalty weight %g",
                  resolution_weight, penalty_weight);
    const Layout l = layout(N, iteration);
    NUNIF_REQUIRE(aligned(workspace, 256) && workspace_bytes >= l.total,
                  "stlizer_pass3_grad_opt: workspace of %lld bytes (need %lld, 256-byte aligned)", (long long)workspace_bytes, (long long)l.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Ws ws = bind(workspace, l);
    EvalConsts ec;
    const double gw = 1.0 / 9.0, M = (double)l.M;
    for (int k = 0; k < 3; ++k) {
        ec.c[k] = 2.0 * gw / (M - (k + 1));
        ec.h[k] = gw / (M - (k + 1));
    }
    ec.cp = 2.0 * penalty_weight / M;
    ec.hp = penalty_weight / M;
    ec.rw = resolution_weight;
    const dim3 grid((unsigned)l.tiles, 3);
    const int slots = iteration * kMaxIter;
    ProfScope prof("stlizer_pass3_grad_opt", s, 0.0, (double)l.vec_bytes * 4.0 * kLaunchesPerSlot * slots);
    pass3_move_kernel<<<grid, kThreads, 0, s>>>(ws, -1, ec, paths, weight, N, nullptr);
    NUNIF_LAUNCH_CHECK();
    for (int j = 0; j < slots; ++j) {
        pass3_begin_kernel<<<grid, kThreads, 0, s>>>(ws, j);
        for (int stage = 1; stage <= kGtdLaunch; ++stage) pass3_recursion_kernel<<<grid, kThreads, 0, s>>>(ws, j, stage);
        pass3_move_kernel<<<grid, kThreads, 0, s>>>(ws, j, ec, paths, weight, N, trace_or_null);
        NUNIF_LAUNCH_CHECK();
    }
    pass3_output_kernel<<<grid, kThreads, 0, s>>>(ws, slots - 1, resolution_weight, N, out);
    NUNIF_LAUNCH_CHECK();
    if (log_or_null)
        NUNIF_HIP_CHECK(hipMemcpyAsync(log_or_null, ws.rec, (size_t)slots * kRecDoubles * 8, hipMemcpyDeviceToDevice, s));
    return NUNIF_HIP_OK;
}
