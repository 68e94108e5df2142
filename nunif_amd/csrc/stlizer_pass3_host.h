// stlizer pass 3, host-only: the limits, the launch schedule and the workspace layout of grad_opt (stlizer_pass3.hip).  No device
// code and no HIP header, so that tests/cpp/stlizer_pass3_host_check.cpp can walk it under the host sanitizers.
//
// One LBFGS iteration slot is kLaunchesPerSlot launches, the same for every slot whatever the data:
//   launch 0          begin: finishes the evaluation's partials, takes every decision of the slot (the exits of the previous
//                     iteration, the step entry, the memory update), writes the slot's record, q = -g, dot s[0].q
//   launch 1 .. 9     first loop stage m: al[m-1], q -= al[m-1] y[m-1], dot s[m].q            (returns at once if m >= num_old)
//   launch 10         al[last], q -= al[last] y[last], r = q * H_diag, dot y[last].r
//   launch 11 .. 19   second loop stage c: be, r += s (al - be) of the c-th oldest, dot of the next  (returns if c >= num_old)
//   launch 20         be and r += s[0] (al[0] - be) of the newest pair: r is d; dot g.d
//   launch 21         move: decides gtd, x += t d, evaluates loss and gradient at the new x, writes y and s of the next memory
//                     update into the free ring slot, and the partials of loss, max|g|, sum|g|, max|d t|, y.s, y.y
// Every launch writes its per-workgroup partials into a buffer of its own (index = launch number), so no launch reads a buffer
// that the same launch writes; its consumer finishes them in index order.
#pragma once

#include <cstdint>

namespace nunif {
namespace pass3 {

constexpr int kTile = 256;                    // elements per workgroup, one per thread
constexpr int kHalo = 3;                      // the third difference reaches three elements to either side
constexpr int kHistory = 10;                  // torch.optim.LBFGS(history_size=10)
constexpr int kRing = kHistory + 1;           // one free slot for the candidate pair of the next memory update
constexpr int kMaxIter = 4;                   // LBFGS(max_iter=4): iterations per optimizer.step
constexpr int kMaxN = 1 << 20;
constexpr int kMaxIteration = 1024;
constexpr int kMaxTaps = 4097;
constexpr int kLaunchesPerSlot = 22;
constexpr int kQuantities = 6;                // partials per workgroup and buffer (the move launch uses all six)
constexpr int kRecDoubles = 32;               // one decision record per slot

// fields of a record (all doubles; integers are stored exactly)
enum Rec {
    R_ACTIVE = 0,      // the iteration of this slot runs
    R_EXIT_BEGIN,      // 0, 1 (opt_cond at step entry) or 6 (the step had ended)
    R_EXIT_GTD,        // 0 or 2, by the move launch
    R_EXIT_AFTER,      // 0, 3, 4 or 5, by the begin launch of the next slot
    R_ACCEPTED,        // -1 no memory update, 0 rejected, 1 taken
    R_LOSS, R_MAXG, R_GTD, R_YS, R_MAXG_NEW, R_MAXDT, R_DLOSS,
    R_T, R_HDIAG, R_HEAD, R_NUM_OLD, R_NITER, R_STALE, R_XBUF,      // the optimizer's state after the slot's decisions
    R_AL,              // al[0 .. 9], index 0 the newest pair
    R_END = R_AL + kHistory
};
static_assert(R_END <= kRecDoubles, "record");

struct Layout {
    int64_t M, tiles, Mp, nparts;              // padded length N + 3, workgroups per axis, M rounded up to tiles, 3 * tiles
    int64_t rec, ro, x, t, w, g, q, S, Y, partials, total;      // byte offsets; x holds four vectors: the high words of two buffers (a move reads one, writes the other), then their low words
    int64_t vec_bytes;                         // one [3][Mp] vector
};

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

inline bool shape_ok(int64_t N, int64_t iteration) {
    return N >= 1 && N <= kMaxN && iteration >= 1 && iteration <= kMaxIteration;
}

inline Layout layout(int64_t N, int64_t iteration) {
    Layout l;
    l.M = N + kHalo;
    l.tiles = (l.M + kTile - 1) / kTile;
    l.Mp = l.tiles * kTile;
    l.nparts = 3 * l.tiles;
    l.vec_bytes = 3 * l.Mp * 8;
    int64_t at = 0;
    l.rec = at;       at += align256(iteration * kMaxIter * kRecDoubles * 8);
    l.ro = at;        at += align256(kRing * 8);
    l.x = at;         at += 4 * l.vec_bytes;
    l.t = at;         at += l.vec_bytes;
    l.w = at;         at += l.Mp * 8;
    l.g = at;         at += l.vec_bytes;
    l.q = at;         at += l.vec_bytes;
    l.S = at;         at += kRing * l.vec_bytes;
    l.Y = at;         at += kRing * l.vec_bytes;
    l.partials = at;  at += align256((int64_t)kLaunchesPerSlot * kQuantities * l.nparts * 8);
    l.total = at;
    return l;
}

// torch.optim.LBFGS's tolerances (tolerance_grad, tolerance_change) and the curvature test of its memory update
constexpr double kTolGrad = 1e-7, kTolChange = 1e-9, kYsMin = 1e-10;

// The exits after an iteration's re-evaluation, in torch's order (lbfgs.py:517-526): opt_cond, then the step, then the loss.
// 0: none.  A NaN passes every test, as in torch.
constexpr int exit_after_code(double maxg_new, double maxdt, double dloss) {
    return maxg_new <= kTolGrad ? 3 : (maxdt <= kTolChange ? 4 : (dloss < kTolChange ? 5 : 0));
}

// the ring slot of the i-th newest pair (i = 0 the newest), head the newest's slot
constexpr int ring_slot(int head, int i) { return (head - i + kRing) % kRing; }

// byte offset of one partial: launch's buffer, quantity, workgroup
inline int64_t partial_offset(const Layout &l, int launch, int quantity, int64_t part) {
    return l.partials + (((int64_t)launch * kQuantities + quantity) * l.nparts + part) * 8;
}

}  // namespace pass3
}  // namespace nunif
