"""stlizer pass 3 restated in numpy (tests only): ``calc_scene_weight``, the path preparation, the smoothing filters and
``grad_opt`` of the reference's ``stlizer/multipass_pipeline.py:86-105, :272-366``, with ``torch.optim.LBFGS.step`` (history 10,
max_iter 4, lr 1, no line search) written out decision for decision.  Everything runs in the dtype it is given, ``numpy.float64``
or ``numpy.longdouble``: the longdouble run is the yardstick against which both the reference's recorded float64 and the engine's
float64 are measured.

The objective is quadratic and its three axes are independent.  For one axis with padded target ``t`` and padded weights ``w``,
M = N + 3:  f(x) = (1/9) * sum_k mean(w[:M-k] * (D^k x)^2, k = 1..3) + pw * mean((x - t)^2).  ``loss_grad`` is the closed form of
its gradient (a 7-point stencil), ``exact_minimiser`` solves the heptadiagonal system.

The decision log has one record per LBFGS iteration slot (``iteration * 4`` of them), the same fields the kernel writes:

``exit``      0 the iteration ran to its end; 1 ``opt_cond`` at step entry; 2 ``gtd > -1e-9``; 3 ``opt_cond`` after the
              re-evaluation; 4 ``max|d*t| <= 1e-9``; 5 ``|loss - prev_loss| < 1e-9``; 6 the step had ended before this slot
``accepted``  1 / 0 the memory update ``ys > 1e-10`` was taken / rejected; -1 there was none (first iteration, or exit 1 / 6)
``loss maxg`` the loss and max|g| the iteration started from;  ``gtd`` g.d;  ``ys`` y.s
``maxg_new maxdt dloss``  what exits 3, 4, 5 test (only where the iteration moved and was not the 4th of its step)
"""
import numpy as np

DEFAULT_RESOLUTION = 320
ANGLE_MAX_HARD = 90.0
HISTORY, MAX_ITER = 10, 4
TOL_GRAD, TOL_CHANGE, YS_MIN = 1e-7, 1e-9, 1e-10
LOG_FIELDS = ("exit", "accepted", "loss", "maxg", "gtd", "ys", "maxg_new", "maxdt", "dloss")

MUTATIONS = ("w_right", "mean_M", "ring_off", "no_hdiag", "reeval4", "prev_grad_reset", "res_angle")


# ---------------------------------------------------------------------------------------------------------------- inputs
def jitter_path(seed, n, amplitude=1.0):
    """Per-frame shifts and angles of a hand-held camera: a slow drift plus white jitter."""
    g = np.random.default_rng(seed)
    k = np.arange(n)
    out = []
    for a, f in ((3.0, 0.013), (2.0, 0.021), (0.4, 0.017)):
        out.append(amplitude * (a * 0.2 * np.sin(2 * np.pi * f * k + g.uniform(0, 6)) + a * g.standard_normal(n)))
    return [v.astype(np.float64) for v in out]


def match_scores(seed, n, cuts=()):
    """Mean match scores as pass 1 leaves them: about 0.8, a few frames in the doubtful band, a scene cut well below 0.5."""
    g = np.random.default_rng(seed + 1000)
    s = 0.8 + 0.05 * g.standard_normal(n)
    doubtful = g.random(n) < 0.1
    s[doubtful] = g.uniform(0.5, 0.7, int(doubtful.sum()))
    for c in cuts:
        if 0 <= c < n:
            s[c] = 0.2
    return s.astype(np.float32)


# name -> (N, cuts, resolution, fps, amplitude, seed[, penalty weight; pass 3's own 2e-3 / seconds where absent])
CASES = {
    "n1": (1, (), 320, 30, 1.0, 1), "n2": (2, (), 320, 30, 1.0, 2), "n3": (3, (1,), 320, 30, 1.0, 3),
    "n4": (4, (), 480, 23.976, 1.0, 4), "n5": (5, (1,), 320, 60, 1.0, 5), "n37": (37, (1, 35), 320, 30, 1.0, 6),
    "n255": (255, (128,), 480, 23.976, 1.0, 7), "n256": (256, (253,), 320, 60, 1.0, 8), "n257": (257, (255, 256), 320, 30, 1.0, 9),
    "n300": (300, (150,), 320, 30, 1.0, 14),
    "n1025": (1025, (1, 512, 1023), 480, 30, 1.0, 10), "n5000": (5000, (2560, 4998), 320, 60, 1.0, 11),
    "tiny": (37, (20,), 320, 30, 1e-3, 12), "zero": (37, (20,), 320, 30, 0.0, 13),
    # the exits of torch's LBFGS that ordinary paths do not reach within three steps
    # exit 2 with a rejected memory update, exit 1 just below the gradient tolerance, exit 5; exits 3 and 4 need a stiff penalty
    # (with pass 3's own weight the step is never small while g.d is not): grad_opt takes the weight as an argument
    "micro": (37, (20,), 320, 30, 3e-6, 15), "nano": (37, (20,), 320, 30, 2e-8, 16),
    "exit5": (37, (18,), 320, 30, 10.0 ** -3.375, 151), "exit3": (37, (20,), 320, 30, 1e-2, 15, 1e8),
    # exit 4 needs |g|_1 >= 1 with max|d| <= 1e-9: only a gradient that is rounding noise times a stiff penalty gets there.
    # Here it is the rounding of a float64 x; the engine holds x in two doubles and, like the longdouble run, leaves by exit 2.
    "exit4": (37, (20,), 320, 30, 1e5, 15, 1e13),
}
EXIT_CASES = {"zero": 1, "nano": 1, "micro": 2, "exit3": 3, "exit4": 4, "exit5": 5}              # float64 throughout
ENGINE_EXIT_CASES = {"zero": 1, "nano": 1, "micro": 2, "exit3": 3, "exit4": 2, "exit5": 5}      # x held wider (wide_x)
ITER3_CASES = tuple(CASES)
CONVERGED_CASES = ("n37", "n300", "n1025")
SMOOTHING_SECONDS = 2.0


LONG_N = 70000


def long_case():
    """A path too long for a fixture, generated where it is used: more than 256 tiles per axis, so that the finishing of the
    per-workgroup partials and the tile offsets of the prefix sums both take more than one trip per thread.  Cuts at a tile edge
    and at N - 2.  -> shift_x, shift_y, angle, scores, resolution, fps."""
    sx, sy, an = jitter_path(70, LONG_N)
    return sx, sy, an, match_scores(70, LONG_N, (25600, LONG_N - 2)), 320, 30


def case_input(name):
    """-> shift_x, shift_y, angle [N] float64 (per-frame, before the weights and the prefix sum), scores [N] float32, resolution, fps."""
    n, cuts, resolution, fps, amplitude, seed = CASES[name][:6]
    sx, sy, an = jitter_path(seed, n, amplitude)
    if name == "n257":
        an[5] = 123.0                     # past the hard angle limit
        an[6] = -95.0
    return sx, sy, an, match_scores(seed, n, cuts), resolution, fps


# ------------------------------------------------------------------------------------------------ weights, paths, filters
def calc_scene_weight(scores):
    """:86-105 in fp32, every operation one rounding."""
    s = np.asarray(scores, dtype=np.float32)
    w = np.clip((s - np.float32(0.5)) / np.float32(0.25), np.float32(0), np.float32(1)).astype(np.float32)
    low = w < np.float32(0.65)
    w[low] = w[low] * w[low]
    w[0] = 0
    w[-1] = 0
    return w


def prepare(shift_x, shift_y, angle, weight, dtype=np.float64):
    """:359 and :338-344: clamp the angle, times the fp32 weight, inclusive prefix sums -> [3, N]."""
    w = np.asarray(weight, dtype=np.float32).astype(dtype)
    rows = [np.asarray(shift_x, dtype=dtype), np.asarray(shift_y, dtype=dtype),
            np.clip(np.asarray(angle, dtype=dtype), dtype(-ANGLE_MAX_HARD), dtype(ANGLE_MAX_HARD))]
    return np.stack([np.cumsum(r * w, dtype=dtype) for r in rows])


def kernel_size(seconds, fps):
    k = int(seconds * float(fps))
    return k + 1 if k % 2 == 0 else k


def gaussian_taps(k, dtype=np.float64):
    """``get_gaussian_kernel1d`` in its own expressions."""
    if k == 1:
        return np.ones(1, dtype=dtype)
    sigma = k * 0.15 + 0.35
    half = (k - 1) * 0.5
    x = np.linspace(-half, half, k, dtype=dtype)
    g = np.exp(dtype(-0.5) * (x / dtype(sigma)) ** 2)
    return g / g.sum(dtype=dtype)


def conv_fix(paths, taps, dtype=np.float64):
    """:78-83 and :285-287: replicate pad, correlate, minus the input.  paths [3, N] -> [3, N]."""
    paths = np.asarray(paths, dtype=dtype)
    taps = np.asarray(taps, dtype=dtype)
    k = taps.shape[0]
    pad = (k - 1) // 2
    out = np.empty_like(paths)
    for a in range(paths.shape[0]):
        p = np.concatenate([np.repeat(paths[a, :1], pad), paths[a], np.repeat(paths[a, -1:], pad)])
        win = np.lib.stride_tricks.sliding_window_view(p, k)
        out[a] = (win * taps).sum(axis=1, dtype=dtype) - paths[a]
    return out


# ------------------------------------------------------------------------------------------------------------- objective
def pad_inputs(paths, weight, resolution, dtype=np.float64, mutation=None):
    """:297-302 -> target [3, M], weights [M], resolution_weight."""
    rw = resolution / DEFAULT_RESOLUTION
    paths = np.asarray(paths, dtype=dtype)
    t = np.concatenate([paths, np.repeat(paths[:, -1:], 3, axis=1)], axis=1)
    t[0] *= dtype(rw)
    t[1] *= dtype(rw)
    if mutation == "res_angle":
        t[2] *= dtype(rw)
    w = np.concatenate([np.asarray(weight, dtype=np.float32).astype(dtype), np.zeros(3, dtype=dtype)])
    return t, w, rw


def loss_grad(x, t, w, pw, mutation=None):
    """The loss of :311-322 and its gradient in closed form, in x's dtype.  x, t [3, M]; w [M]."""
    dtype = x.dtype.type
    M = x.shape[1]
    gw = dtype(1.0) / dtype(9.0)
    loss = dtype(0)
    g = np.zeros_like(x)
    for a in range(3):
        d = x[a]
        axis_loss = dtype(0)
        for k in (1, 2, 3):
            d = d[1:] - d[:-1]
            n = d.shape[0]                 # M - k
            if n <= 0:
                break
            wk = w[k:k + n] if mutation == "w_right" else w[:n]
            denom = dtype(M) if mutation == "mean_M" else dtype(n)
            axis_loss = axis_loss + (d * d * wk).sum(dtype=dtype) / denom
            a_k = (dtype(2.0) * gw / denom) * wk * d
            # the adjoint of the k-th difference
            for _ in range(k):
                a_k = np.concatenate([[dtype(0)], a_k]) - np.concatenate([a_k, [dtype(0)]])
            g[a] += a_k
        r = x[a] - t[a]
        loss = loss + axis_loss * gw + (r * r).sum(dtype=dtype) / dtype(M) * dtype(pw)
        g[a] += (dtype(2.0) * dtype(pw) / dtype(M)) * r
    return loss, g


def exact_minimiser(t, w, pw):
    """argmin of the objective, per axis, in float64 by a dense SPD solve refined once in longdouble.  t [3, M] -> [3, M]."""
    t = np.asarray(t, dtype=np.float64)
    M = t.shape[1]
    A = np.zeros((M, M))
    D = np.eye(M)
    for k in (1, 2, 3):
        D = D[1:] - D[:-1]
        n = D.shape[0]
        if n <= 0:
            break
        A += (D.T * (np.asarray(w[:n], dtype=np.float64) / (9.0 * n))) @ D
    A += np.eye(M) * (pw / M)
    b = t * (pw / M)
    try:
        from scipy.linalg import solveh_banded
        ab = np.zeros((4, M))
        for u in range(4):
            ab[3 - u, u:] = np.diagonal(A, u)
        solve = lambda rhs: solveh_banded(ab, rhs)                          # noqa: E731
    except ImportError:
        solve = lambda rhs: np.linalg.solve(A, rhs)                         # noqa: E731
    x = np.stack([solve(b[a]) for a in range(3)])
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(2):
        res = (bl - (Al @ x.astype(np.longdouble).T).T).astype(np.float64)
        x = x + np.stack([solve(res[a]) for a in range(3)])
    return x


def objective(x, t, w, pw):
    """f in longdouble (for the objective gap of the converged cases)."""
    return loss_grad(np.asarray(x, dtype=np.longdouble), np.asarray(t, dtype=np.longdouble), np.asarray(w, dtype=np.longdouble), pw)[0]


# ----------------------------------------------------------------------------------------------------------------- LBFGS
def _record(**kw):
    rec = {f: float("nan") for f in LOG_FIELDS}
    rec["exit"], rec["accepted"] = 0, -1
    rec.update(kw)
    return rec


def lbfgs(t, w, pw, iteration, mutation=None, wide_x=False):
    """``iteration`` calls of ``torch.optim.LBFGS(history_size=10, max_iter=4).step`` from x = t.  -> x, trace, log.
    ``wide_x``: x alone is held in longdouble and the closure's differences are taken from it before they are rounded, everything
    else stays in t's dtype: the shape of the engine, which holds x in two doubles."""
    dtype = t.dtype.type
    x = t.astype(np.longdouble) if wide_x else t.copy()

    def closure(xc, t, w, pw, mutation=None):
        if not wide_x:
            return loss_grad(xc, t, w, pw, mutation)
        loss, g = loss_grad(xc, t.astype(np.longdouble), w.astype(np.longdouble), pw, mutation)
        return dtype(loss), g.astype(dtype)
    flat = lambda v: v.reshape(-1)                                          # noqa: E731
    d = step_t = prev_g = None
    old_dirs, old_stps, ro = [], [], []
    H = dtype(1)
    al = [None] * HISTORY
    n_iter_total = 0
    trace, log = [], []
    for _ in range(iteration):
        loss, g = closure(x, t, w, pw, mutation)
        slot = 0
        if mutation == "prev_grad_reset":
            prev_g = None if prev_g is None else np.zeros_like(prev_g)
        if np.abs(g).max() <= TOL_GRAD:
            log.append(_record(exit=1, loss=loss, maxg=np.abs(g).max()))
            trace.append(x.astype(dtype))
            slot = 1
        else:
            while slot < MAX_ITER:
                slot += 1
                n_iter_total += 1
                rec = _record(loss=loss, maxg=np.abs(g).max())
                if n_iter_total == 1:
                    d = -g
                    H = dtype(1)
                else:
                    y = g - prev_g
                    s = d * step_t
                    ys = flat(y).dot(flat(s))
                    rec["ys"] = ys
                    rec["accepted"] = int(ys > YS_MIN)
                    if ys > YS_MIN:
                        if len(old_dirs) == HISTORY:
                            drop = 1 if mutation == "ring_off" else 0
                            old_dirs.pop(drop), old_stps.pop(drop), ro.pop(drop)
                        old_dirs.append(y), old_stps.append(s), ro.append(dtype(1) / ys)
                        if mutation != "no_hdiag":
                            H = ys / flat(y).dot(flat(y))
                    q = -g
                    num_old = len(old_dirs)
                    for i in range(num_old - 1, -1, -1):
                        al[i] = flat(old_stps[i]).dot(flat(q)) * ro[i]
                        q = q - al[i] * old_dirs[i]
                    d = q * H
                    for i in range(num_old):
                        be = flat(old_dirs[i]).dot(flat(d)) * ro[i]
                        d = d + (al[i] - be) * old_stps[i]
                prev_g = g.copy()
                prev_loss = loss
                step_t = min(dtype(1), dtype(1) / np.abs(g).sum(dtype=dtype)) if n_iter_total == 1 else dtype(1)
                gtd = flat(g).dot(flat(d))
                rec["gtd"] = gtd
                if gtd > -TOL_CHANGE:
                    rec["exit"] = 2
                    log.append(rec), trace.append(x.astype(dtype))
                    break
                x = x + step_t * d
                trace.append(x.astype(dtype))
                last = slot == MAX_ITER
                if not last or mutation == "reeval4":
                    loss, g = closure(x, t, w, pw, mutation)
                    rec["maxg_new"] = np.abs(g).max()
                    rec["maxdt"] = np.abs(d * step_t).max()
                    rec["dloss"] = abs(loss - prev_loss)
                    if rec["maxg_new"] <= TOL_GRAD:
                        rec["exit"] = 3
                    elif rec["maxdt"] <= TOL_CHANGE:
                        rec["exit"] = 4
                    elif rec["dloss"] < TOL_CHANGE:
                        rec["exit"] = 5
                log.append(rec)
                if last or rec["exit"]:
                    break
        while slot < MAX_ITER:
            slot += 1
            log.append(_record(exit=6))
            trace.append(x.astype(dtype))
    return x, np.stack(trace), log


def grad_opt(paths, weight, resolution, iteration=100, penalty_weight=1e-3, dtype=np.float64, mutation=None, wide_x=False):
    """:292-334 on prepared paths [3, N] -> fixes [3, N], trace [iteration * 4, 3, N + 3], log."""
    t, w, rw = pad_inputs(paths, weight, resolution, dtype, mutation)
    x, trace, log = lbfgs(t, w, penalty_weight, iteration, mutation, wide_x)
    out = (x - t)[:, :-3].astype(dtype)
    out[0] /= dtype(rw)
    out[1] /= dtype(rw)
    if mutation == "res_angle":
        out[2] /= dtype(rw)
    return out, trace, log


def penalty_weight(name=None, seconds=SMOOTHING_SECONDS):
    """The penalty weight of a case: ``pass3_smoothing``'s 2e-3 / seconds (:349) unless the case names its own."""
    if name is not None and len(CASES[name]) > 6:
        return CASES[name][6]
    return 2e-3 / seconds


def margins(log):
    """Per record, the factor by which every decision quantity it tested is away from its threshold (>= 1; inf if untested)."""
    out = []
    for rec in log:
        m = []
        if rec["exit"] in (1, 6):
            if rec["exit"] == 1:
                m.append(TOL_GRAD / max(rec["maxg"], 1e-300))
            out.append(min(m) if m else np.inf)
            continue
        m.append(rec["maxg"] / TOL_GRAD)
        if rec["accepted"] >= 0:
            ys = float(rec["ys"])
            m.append(ys / YS_MIN if ys > YS_MIN else (np.inf if ys <= 0 else YS_MIN / ys))
        gtd = float(rec["gtd"])
        m.append(-gtd / TOL_CHANGE if gtd <= -TOL_CHANGE else (np.inf if gtd >= 0 else TOL_CHANGE / -gtd))
        for key, tol, code in (("maxg_new", TOL_GRAD, 3), ("maxdt", TOL_CHANGE, 4), ("dloss", TOL_CHANGE, 5)):
            v = float(rec[key])
            if rec["exit"] == 2 or np.isnan(v):
                break
            m.append(tol / max(v, 1e-300) if rec["exit"] == code else v / tol)
            if rec["exit"] == code:
                break
        out.append(min(m))
    return out


def converged_measures(paths, weight, resolution, pw, runs, scales):
    """For each run (fixes [3, N] of the problem whose target is scaled by its scale): the max distance of its x to the exact
    minimiser and its objective gap f - f_exact.  -> list of (d, g)."""
    t, wp, rw = pad_inputs(paths, weight, resolution)
    x_star = exact_minimiser(t, wp, pw)
    f_star = objective(x_star, t, wp, pw)
    out = []
    for fix, scale in zip(runs, scales):
        x = np.concatenate([np.asarray(fix, dtype=np.float64), np.zeros((3, 3))], axis=1)
        x[:2] *= rw
        ts = t * scale
        x = x + ts
        x[:, -3:] = (x_star * scale)[:, -3:]                                 # the padding is not returned: take the minimiser's
        out.append((float(np.abs(x - x_star * scale).max()), float(objective(x, ts, wp, pw) - f_star * scale * scale)))
    return out


PERTURBATION_SCALES = [1.0] + [1 + k * 2.0 ** -52 for k in (1, 2, 3, 4)] + [1 - k * 2.0 ** -52 for k in (1, 2, 3, 4)]


def converged_ratios(golden, name, engine_fix):
    """d(engine) / max d(ref) and g(engine) / max g(ref) over the nine recorded reference runs of a converged case."""
    paths, w = golden[f"ref/{name}/paths"], golden[f"ref/{name}/weight"]
    runs = [golden[f"ref/{name}/out100"]] + list(golden[f"ref/{name}/pert100"])
    ref = converged_measures(paths, w, CASES[name][2], penalty_weight(name), runs, PERTURBATION_SCALES)
    d_hip, g_hip = converged_measures(paths, w, CASES[name][2], penalty_weight(name), [engine_fix], [1.0])[0]
    d_ref, g_ref = max(m[0] for m in ref), max(m[1] for m in ref)
    return d_hip, d_ref, g_hip, g_ref
