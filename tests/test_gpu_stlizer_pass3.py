"""stlizer pass 3 on the engine against the reference's recorded float64 (tests/golden/stlizer_pass3*.npz, written by
tests/golden/make_stlizer_pass3.py) with the longdouble restatement (tests/stlizer_pass3_ref.py) as the yardstick.

Every numeric pin has the project's form ``e_hip <= 2.2 * e_ref + one float64 ulp of the largest path value``: ``e_ref`` is the
reference's own recorded float64 against the longdouble run, ``e_hip`` the engine's against the same run.  The reference's LBFGS
is chaotic under rounding (DESIGN.md has the table), so this holds over the first steps only (``iteration = 3``); at 100 steps the
engine is held to the family of rounding-perturbed reference runs instead: its distance to the exact minimiser and its objective
gap are at most twice the worst of the nine recorded reference runs.

The decision log is compared record for record in its decisions (which exit, memory update taken or not) with the restatement
run in the engine's shape (float64 throughout, x alone held wider, ``wide_x``); its float fields are sums that the engine
associates differently and are held to 1e-6 relative on the ordinary cases.
"""
import functools
import os
import types

import numpy as np
import pytest
import torch

import stlizer_pass3_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 2.2
FLOAT_FIELDS = ("loss", "maxg", "gtd", "ys", "maxg_new", "maxdt", "dloss")
ORDINARY = ("n4", "n5", "n37", "n255", "n256", "n257", "n300", "n1025", "n5000", "tiny")


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(os.path.join(GOLDEN, "stlizer_pass3.npz")))
    g.update(np.load(os.path.join(GOLDEN, "stlizer_pass3_n5000.npz")))
    return g


@functools.lru_cache(maxsize=None)
def yardstick(name, iteration=3):
    """The longdouble run of a case on the reference's own float64 paths -> out, trace, and the log of the engine-shaped run."""
    g = golden()
    paths, w, res = g[f"ref/{name}/paths"], g[f"ref/{name}/weight"], R.CASES[name][2]
    out, trace, _ = R.grad_opt(paths, w, res, iteration, R.penalty_weight(name), dtype=np.longdouble)
    # the decisions of the engine's shape: float64 throughout, x alone held wider (the engine holds it in two doubles)
    _, _, log64 = R.grad_opt(paths, w, res, iteration, R.penalty_weight(name), wide_x=True)
    return out, trace, log64


def ulp_of(a):
    return float(np.spacing(np.abs(np.asarray(a, dtype=np.float64)).max()))


def err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.longdouble) - np.asarray(b, dtype=np.longdouble)).max())


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def decode(lg):
    """Device records [slots, 32] -> the restatement's (exit, accepted) pairs and the float fields."""
    from nunif_amd.stlizer.pass3 import REC
    lg = lg.cpu().numpy()
    recs = []
    for row in lg:
        exit_code = int(row[REC["exit_begin"]]) or int(row[REC["exit_gtd"]]) or int(row[REC["exit_after"]])
        rec = {"exit": exit_code, "accepted": int(row[REC["accepted"]])}
        rec.update({key: row[REC[key]] for key in FLOAT_FIELDS})
        recs.append(rec)
    return recs


def compare_floats(name, got, want):
    """Every float field the restatement's record holds, to 1e-6 relative: they are sums that the engine associates differently.
    dloss is a difference of two losses, each good to about 1e-13 of itself: it gets that much of the loss on top."""
    for j, (a, b) in enumerate(zip(got, want)):
        for key in FLOAT_FIELDS:
            if np.isnan(float(b[key])):
                continue
            atol = 1e-12 * abs(float(b["loss"])) if key == "dloss" else 0.0
            assert np.isclose(a[key], float(b[key]), rtol=1e-6, atol=atol), (name, j, key, a[key], b[key])


def run_engine(name, iteration=3, **kw):
    from nunif_amd.stlizer import pass3 as P
    g = golden()
    out, tr, lg = P.grad_opt_traced(dev(g[f"ref/{name}/paths"]), dev(g[f"ref/{name}/weight"]), R.CASES[name][2], iteration,
                                    R.penalty_weight(name), **kw)
    return out, tr, lg


@pytest.mark.parametrize("name", list(R.CASES))
def test_scene_weight_is_bit_equal(name):
    from nunif_amd.stlizer.pass3 import calc_scene_weight
    g = golden()
    w = calc_scene_weight(dev(g[f"in/{name}/scores"]))
    assert w.dtype == torch.float32 and torch.equal(w.cpu(), torch.from_numpy(g[f"ref/{name}/weight"]))
    w2 = calc_scene_weight(g[f"in/{name}/scores"].tolist(), device=DEV)
    assert torch.equal(w2.cpu(), w.cpu())


@pytest.mark.parametrize("name", list(R.CASES))
def test_prefix_sums_within_the_references_own_error(name):
    from nunif_amd.stlizer.pass3 import prepare
    g = golden()
    sx, sy, an = (g[f"in/{name}/{k}"] for k in ("shift_x", "shift_y", "angle"))
    w = g[f"ref/{name}/weight"]
    exact = R.prepare(sx, sy, an, w, dtype=np.longdouble)
    ref = g[f"ref/{name}/paths"]
    got = prepare(dev(sx), dev(sy), dev(an), dev(w)).cpu().numpy()
    e_ref, e_hip = err(ref, exact), err(got, exact)
    print(f"{name}: prefix e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip <= FACTOR * e_ref + ulp_of(ref)


@pytest.mark.parametrize("method", ["gaussian", "savgol"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_filters_within_the_references_own_error(name, method):
    from nunif_amd.stlizer import pass3 as P
    g = golden()
    paths, taps, fps = g[f"ref/{name}/paths"], g[f"ref/{name}/taps_{method}"], R.CASES[name][3]
    ours = P.gen_smoothing_kernel(method, R.kernel_size(R.SMOOTHING_SECONDS, fps), DEV)
    assert ours.shape == (1, 1, taps.shape[0]) and ours.dtype == torch.float64
    # the same expressions on another host: exp, the sum and the division may each round the other way
    assert np.allclose(ours.flatten().cpu().numpy(), taps, rtol=4 * 2.0 ** -52, atol=0.0)
    exact = R.conv_fix(paths, taps, dtype=np.longdouble)
    ref = g[f"ref/{name}/{method}"]
    p = dev(paths)
    got = P.smoothing_fix(p, dev(taps)).cpu().numpy()                        # the kernel on the reference's own taps
    fix = P.conv1d_smoothing(p[0].reshape(1, 1, -1), p[1].reshape(1, 1, -1), p[2].reshape(1, 1, -1), method, R.SMOOTHING_SECONDS,
                             fps, DEV)
    assert all(f.shape == (paths.shape[1],) and f.dtype == torch.float64 for f in fix)
    scale = np.abs(paths).max() + 1e-300
    assert np.abs(torch.stack(fix).cpu().numpy() - got).max() <= 16 * 2.0 ** -52 * scale     # taps that differ by 4 ulp at most
    e_ref, e_hip = err(ref, exact), err(got, exact)
    print(f"{name} {method}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip <= FACTOR * e_ref + ulp_of(paths)


@pytest.mark.parametrize("name", list(R.ITER3_CASES))
def test_trajectory_parity_at_three_steps(name):
    """The test that shows the feature: it needs nunif_amd.stlizer.pass3 and the grad_opt symbol."""
    g = golden()
    exact_out, exact_trace, log64 = yardstick(name)
    ref = g[f"ref/{name}/out3"]
    out, tr, lg = run_engine(name, trace=True, log=True)
    out, tr = out.cpu().numpy(), tr.cpu().numpy()
    rw = R.CASES[name][2] / R.DEFAULT_RESOLUTION
    ulp = ulp_of(g[f"ref/{name}/paths"] * rw)
    e_ref, e_hip = err(ref, exact_out), err(out, exact_out)
    print(f"{name}: e_ref {e_ref:.3e} e_hip {e_hip:.3e} bound {FACTOR * e_ref + ulp:.3e}")
    assert tr.shape == exact_trace.shape == (12, 3, ref.shape[1] + 3)
    assert e_hip <= FACTOR * e_ref + ulp
    # the last trace row is the x the fixes come from, in the optimizer's units (the fixes times resolution / 320)
    assert err(tr[-1], exact_trace[-1]) <= FACTOR * e_ref * rw + ulp
    got = decode(lg)
    assert [(r["exit"], r["accepted"]) for r in got] == [(r["exit"], r["accepted"]) for r in log64]
    if name in ORDINARY:
        compare_floats(name, got, log64)


@pytest.mark.parametrize("name", list(R.ITER3_CASES))
def test_every_trace_row_within_the_output_bound(name):
    """Every trace row against the longdouble run, held to the bound of the outputs: ``2.2 * e_ref + ulp`` with ``e_ref`` the
    reference's recorded OUTPUT against the longdouble run.  The iterates between the steps are ten times more sensitive to the
    rounding of x than the third step's result (a numpy run with x in float64 misses this bound on six cases, 6.0e-11 against
    7.3e-12 on n255); the engine meets it because it holds x in two doubles."""
    g = golden()
    exact_out, exact_trace, _ = yardstick(name)
    _, tr, _ = run_engine(name, trace=True)
    tr = tr.cpu().numpy()
    rw = R.CASES[name][2] / R.DEFAULT_RESOLUTION
    e_ref = err(g[f"ref/{name}/out3"], exact_out)
    e_rows = [err(tr[j], exact_trace[j]) for j in range(tr.shape[0])]
    print(f"{name}: worst trace row {max(e_rows):.3e} (row {int(np.argmax(e_rows))}) bound {FACTOR * e_ref * rw:.3e}")
    assert max(e_rows) <= FACTOR * e_ref * rw + ulp_of(g[f"ref/{name}/paths"] * rw)


@pytest.mark.parametrize("name", list(R.ENGINE_EXIT_CASES))
def test_early_exit_cases(name):
    exact_out, _, log64 = yardstick(name)
    out, _, lg = run_engine(name, log=True)
    codes = [r["exit"] for r in decode(lg)]
    assert R.ENGINE_EXIT_CASES[name] in codes and codes == [r["exit"] for r in log64]
    ref = golden()[f"ref/{name}/out3"]
    assert err(out.cpu().numpy(), exact_out) <= FACTOR * err(ref, exact_out) + ulp_of(golden()[f"ref/{name}/paths"])


@pytest.mark.parametrize("name", ["zero", "n1", "n2"])
def test_nothing_to_smooth_is_exactly_zero(name):
    out, _, _ = run_engine(name)
    assert torch.equal(out.cpu(), torch.zeros_like(out.cpu()))


@pytest.mark.parametrize("name", list(R.CONVERGED_CASES))
def test_converged_parity_with_the_family_of_reference_runs(name):
    """tools/time_pass3.py computes the same ratios with the same function and writes them to profiles/stlizer_pass3.txt."""
    out, _, _ = run_engine(name, iteration=100)
    d_hip, d_ref, g_hip, g_ref = R.converged_ratios(golden(), name, out.cpu().numpy())
    print(f"{name}: d(engine) {d_hip:.3e} max d(ref) {d_ref:.3e} ratio {d_hip / d_ref:.3f}; "
          f"g(engine) {g_hip:.3e} max g(ref) {g_ref:.3e} ratio {g_hip / g_ref:.3f}")
    assert d_hip <= 2 * d_ref and g_hip <= 2 * g_ref


@functools.lru_cache(maxsize=None)
def long_yardstick():
    sx, sy, an, scores, res, fps = R.long_case()
    w = R.calc_scene_weight(scores)
    paths = R.prepare(sx, sy, an, w)
    exact = R.grad_opt(paths, w, res, 3, R.penalty_weight(), dtype=np.longdouble)
    f64 = R.grad_opt(paths, w, res, 3, R.penalty_weight())
    return (sx, sy, an, scores, res, fps), w, paths, exact, f64


def test_a_path_of_70000_frames_takes_the_second_trip_of_every_finishing_loop():
    """N = 70 000: 274 tiles per axis, 822 partials, so each thread of a finishing pass sums more than one partial and each thread
    of the prefix kernel more than one tile sum.  Too long for a fixture: the inputs are generated here and ``e_ref`` is the
    float64 restatement's own error against the longdouble run."""
    from nunif_amd.stlizer import pass3 as P
    (sx, sy, an, scores, res, fps), w, paths, exact, f64 = long_yardstick()
    assert P.workspace_bytes(R.LONG_N, 3) > 0 and (R.LONG_N + 3 + 255) // 256 > 256
    weight = P.calc_scene_weight(dev(scores))
    assert np.array_equal(weight.cpu().numpy(), w)
    # prefix sums
    exact_paths = R.prepare(sx, sy, an, w, dtype=np.longdouble)
    got_paths = P.prepare(dev(sx), dev(sy), dev(an), weight).cpu().numpy()
    e_ref, e_hip = err(paths, exact_paths), err(got_paths, exact_paths)
    print(f"long: prefix e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip <= FACTOR * e_ref + ulp_of(paths)
    # a filter over tile edges far from the ends
    taps = R.gaussian_taps(R.kernel_size(R.SMOOTHING_SECONDS, fps))
    exact_fix = R.conv_fix(paths, taps, dtype=np.longdouble)
    got_fix = P.smoothing_fix(dev(paths), dev(taps)).cpu().numpy()
    e_ref, e_hip = err(R.conv_fix(paths, taps), exact_fix), err(got_fix, exact_fix)
    print(f"long: gaussian e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip <= FACTOR * e_ref + ulp_of(paths)
    # three steps of grad_opt: fixes, every iterate, every decision
    out, tr, lg = P.grad_opt_traced(dev(paths), weight, res, 3, R.penalty_weight(), trace=True, log=True)
    out, tr = out.cpu().numpy(), tr.cpu().numpy()
    e_ref, e_hip = err(f64[0], exact[0]), err(out, exact[0])
    e_rows = max(err(tr[j], exact[1][j]) for j in range(tr.shape[0]))
    print(f"long: e_ref {e_ref:.3e} e_hip {e_hip:.3e} worst trace row {e_rows:.3e}")
    assert e_hip <= FACTOR * e_ref + ulp_of(paths) and e_rows <= FACTOR * e_ref + ulp_of(paths)
    got = decode(lg)
    assert min(R.margins(f64[2])) >= 4.0
    assert [(r["exit"], r["accepted"]) for r in got] == [(r["exit"], r["accepted"]) for r in f64[2]]
    compare_floats("long", got, f64[2])


@pytest.mark.parametrize("n", [40, 300])
def test_the_longest_filter(n):
    """K = 4097 taps, the most the entry takes: the window of a tile is 4352 doubles and every thread loads 17 of them; at N = 40
    nearly all of it is replicated padding, at N = 300 there are two tiles."""
    from nunif_amd.stlizer import pass3 as P
    sx, sy, an = R.jitter_path(41, n)
    paths = R.prepare(sx, sy, an, R.calc_scene_weight(R.match_scores(41, n, (n // 2,))))
    taps = R.gaussian_taps(P.MAX_TAPS)
    exact = R.conv_fix(paths, taps, dtype=np.longdouble)
    got = P.smoothing_fix(dev(paths), dev(taps)).cpu().numpy()
    e_ref, e_hip = err(R.conv_fix(paths, taps), exact), err(got, exact)
    print(f"K 4097 N {n}: e_ref {e_ref:.3e} e_hip {e_hip:.3e}")
    assert e_hip <= FACTOR * e_ref + ulp_of(paths)


def test_the_filter_entry_refuses_too_many_and_even_taps():
    from nunif_amd import _hip
    from nunif_amd.stlizer import pass3 as P
    paths = torch.zeros((3, 8), dtype=torch.float64, device=DEV)
    for k in (P.MAX_TAPS + 2, 4, 0):
        with pytest.raises(_hip.NunifHipError) as e:
            P.smoothing_fix(paths, torch.ones(max(k, 1), dtype=torch.float64, device=DEV)[:k])
        assert e.value.status == -1 and "taps" in str(e.value)


def test_two_calls_two_streams_and_a_reused_workspace_are_bit_equal():
    from nunif_amd.stlizer import pass3 as P
    first = run_engine("n257", trace=True)
    again = run_engine("n257", trace=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        other = run_engine("n257")
        torch.cuda.current_stream(DEV).synchronize()
    assert torch.equal(first[0], other[0])
    ws = torch.empty(P.workspace_bytes(1025, 3), dtype=torch.uint8, device=DEV)
    big = run_engine("n1025", workspace=ws)
    small = run_engine("n257", workspace=ws)                                 # the same bytes, another problem
    assert torch.equal(small[0], first[0]) and torch.equal(run_engine("n1025", workspace=ws)[0], big[0])


def test_a_short_workspace_and_shapes_outside_the_limits_are_refused():
    from nunif_amd import _hip
    from nunif_amd.stlizer import pass3 as P
    ws = torch.empty(P.workspace_bytes(37, 3) - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(_hip.NunifHipError) as e:
        run_engine("n37", workspace=ws)
    assert e.value.status == -1 and "workspace" in str(e.value)
    for n, it in ((0, 1), (P.MAX_FRAMES + 1, 1), (10, 0), (10, P.MAX_ITERATION + 1)):
        with pytest.raises(ValueError):
            P.workspace_bytes(n, it)
    with pytest.raises(ValueError):
        run_engine("n37", iteration=P.MAX_ITERATION + 1)
    with pytest.raises(ValueError):
        P.gen_smoothing_kernel("gaussian", P.MAX_TAPS + 2, DEV)
    cpu = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.grad_opt(cpu, cpu, cpu, torch.ones(8), 320)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.calc_scene_weight([0.8] * 8, device="cpu")


@pytest.mark.parametrize("method", ["grad_opt", "gaussian", "savgol"])
def test_pass3_over_transforms_equals_pass3_smoothing_and_host_lists_equal_the_tensors(method):
    from nunif_amd.stlizer import pass3 as P
    sx, sy, an = R.jitter_path(77, 40)
    an[3] = 100.0
    scores = R.match_scores(77, 40, (20,))
    transforms = [([float(sx[i]), float(sy[i])], 1.0, float(an[i]), [160.0, 90.0], 0.5) for i in range(40)]
    args = types.SimpleNamespace(state={"device": torch.device(DEV)}, resolution=480, filter=method, smoothing=2.0)
    weight = P.calc_scene_weight(scores.tolist(), device=DEV)
    fixes = P.pass3(transforms, weight, 30, args)
    direct = P.pass3_smoothing(dev(sx), dev(sy), dev(np.clip(an, -90, 90)), weight, method, 2.0, 30, 480, DEV)
    assert all(f.dtype == torch.float64 and f.shape == (40,) and f.device.type == "cuda" for f in fixes)
    assert all(torch.equal(a, b) for a, b in zip(fixes, direct))
    lists = P.pass3(transforms, weight, 30, args, host=True)
    assert all(isinstance(row, list) and row == f.cpu().tolist() for row, f in zip(lists, fixes))
