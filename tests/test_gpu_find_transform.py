"""find_transform on the HIP engine (nunif_amd/csrc/find_transform.hip, nunif_amd/stlizer/find_transform.py) on the GPU.

Accuracy is measured against the float64 restatement (tests/find_transform_ref.py) under the bound that
tests/test_find_transform_cpu.py shows an independent fp32 implementation to meet: per case the RMS over the pairs of the shift,
angle and scale errors within K times the reference's own fp32 error (tests/golden/find_transform.npz) plus one fp32 ulp of the
normalised coordinate, and the first three trace steps within K times the reference's own deviation plus one ulp.  Everything else
here is bit equality: the only coupling between pairs is an integer sum."""
import importlib
import types

import pytest
import torch

import find_transform_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def M():
    return importlib.import_module("nunif_amd.stlizer.find_transform")


def run_case(M, name, **extra):
    xy1, xy2, mask, center, kwargs = R.fixture_input(name)
    out = M.find_transform_traced(xy1.to(DEV), xy2.to(DEV), center.to(DEV), None if mask is None else mask.to(DEV), trace=True,
                                  **kwargs, **extra)
    return [t.cpu() for t in out]


@pytest.fixture(scope="module")
def results(M):
    """Every case once, in the order of CASES: one cached workspace serves all of them (different B, N, iteration)."""
    with torch.inference_mode():
        return {name: run_case(M, name) for name in R.CASES}


@pytest.mark.parametrize("name", list(R.CASES))
def test_outputs_and_early_trace_against_float64(results, name):
    shift, scale, angle, center, trace = results[name]
    B, it = len(R.CASES[name][1]), R.CASES[name][4]["iteration"]
    assert shift.shape == (B, 2) and scale.shape == (B, 1) and angle.shape == (B, 1) and center.shape == (B, 2)
    assert trace.shape == (it, B, 4) and torch.equal(center, R.fixture_input(name)[3])
    if name in R.RMS_CASES:
        print(name, "e_gpu", R.output_errors((shift, scale, angle), R.restated(name)), "bound", R.output_bound(name))
    print(name, "early trace error", R.trace_errors(trace, R.restated(name)[4]).tolist(), "bound", R.trace_bound(name).tolist())
    ratio = R.worst_ratio(name, (shift, scale, angle), trace)
    print(name, "worst error / bound", ratio)
    assert ratio <= 1.0


def test_outputs_follow_from_the_last_trace_step(results):
    for name, (shift, scale, angle, _, trace) in results.items():
        xy1, _, _, center, _ = R.fixture_input(name)
        ns = R.norm_scale_of(xy1, center).float().view(-1, 1)
        assert torch.equal(shift, trace[-1][:, 0:2] * ns), name
        assert torch.equal(scale, trace[-1][:, 2:3]), name
        assert (angle - torch.rad2deg(trace[-1][:, 3:4])).abs().max() <= 1e-5, name


def test_permuting_the_pairs_permutes_the_outputs_bit_for_bit(M, results):
    xy1, xy2, mask, center, kwargs = R.fixture_input("d")
    perm = torch.randperm(xy1.shape[0], generator=torch.Generator().manual_seed(2))
    assert not torch.equal(perm, torch.arange(xy1.shape[0]))
    got = M.find_transform_traced(xy1[perm].to(DEV), xy2[perm].to(DEV), center[perm].to(DEV), mask[perm].to(DEV), trace=True, **kwargs)
    shift, scale, angle, _, trace = [t.cpu() for t in got]
    want = results["d"]
    assert torch.equal(shift, want[0][perm]) and torch.equal(scale, want[1][perm]) and torch.equal(angle, want[2][perm])
    assert torch.equal(trace, want[4][:, perm])


def test_two_calls_and_two_streams_are_bit_equal(M, results):
    for name in ("c", "h"):
        again = run_case(M, name)
        stream = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(stream):
            other = run_case(M, name)
        stream.synchronize()
        for a, b, c in zip(results[name], again, other):
            assert torch.equal(a, b) and torch.equal(a, c), name


def test_trace_is_optional_and_changes_nothing(M, results):
    xy1, xy2, mask, center, kwargs = R.fixture_input("c")
    shift, scale, angle, c = M.find_transform(xy1.to(DEV), xy2.to(DEV), center.to(DEV).view(-1, 1, 2), mask.to(DEV), **kwargs)
    assert torch.equal(shift.cpu(), results["c"][0]) and torch.equal(scale.cpu(), results["c"][1])
    assert torch.equal(angle.cpu(), results["c"][2]) and c.shape == (3, 2) and c.device.type == "cuda"


def test_workspace_is_reused_and_grown_across_shapes(M, results):
    """The cached workspace served b (tiny), then e (largest), then j: a stale count slot or state of an earlier shape would show."""
    for name in ("e", "a", "h", "b"):
        for a, b in zip(results[name], run_case(M, name)):
            assert torch.equal(a, b), name
    need = M.workspace_bytes(32, 1025, 20)
    assert any(ws.numel() >= need for ws in M._workspaces.values())


def test_workspace_one_byte_short_is_refused(M, results):
    from nunif_amd._hip import NunifHipError
    need = M.workspace_bytes(3, 65, 20)
    exact = torch.empty(need, dtype=torch.uint8, device=DEV)
    for a, b in zip(results["c"], run_case(M, "c", workspace=exact)):
        assert torch.equal(a, b)
    with pytest.raises(NunifHipError, match="workspace"):
        run_case(M, "c", workspace=exact[:need - 1])


def test_empty_pair_keeps_the_identity_and_the_others_follow_their_batch(results):
    shift, scale, angle, _, trace = results["j"]
    assert torch.equal(shift[1], torch.zeros(2)) and scale[1] == 1.0 and angle[1] == 0.0
    assert torch.equal(trace[:, 1], torch.tensor([0.0, 0.0, 1.0, 0.0]).expand(trace.shape[0], 4))
    # the other pairs against the float64 answer for this batch of four, under the output bound over those three pairs
    # (tests/test_find_transform_cpu.py: a divisor other than the batch's count misses it)
    keep = [0, 2, 3]
    ratio = R.output_ratio("j", (shift, scale, angle), keep)
    print("j pairs 0, 2, 3: error / bound", ratio, R.output_bound("j", keep))
    assert ratio <= 1.0


def test_pass2_batches_and_returns_the_references_structure(M):
    g = torch.Generator().manual_seed(9)
    xy1, xy2, mask, _, _ = R.fixture_input("d")
    counts = [int(torch.randint(20, 120, (1,), generator=g)) for _ in range(40)]
    p1 = [xy1[i % 16, :n].clone() for i, n in enumerate(counts)]
    p2 = [xy2[i % 16, :n].clone() + 0.01 * i for i, n in enumerate(counts)]
    args = types.SimpleNamespace(state={"device": torch.device(DEV)}, batch_size=1, iteration=50)
    center, resize_scale = [284, 160], 0.5
    got = M.pass2(p1, p2, center, resize_scale, args)
    assert isinstance(got, list) and len(got) == 40
    k1, k2, km = M.pack_points(p1, p2)
    assert k1.shape == (40, max(counts), 2)
    want = []
    for a, b, m in zip(k1.split(32), k2.split(32), km.split(32)):
        c = torch.tensor(center, dtype=torch.float32, device=DEV).view(1, 2).expand(a.shape[0], 2)
        want.append(M.find_transform(a.to(DEV), b.to(DEV), c, mask=m.to(DEV), iteration=50, sigma=2.0, disable_scale=True))
    assert [w[0].shape[0] for w in want] == [32, 8]
    shift, scale, angle = [torch.cat([w[k] for w in want]).cpu() for k in range(3)]
    for i, t in enumerate(got):
        assert isinstance(t, tuple) and len(t) == 5
        assert isinstance(t[0], list) and len(t[0]) == 2 and all(type(v) is float for v in t[0])
        assert type(t[1]) is float and type(t[2]) is float and t[3] is center and t[4] == resize_scale
        assert t[0] == shift[i].tolist() and t[1] == scale[i].item() and t[2] == angle[i].item()
        assert t[1] == 1.0
    assert M.pass2([], [], center, resize_scale, args) == []


def test_host_tensor_2d_input_and_fp16_raise(M):
    xy = torch.zeros((2, 4, 2), device=DEV)
    c = torch.zeros((2, 2), device=DEV)
    for a, b in [(xy.cpu(), xy.cpu()), (xy[0], xy[0]), (xy.half(), xy.half()), (xy, xy.double())]:
        with pytest.raises(RuntimeError, match=r"nunif\.utils\.superpoint\.find_transform"):
            M.find_transform(a, b, c)


def test_needs_no_grad_mode(M, results):
    with torch.inference_mode(False), torch.no_grad():
        for a, b in zip(results["b"], run_case(M, "b")):
            assert torch.equal(a, b)
