"""find_transform on the HIP engine, the part that needs no GPU: the restatement tests/find_transform_ref.py (closed-form gradients,
float64 = truth) against torch autograd and against the reference's own fp32 run in tests/golden/find_transform.npz, the bound the
GPU test uses shown to be met by an independent fp32 implementation and missed 10-fold by seven deliberate mistakes, and the
host-only side of the C ABI.

The loss is L1, so two correct fp32 implementations part ways wherever a residual or an outlier test lands on a tie.  Accuracy is
therefore measured per case as an RMS over the pairs against float64 and bounded by K times the reference's own such error plus one
fp32 ulp of the normalised coordinate (find_transform_ref.output_bound; measured values: profiles/find_transform_errloc.txt)."""
import ctypes
import importlib
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import find_transform_ref as R
from conftest import ROOT

from oracle import refstub


def engine_module():
    # nunif_amd.stlizer exports the function under the module's own name, so the attribute is the function
    return importlib.import_module("nunif_amd.stlizer.find_transform")


@pytest.mark.parametrize("name", ["b", "c", "h"])
def test_closed_form_gradient_equals_autograd_in_float64(name):
    xy1, xy2, mask, center, kwargs = R.fixture_input(name)
    B = xy1.shape[0]
    with torch.inference_mode(False), torch.enable_grad():
        xy1n, xy2n, _ = R.normalise(xy1.clone(), xy2.clone(), center.clone(), mask, torch.float64)
        mask = mask.clone()
        g = torch.Generator().manual_seed(5)
        for sigma in (None, 2.0):
            t = ((torch.rand((B, 1, 2), generator=g, dtype=torch.float64) - 0.5) * 0.1).requires_grad_(True)
            s = (1.0 + (torch.rand((B, 1, 1), generator=g, dtype=torch.float64) - 0.5) * 0.1).requires_grad_(True)
            r = ((torch.rand((B, 1, 1), generator=g, dtype=torch.float64) - 0.5) * 0.1).requires_grad_(True)
            sel = R.select((R.transform(xy1n, t, s, r)[1] - xy2n).abs().detach(), mask, sigma)
            assert int(sel.sum()) > 0
            R.loss_value(xy1n, xy2n, t, s, r, sel).backward()
            g_t, g_s, g_r = [x.detach() / int(sel.sum()) for x in R.gradient_sums(xy1n, xy2n, t.detach(), s.detach(), r.detach(), sel)]
            assert (g_t - t.grad.view(B, 2)).abs().max() <= 1e-12
            assert (g_s - s.grad.view(B)).abs().max() <= 1e-12
            assert (g_r - r.grad.view(B)).abs().max() <= 1e-12


@pytest.mark.parametrize("sum_dtype", [None, torch.float64], ids=["torch_sums", "double_sums"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_restatement_meets_the_bound_of_the_gpu_test(name, sum_dtype):
    """e_alt <= K * e_ref + floor on the outputs (cases with enough pairs) and on the first three trace steps (every case)."""
    alt = R.restated(name, torch.float32, None, sum_dtype)
    if name in R.RMS_CASES:
        e_ref, e_alt = R.output_errors(R.fixture_output(name), R.restated(name)), R.output_errors(alt, R.restated(name))
        print(name, "e_ref", e_ref, "e_alt", e_alt, "bound", R.output_bound(name))
    ratio = R.worst_ratio(name, alt[:3], alt[4])
    print(name, "worst error / bound", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixture_trace_starts_on_the_float64_trajectory(name):
    """The reference's own first three steps sit within a few ulp of the restatement's: schedule, bias corrections and the batch-wide
    mean of the restatement are the reference's (a wrong one is off by far more: see the mutations)."""
    ref_trace, truth = R.fixture_output(name)[3], R.restated(name)[4]
    assert ref_trace.shape == truth.shape == (R.CASES[name][4]["iteration"], len(R.CASES[name][1]), 4)
    assert float(R.trace_errors(ref_trace, truth).max()) <= 4 * R.ULP


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_mutation_misses_the_bound_tenfold_on_pass2s_own_call(mutate):
    """Case h has pairs of 3 .. 33 points next to the large ones: only a pair without an outlier can have an element below
    ``mean - sigma * std`` (the losses are non-negative), which is where the two-sided test differs."""
    got = R.restated("h", torch.float64, mutate)
    ratio = R.worst_ratio("h", got[:3], got[4])
    print(mutate, "error / bound", ratio)
    assert ratio >= 10.0


def test_wrong_divisor_shows_on_the_non_empty_pairs_of_case_j():
    """The GPU test holds pairs 0, 2, 3 of case j to the output bound over those three pairs: the fp32 restatements meet it, and
    dividing by the pair's own count instead of the batch's (the empty pair adds nothing to either) misses it 10-fold."""
    keep = [0, 2, 3]
    for sum_dtype in (None, torch.float64):
        assert R.output_ratio("j", R.restated("j", torch.float32, None, sum_dtype), keep) <= 1.0
    ratio = R.output_ratio("j", R.restated("j", torch.float64, "pair_count"), keep)
    print("pair_count on j", ratio)
    assert ratio >= 10.0


def test_empty_pair_stays_at_the_identity():
    shift, scale, angle, _, _ = R.restated("j")
    assert torch.equal(shift[1], torch.zeros(2, dtype=torch.float64)) and scale[1] == 1.0 and angle[1] == 0.0


needs_reference = pytest.mark.skipif(not refstub.reference_available(), reason="reference checkout not mounted")


@needs_reference
def test_signature_is_the_references():
    refstub.install()
    from nunif.utils import superpoint as KU
    assert inspect.signature(engine_module().find_transform) == inspect.signature(KU.find_transform)


@needs_reference
def test_pack_points_equals_the_references():
    refstub.install()
    from stlizer import multipass_pipeline as MP
    g = torch.Generator().manual_seed(3)
    b1 = [torch.rand((n, 2), generator=g) * 500 for n in (5, 0, 17, 9)]
    b2 = [torch.rand((n, 2), generator=g) * 500 for n in (5, 0, 17, 9)]
    for got, ref in zip(engine_module().pack_points(b1, b2), MP.pack_points(b1, b2)):
        assert got.dtype == ref.dtype and torch.equal(got, ref)


@needs_reference
def test_fixture_regenerates_to_the_committed_values(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tests", "golden"))
    G = importlib.import_module("make_find_transform")
    monkeypatch.delitem(sys.modules, "make_find_transform")
    fx = R.fixture()
    with torch.inference_mode(False):
        got = G.generate()
    assert set(got) == set(fx)
    for key, value in got.items():
        assert np.array_equal(fx[key], value), key


def test_fixture_inputs_are_the_seeded_cases():
    for name in R.CASES:
        for got, want in zip(R.fixture_input(name)[:4], R.case_input(name)[:4]):
            assert (got is None and want is None) or torch.equal(got, want), name


def test_workspace_bytes_matches_the_documented_layout(hiplib):
    def align256(v):
        return (v + 255) // 256 * 256
    for B, N, it in [(1, 1, 1), (3, 65, 20), (16, 257, 50), (32, 1025, 20), (4096, 8192, 1024), (7, 33, 63)]:
        want = align256(4 * it) + align256(96 * B) + 2 * align256(8 * B * N)
        assert hiplib.nunif_hip_find_transform_workspace_bytes(B, N, it) == want, (B, N, it)
        assert engine_module().workspace_bytes(B, N, it) == want


def test_arguments_beyond_the_limits_are_refused(hiplib):
    for B, N, it in [(0, 1, 1), (4097, 1, 1), (1, 0, 1), (1, 8193, 1), (1, 1, 0), (1, 1, 1025), (-1, 5, 5)]:
        assert hiplib.nunif_hip_find_transform_workspace_bytes(B, N, it) == -1, (B, N, it)
        with pytest.raises(ValueError, match="find_transform"):
            engine_module().workspace_bytes(B, N, it)
        # refused before any pointer is touched or anything is launched
        status = hiplib.nunif_hip_find_transform(None, None, None, None, B, N, it, 0.1, 0.1, 2.0, 0.0, 2.0, 8, None, None, None, None, 0,
                                                 None, None)
        assert status != 0 and b"bad shape" in hiplib.nunif_hip_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert hiplib.nunif_hip_find_transform(p, p, None, p, 1, 1, 1, 0.1, 0.1, 2.0, 0.0, 2.0, 32, p, p, p, p, 1 << 20, None, None) != 0
    assert b"flags" in hiplib.nunif_hip_last_error()


def test_host_tensor_2d_input_and_fp16_raise_naming_the_references_function():
    M = engine_module()
    xy = torch.zeros((2, 4, 2))
    with pytest.raises(RuntimeError, match=r"nunif\.utils\.superpoint\.find_transform"):
        M.find_transform(xy, xy, torch.zeros((2, 2)))
    with pytest.raises(RuntimeError, match=r"nunif\.utils\.superpoint\.find_transform"):
        M.find_transform(xy[0], xy[0], [0.0, 0.0])
    from nunif_amd import stlizer
    assert stlizer.find_transform is M.find_transform and stlizer.pack_points is M.pack_points and stlizer.pass2 is M.pass2
