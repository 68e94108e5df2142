"""sbs.row_flow_v2 on the GPU (csrc/rowflow_v2.hip: one launch, R x T = 5 x 62 output pixels per workgroup pass).

delta and the six debug taps are held region by region to the float64 net, with the error of the reference's own fp16 autocast
(tests/row_flow_v2_ref.py ``emulated``) as the yardstick: ``errloc.check_localised`` with the side nets' limits (2.1 global, 3.6 per
region) for delta and the project's tap limits (3.5 / 5.5) for the taps, cells = the kernel's band x tile, aligned and
half-shifted.  tests/test_row_flow_v2_cpu.py shows that kernel-shaped mistakes fail exactly this check.  Shapes: the smallest at
which the kernel can go wrong — narrower than the halo (1 x 8), odd (3 x 31), the fixture's, T-1 / T / T+1 / 2T+1 columns,
R-1 / R / R+1 rows, and 392 x 686 = 948 tiles, more than the persistent grid of 512 holds.

Worst ratios measured on an MI355X: see profiles/row_flow_v2_errloc.txt.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import errloc as E
import row_flow_v2_ref as V
import sidenet_cases as S
from conftest import GOLDEN, psnr
from oracle import row_flow_v3 as ORF
from oracle.forward_warp import synth_depth

from nunif_amd.synthetic import row_flow_v2_state_dict

pytestmark = pytest.mark.gpu

R, T = V.R, V.T
SHAPES = [(1, 1, 8), (1, 3, 31), (2, 58, 104),
          (1, R + 1, T - 1), (1, R + 1, T), (1, R + 1, T + 1), (1, R + 1, 2 * T + 1), (1, R - 1, T + 1), (1, R, T + 1)]
BIG = (1, 392, 686)
CASES = [(s, f) for s in SHAPES for f in (False, True)]


@functools.lru_cache(maxsize=None)
def _sd():
    return row_flow_v2_state_dict(V.WEIGHT_SEED)


def _planes(shape, seed=7):
    b, h, w = shape
    return ORF.make_input(synth_depth(seed, b, h, w, "smooth_edges"), 2.0, 0.5, max(h, w))


@functools.lru_cache(maxsize=None)
def _refs(shape, flip, taps=False):
    """(x, float64, emulation[, taps64, taps_emulated]) of one case, computed once per process and left unchanged."""
    E.set_threads()
    with torch.inference_mode():
        x = _planes(shape)
        t64, te = ({}, {}) if taps else (None, None)
        return x, V.oracle64(_sd(), x, flip, taps=t64), V.emulated(_sd(), x, flip, taps=te), t64, te


@pytest.fixture(scope="module")
def model(hiplib):
    from nunif_amd.iw3.models.row_flow_v2 import RowFlowV2
    m = RowFlowV2().eval()
    m.load_state_dict(_sd(), strict=True)
    m = m.to("cuda:0")
    m.delta_output = True
    return m


@pytest.fixture(scope="module")
def g():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "row_flow_v2.npz")).items()}


def _check(y, y64, ye, A, B, label):
    st = E.localised_stats(y, y64, ye, V.CELLS, B, S.tau_for(y64))
    print(f"[row_flow_v2 errloc] {label}: global {st['global']:.3f} worst {st['worst']:.3f}")
    return E.assert_localised(st, A, B, S.tau_for(y64), label)


@pytest.mark.parametrize("shape,flip", CASES + [(BIG, False), (BIG, True)], ids=lambda v: str(v).replace(" ", ""))
def test_delta_localised_against_float64(model, shape, flip):
    x, y64, ye, _, _ = _refs(shape, flip)
    y = model.infer_delta(x.to("cuda:0"), flip=flip).cpu()
    assert y.shape == (shape[0], 1) + shape[1:]
    _check(y, y64, ye, E.A_SIDE, E.B_SIDE, f"delta {shape} flip={flip}")


@pytest.mark.parametrize("shape,flip", [((2, 58, 104), False), ((1, R + 1, 2 * T + 1), True), ((1, 3, 31), True)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_debug_taps_localised_against_float64(model, shape, flip):
    x, y64, ye, t64, te = _refs(shape, flip, True)
    y, taps = model.debug_taps(x.to("cuda:0"), flip=flip)
    assert torch.equal(y, model.infer_delta(x.to("cuda:0"), flip=flip))            # the debug launch computes the same delta
    assert list(taps) == list(V.TAP_NAMES)
    for name in V.TAP_NAMES:
        _check(taps[name].cpu(), t64[name], te[name], E.A_TAP, E.B_TAP, f"tap {name} {shape} flip={flip}")
    assert torch.equal(taps["non_overlap"] + taps["residual"], y)                  # the sum is formed in fp32


def test_flip_is_the_unflipped_call_on_the_mirrored_planes(model):
    for shape in ((2, 58, 104), (1, R + 1, 2 * T + 1), (1, 1, 8)):
        x = _planes(shape).to("cuda:0")
        assert torch.equal(model.infer_delta(x, flip=True), model.infer_delta(torch.flip(x, (3,)).contiguous(), flip=False))


def test_batch_independent_and_deterministic_across_calls_and_streams(model):
    x = _planes((3, 58, 104)).to("cuda:0")
    y = model.infer_delta(x)
    for b in range(3):
        assert torch.equal(model.infer_delta(x[b:b + 1].contiguous()), y[b:b + 1])
    assert torch.equal(model.infer_delta(x), y)
    big = _planes(BIG).to("cuda:0")
    y0 = model.infer_delta(big)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = model.infer_delta(big)
    with torch.cuda.stream(s2):
        b = model.infer_delta(big, flip=True)
    torch.cuda.synchronize()
    assert torch.equal(a, y0) and torch.equal(b, model.infer_delta(big, flip=True))


def test_end_to_end_against_the_reference_fixture(model, g):
    from nunif_amd.iw3.backward_warp import apply_divergence_nn_LR
    depth, c = (t.to("cuda:0") for t in V.fixture_inputs())
    d2 = model(ORF.make_input(depth, 2.0, 0.5, 104))
    assert d2.shape == (2, 2, 58, 104) and float(d2[:, 1].abs().max()) == 0.0
    packed = torch.cat([c, ORF.make_input(depth, 2.0, 0.5, 104), torch.zeros_like(c[:, :2])], dim=1)
    assert torch.equal(model(packed), d2)                                          # the 8-channel packed input
    left, right = apply_divergence_nn_LR(model, c, depth, 2.0, 0.5, steps=1, synthetic_view="both")
    assert psnr(left.cpu(), g["left"]) >= 50.0 and psnr(right.cpu(), g["right"]) >= 50.0, \
        (psnr(left.cpu(), g["left"]), psnr(right.cpu(), g["right"]))
    ls, rs = apply_divergence_nn_LR(model, c[:1], depth[:1], 3.0, 0.5, steps=2, synthetic_view="both")
    assert psnr(ls.cpu(), g["left_s2"]) >= 50.0 and psnr(rs.cpu(), g["right_s2"]) >= 50.0, \
        (psnr(ls.cpu(), g["left_s2"]), psnr(rs.cpu(), g["right_s2"]))
    lo, ro = apply_divergence_nn_LR(model, c[:1], depth[:1], 2.0, 0.5, steps=1, synthetic_view="right")
    assert torch.equal(lo, c[:1]) and psnr(ro.cpu(), g["right_only"]) >= 50.0


def test_apply_divergence_method_name_stereo_width_and_convergence_tensor(model):
    from nunif_amd.iw3.utils import apply_divergence
    from conftest import synth_image
    depth = synth_depth(5, 2, 58, 104, "smooth_edges").to("cuda:0")
    c = torch.stack([synth_image(73, 3, 116, 208), synth_image(74, 3, 116, 208)]).to("cuda:0")
    args = SimpleNamespace(mapper="none", convergence=0.5, divergence=2.0, method="row_flow_v2", synthetic_view="both",
                           warp_steps=None, stereo_width=156, preserve_screen_border=False, disable_amp=False)
    left, right = apply_divergence(depth, c, args, side_model=model)
    assert left.shape == right.shape == c.shape and (left - c).abs().mean().item() > 1e-3
    assert bool(torch.isfinite(left).all()) and bool(torch.isfinite(right).all())
    args.convergence = torch.full((2, 1, 1, 1), 0.5, device="cuda:0")
    lt, rt = apply_divergence(depth, c, args, side_model=model)
    assert torch.equal(lt, left) and torch.equal(rt, right)                        # per-frame tensor == the scalar, byte for byte


def test_a_cpu_resident_model_raises(hiplib):
    from nunif_amd.iw3.models.row_flow_v2 import RowFlowV2
    cpu_model = RowFlowV2().eval()
    cpu_model.delta_output = True
    with pytest.raises(RuntimeError):
        cpu_model(torch.rand(1, 3, 64, 64))         # no engine on the CPU: no fallback
