"""stlizer's outpaint network and EMA frame buffer on the HIP engine (nunif_amd/csrc/outpaint.hip) against the float64 restatement
(tests/outpaint_f64.py), with the reference class's own fp32 result (tests/golden/outpaint.npz) as the yardstick.

Per tensor ``e_ref = max |reference fp32 - f64|`` and ``e_hip = max |engine - f64|``: the outputs of ``infer`` (composite, raw) and
of the eval ``forward`` must satisfy ``e_hip <= 2.2 * e_ref + A``, the five taps ``e_hip <= 3.5 * e_ref + A`` (the project's
constants, as tests/test_gpu_superpoint.py), ``A`` = two fp32 ulp at the tensor's largest magnitude.  The same two constants bound
every 8 x 8 cell of the map on its own (64 x 64 output pixels; aligned and shifted by half a cell, ``errloc.localised_stats`` with
B = the constant and tau = ``A``): a window, a pool tile and a pad corner each go wrong alone.  The composite and the forward are the
raw map behind a clamp and a ``where``: in a cell only the handful of masked pixels that the clamp does not saturate carry any error
at all, and the maximum over a handful of samples of two independent fp32 roundings is not bounded by a ratio.  A clamp is
1-Lipschitz, so their per-cell yardstick is the reference's error on the UNCLAMPED map in that cell.  Where the fixture does not hold a
tensor (cases d and g, the taps of c, d, f, g, the eval forward of the resized cases) the yardstick is the restatement in fp32, which
tests/test_outpaint_cpu.py ties to the reference class.  The composite and the forward yardsticks are the recorded raw map behind the
reference's own ``where`` / clamp (tests/outpaint_f64.finish).
Measured worst ratios on an MI355X: raw 1.773 (b: e_ref 1.65e-06, e_hip 2.92e-06), composite and forward 1.839 (a), taps 1.523 (b proj);
per cell raw 1.719 (d), taps 1.772 (b proj), composite 1.123, forward 1.081; buffer step 1.000; OutpaintBorder 1.146 / 0.737.
Parity is against SEEDED weights and synthetic frames: the released checkpoint is not available offline.
"""
import math
import os

import numpy as np
import pytest
import torch

import errloc as E
import outpaint_f64 as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATIO, TAP_RATIO = 2.2, 3.5


def ulp32(v):
    return 2.0 ** (math.floor(math.log2(max(float(v), 1e-30))) - 23)


def check(tag, hip, ref32, ref64, ratio=RATIO, cell=None, cell_noise=None):
    """``cell_noise`` = (fp32, float64) of the map whose error is the per-cell yardstick (default: ref32, ref64)."""
    hip, ref32, ref64 = (torch.as_tensor(t).double().cpu() for t in (hip, ref32, ref64))
    assert hip.shape == ref64.shape == ref32.shape, (tag, hip.shape, ref32.shape, ref64.shape)
    e_ref, e_hip = (ref32 - ref64).abs().max().item(), (hip - ref64).abs().max().item()
    A = 2 * ulp32(ref64.abs().max().item())
    print(f"\n[outpaint] {tag}: e_ref {e_ref:.4g} e_hip {e_hip:.4g} ratio {e_hip / max(e_ref, 1e-30):.3f} A {A:.3g}")
    assert e_hip <= ratio * e_ref + A, (tag, e_hip, e_ref, A)
    if cell:
        n32, n64 = (torch.as_tensor(t).double().cpu() for t in (cell_noise or (ref32, ref64)))
        st = E.localised_stats(hip, ref64, ref64 + (n32 - n64), [(cell, 0)], ratio, A)
        print(f"[outpaint] {tag}: worst cell ratio {st['worst']:.3f}")
        assert st["_finite"] and st["worst"] <= ratio, (tag, E.format_regions(st))


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "outpaint.npz")))


@pytest.fixture(scope="module")
def sd():
    from nunif_amd.synthetic import light_outpaint_state_dict
    return light_outpaint_state_dict(R.WEIGHT_SEED)


@pytest.fixture(scope="module")
def model(sd):
    from nunif_amd.stlizer.models.light_outpaint_v1 import LightOutpaintV1
    m = LightOutpaintV1()
    m.load_state_dict(sd)
    return m.eval().to("cuda")


_cache = {}


def restated_raw(sd, name, mode, dtype):
    """(the net's output at the frame's size, taps) of the restatement: what ``infer`` makes of it for ``raw`` / ``composite``,
    without the resize to max_size for ``forward``.  Computed once per (case, dtype) and shared."""
    x, mask = R.case_input(name)
    max_size = R.CASES[name][3]
    if mode == "forward" and max(x.shape[-2:]) <= max_size:
        mode = "raw"                                                # the same net call
    key = (name, "forward" if mode == "forward" else "raw", dtype)
    if key not in _cache:
        with torch.inference_mode():
            _cache[key] = R.infer(sd, x, mask, 2 ** 30 if key[1] == "forward" else max_size, "raw", dtype)
    return _cache[key]


def restated(sd, name, mode, dtype):
    x, mask = R.case_input(name)
    out, taps = restated_raw(sd, name, mode, dtype)
    return R.finish(x, mask, out, mode), taps


def yardstick_raw(sd, fixture, name, mode):
    B, H, W, max_size = R.CASES[name][:4]
    if f"out/{name}/raw" in fixture and (mode != "forward" or max(H, W) <= max_size):
        return torch.from_numpy(fixture[f"out/{name}/raw"])
    return restated_raw(sd, name, mode, torch.float32)[0]


def yardstick(sd, fixture, name, mode):
    x, mask = R.case_input(name)
    return R.finish(x, mask, yardstick_raw(sd, fixture, name, mode), mode)


def unclamped(sd, fixture, name, mode):
    return yardstick_raw(sd, fixture, name, mode), restated_raw(sd, name, mode, torch.float64)[0]


@pytest.mark.parametrize("name", list(R.CASES))
def test_infer_and_taps_against_float64(model, sd, fixture, name):
    x, mask = R.case_input(name)
    max_size = R.CASES[name][3]
    xd, md = x.cuda(), mask.cuda()
    raw = model.infer(xd, md, max_size=max_size, composite=False)
    taps = {t: model.debug_tap(t) for t in R.TAPS}
    comp = model.infer(xd, md, max_size=max_size, composite=True)
    assert raw.dtype == torch.float32 and raw.shape == x.shape
    check(f"{name} raw", raw, yardstick(sd, fixture, name, "raw"), restated(sd, name, "raw", torch.float64)[0], cell=64)
    check(f"{name} composite", comp, yardstick(sd, fixture, name, "composite"), restated(sd, name, "composite", torch.float64)[0], cell=64,
          cell_noise=unclamped(sd, fixture, name, "composite"))
    m3 = mask.expand_as(x)
    assert torch.equal(comp.cpu()[~m3], x[~m3]), "composite: pixels outside the mask are the input's"
    assert float(comp.cpu()[m3].min()) >= 0.0 and float(comp.cpu()[m3].max()) <= 1.0
    t64, t32 = restated(sd, name, "raw", torch.float64)[1], restated(sd, name, "raw", torch.float32)[1]
    for t in R.TAPS:
        key = f"tap/{name}/{t}"
        ref32 = torch.from_numpy(fixture[key]) if key in fixture else t32[t]
        check(f"{name} {t}", taps[t], ref32, t64[t], TAP_RATIO, cell=8)


@pytest.mark.parametrize("name", list(R.CASES))
def test_eval_forward_against_float64_and_its_definition(model, sd, fixture, name):
    x, mask = R.case_input(name)
    got = model(x.cuda(), mask.cuda())
    check(f"{name} forward", got, yardstick(sd, fixture, name, "forward"), restated(sd, name, "forward", torch.float64)[0], cell=64,
          cell_noise=unclamped(sd, fixture, name, "forward"))
    raw = model.infer(x.cuda(), mask.cuda(), max_size=2 ** 30, composite=False)
    mf = mask.expand_as(x).float().cuda()
    assert torch.equal(got, (x.cuda() * (1 - mf) + raw * mf).clamp(0, 1))
    model.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        model(x.cuda(), mask.cuda())
    model.eval()


def test_empty_mask_leaves_the_frames_unchanged(model):
    x, mask = R.case_input("c")
    out = model.infer(x.cuda(), torch.zeros_like(mask).cuda(), composite=True)
    assert torch.equal(out.cpu(), x)


def test_batch_call_and_stream_invariance(model):
    x, mask = R.case_input("c")
    xd, md = x.cuda(), mask.cuda()
    for composite in (False, True):
        both = model.infer(xd, md, composite=composite)
        taps = model.debug_tap("dec")
        for b in range(2):
            one = model.infer(xd[b:b + 1], md[b:b + 1], composite=composite)
            assert torch.equal(one[0], both[b]), (composite, b)
            assert torch.equal(model.debug_tap("dec")[0], taps[b])
        again = model.infer(xd, md, composite=composite)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            third = model.infer(xd, md, composite=composite)
        side.synchronize()
        assert torch.equal(both, again) and torch.equal(both, third)
    with torch.autocast(device_type="cuda"):                        # an ambient autocast is ignored
        fourth = model.infer(xd, md, composite=True)
    assert fourth.dtype == torch.float32 and torch.equal(fourth, both)


# ---- the EMA buffer --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("decay", [0.25, 0.5])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_buffer_step_against_float64(B, decay):
    from nunif_amd.stlizer.outpaint import buffer_step
    frames, coarse = R.buffer_case(B, clean_frame=1)
    reset = [j in (0, 2) for j in range(B)]
    g = torch.Generator().manual_seed(5)
    start = torch.rand(3, *frames.shape[2:], generator=g)
    buf = start.clone().cuda()
    got = buffer_step(frames.cuda(), coarse.cuda(), buf, reset, decay)
    want64, buf64 = R.buffer_step(frames, coarse, start, reset, decay, torch.float64)
    want32, buf32 = R.buffer_step(frames, coarse, start, reset, decay, torch.float32)
    check(f"buffer B{B} d{decay} frames", got, want32, want64)
    check(f"buffer B{B} d{decay} buffer", buf, buf32, buf64)
    if B > 1:
        assert torch.equal(got[1].cpu(), frames[1].clamp(0, 1)), "a frame without NaN only gets the clamp"
    zeroed, mask = buffer_step(frames.cuda())
    assert torch.equal(mask.cpu().bool(), torch.isnan(frames[:, 0:1]))
    assert torch.equal(zeroed.cpu(), torch.where(torch.isnan(frames), torch.zeros(()), frames))


def test_buffer_step_one_batch_of_five_equals_two_and_three():
    from nunif_amd.stlizer.outpaint import buffer_step
    frames, coarse = R.buffer_case(5)
    frames, coarse = frames.cuda(), coarse.cuda()
    reset = [True, False, True, False, False]
    b5 = torch.zeros(3, *frames.shape[2:], device="cuda")
    b23 = b5.clone()
    all5 = buffer_step(frames, coarse, b5, reset, 0.25)
    first = buffer_step(frames[:2], coarse[:2], b23, reset[:2], 0.25)
    second = buffer_step(frames[2:], coarse[2:], b23, reset[2:], 0.25)
    assert torch.equal(all5, torch.cat([first, second])) and torch.equal(b5, b23)


@pytest.mark.parametrize("buffer_decay", [0.6, 0.0])
def test_outpaint_border_over_seven_frames(model, sd, buffer_decay):
    """OutpaintBorder in batches of 3, 3, 1 on frames that the engine's own apply_transform warped out of NaN-padded frames,
    against the float64 restatement of multipass_pipeline.py:447-474 on those same warped frames (so both sides see one mask)."""
    from nunif_amd.nunif.utils.superpoint import apply_transform
    from nunif_amd.stlizer.outpaint import OutpaintBorder
    g = torch.Generator().manual_seed(77)
    H, W, pad = 48, 80, 8
    low = torch.rand(7, 3, 6, 9, generator=g)
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False).clamp(0, 1)
    xin = torch.nn.functional.pad(x, (pad,) * 4, value=math.nan).cuda()
    shifts = torch.tensor([[2.5 * math.sin(j), -1.75 * math.cos(j)] for j in range(7)])
    angles = torch.tensor([1.5 * math.sin(0.7 * j + 0.3) for j in range(7)])
    centers = torch.tensor([[W // 2 + pad, H // 2 + pad]] * 7, dtype=torch.float32)
    z = apply_transform(xin, shifts.cuda(), torch.ones(7).cuda(), angles.cuda(), centers.cuda(), padding_mode="border")
    nan = torch.isnan(z)
    assert nan.any() and not nan.all() and torch.equal(nan[:, 0], nan[:, 1])
    weights = [1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0]                  # frame 4 starts a scene: the buffer is reset there
    parts = [(0, 3), (3, 6), (6, 7)]
    border = OutpaintBorder(model, buffer_decay, fps=30.0)
    assert border.decay == (R.blend_weight(buffer_decay, 30.0) if buffer_decay > 0 else 0.0)
    got = torch.cat([border(z[a:b], weights[a:b]) for a, b in parts]).cpu()
    zc = z.cpu()
    batches, sw = [zc[a:b] for a, b in parts], [weights[a:b] for a, b in parts]
    want64 = torch.cat(R.border(sd, batches, sw, buffer_decay, 30.0, torch.float64))
    want32 = torch.cat(R.border(sd, batches, sw, buffer_decay, 30.0, torch.float32))
    assert got.shape == zc.shape and not torch.isnan(got).any()
    check(f"border decay {buffer_decay}", got, want32, want64)
    keep = ~nan.cpu()
    assert torch.equal(got[keep], zc[keep].clamp(0, 1)), "pixels the warp filled are only clamped"
    border.reset()
    assert border.buffer is None
    clean = x.cuda()[:2]
    assert torch.equal(border(clean, [1.0, 1.0]), clean), "frames without NaN come back unchanged"
