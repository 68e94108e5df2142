"""The light inpaint nets (``inpaint.light_inpaint_v1``, ``inpaint.light_video_inpaint_v1`` small / medium / large) held window by
window and tap by tap to a float64 oracle.

``csrc/light_inpaint.hip`` goes wrong per window (the zero-padded map of the shifted blocks, the per-window transposed copy of the
token mixing, the gate through LDS), per conv patch (three 3 x 3 kernels chosen by channel and patch count), per token (the mask
rule, the LayerNorms) and per frame (the 12 x 12 temporal mixing).  ``tests/errloc.py``: per image, max|y - y64| <= A max|emu - y64|
and, in every (64, 64) and (32, 128) cell of the output (aligned and shifted by half a cell), region_max(y - y64) <= B region_max(emu -
y64) + tau, with the project's constants for clamped outputs (A_OUT 2.5, B_OUT 3.75, TAU_OUT 5e-4); the fp16 maps of
``nunif_hip_light_inpaint_debug_taps`` the same way per window and conv patch of their level with A_TAP 3.5, B_TAP 5.5 and
tau = 2e-3 x the map's rms, over all channels and per 16-channel group; the masks exactly (``hard``, ``mtok``) or to fp32 rounding
(``soft``).  emu = the reference's own fp16-autocast arithmetic on the same pre-processed input.  Cases and why:
``tests/inpaint_cases.py``; what the check catches: ``test_errloc_inpaint.py``.  The figures measured on an MI355X are in
``profiles/light_inpaint_errloc.txt``.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import errloc as E
import inpaint_cases as S
from oracle import dilation as OD
from oracle import light_inpaint as OL

pytestmark = pytest.mark.gpu


def new_model(net, regime="benign"):
    from nunif_amd.nunif.models import create_model
    from nunif_amd.iw3 import models  # noqa: F401  (registers the factories)
    m = create_model(net).eval()
    m.load_state_dict(S.state_dict(net, regime), strict=True)
    return m.to("cuda:0")


make_model = functools.lru_cache(maxsize=None)(new_model)


def run(case, model=None, x=None, mask=None):
    """The engine's output of a case on the CPU, in the frame the net ran in (mirrored back when the case flips)."""
    net, shape, flip, regime = case[:4]
    ref = S.references(case)
    x, mask = ref["x"] if x is None else x, ref["mask"] if mask is None else mask
    y = (model or make_model(net, regime)).infer(x.to("cuda:0"), mask.to("cuda:0"), mirror_x=flip, **ref["pre"]).cpu()
    return torch.flip(y, (3,)) if flip else y


def check_output(y, case, label, capsys):
    ref = S.references(case)
    assert y.shape == ref["y64"].shape and y.dtype == torch.float32, (label, y.shape, y.dtype)
    st = S.output_stats(y, ref, case[0])
    with capsys.disabled():
        print(f"\nerrloc {label}: global {st['global']:.2f} worst {st['worst']:.2f} (err {st['_gmax']:.2e} noise {st['_nmax']:.2e}) "
              f"{E.summary(st)['bands']}")
    return E.assert_localised(st, E.A_OUT, E.B_OUT, E.TAU_OUT, label=label)


# ---- the outputs, window by window --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_output_window_by_window(hiplib, capsys, case):
    if case == S.DMA_CASE:
        assert S.conv_patches(case[1]) > 24, "the level-1 GLU conv no longer reaches the LDS-DMA kernel"
    y = run(case)
    ref = S.references(case)
    keep = ~ref["taps64"]["soft"].expand_as(y).gt(0)                    # outside the soft mask: the input, bit for bit
    xm = torch.flip(ref["x"], (3,)) if case[2] else ref["x"]
    assert torch.equal(y[keep], xm[keep])
    check_output(y, case, S.case_id(case), capsys)


# ---- the taps -----------------------------------------------------------------------------------------------------------------------
def _n_iter(n, w, base_width):
    return 0 if n <= 0 else (max(round(w / base_width * n), 1) if base_width is not None else n)


def engine_taps(case):
    net, shape, flip, regime = case[:4]
    ref = S.references(case)
    pre, w = ref["pre"], shape[2]
    eng = make_model(net, regime).engine()
    out, taps = eng.debug_taps(ref["x"].to("cuda:0"), ref["mask"].to("cuda:0").contiguous().view(torch.uint8), pre.get("closing", False),
                               _n_iter(pre.get("inner_dilation", 0), w, pre.get("base_width")),
                               _n_iter(pre.get("outer_dilation", 0), w, pre.get("base_width")), mirror_x=flip)
    return out.cpu(), {k: v.cpu() for k, v in taps.items()}


def blur64(hard):
    """clamp(gaussian15(hard) + hard) in float64 (``oracle.light_inpaint.mask_blur`` with a float64 kernel)."""
    k = 15
    sigma, half = k * 0.15 + 0.35, (k - 1) * 0.5
    g = torch.exp(-0.5 * (torch.linspace(-half, half, steps=k, dtype=torch.float64) / sigma).pow(2))
    g = g / g.sum()
    m = F.pad(hard.double(), (k // 2,) * 4, mode="replicate")
    m = F.conv2d(F.conv2d(m, g.view(1, 1, 1, k)), g.view(1, 1, k, 1))
    return torch.clamp(m + hard.double(), 0, 1)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_taps_window_by_window(hiplib, capsys, case):
    check_taps(case, S.case_id(case), capsys)


def check_taps(case, label, capsys):
    net, shape, flip = case[:3]
    ref = S.references(case)
    t64, te = ref["taps64"], ref["tapse"]
    out, taps = engine_taps(case)
    assert torch.equal(torch.flip(out, (3,)) if flip else out, run(case)), "infer with taps != infer without"
    assert set(taps) == set(t64)
    assert torch.equal(taps["hard"], t64["hard"]) and torch.equal(taps["mtok"], t64["mtok"])
    s64 = blur64(t64["hard"])
    e_ref, e_hip = float((t64["soft"].double() - s64).abs().max()), float((taps["soft"].double() - s64).abs().max())
    lines = [f"soft: e_hip {e_hip:.2e} e_ref {e_ref:.2e}"]
    assert e_hip <= 2.2 * e_ref + 2.0 ** -23, (e_hip, e_ref)
    failures = []
    for name, level in S.tap_names(net):
        t = taps[name].float()
        assert t.shape == t64[name].shape, (name, t.shape, t64[name].shape)
        for group in (None, 16):
            st = S.tap_stats(t, t64[name], te[name], net, level, group)
            lines.append(f"{name}{'' if group is None else ' /16ch'}: global {st['global']:.2f} worst {st['worst']:.2f}")
            try:
                E.assert_localised(st, E.A_TAP, E.B_TAP, S.tau_for(t64[name]), label=f"{S.case_id(case)} {name} group {group}")
            except AssertionError as e:
                failures.append(str(e))
    with capsys.disabled():
        print(f"\ntaps {label}: " + "; ".join(lines))
    assert not failures, "first failing tap:\n" + failures[0]


# ---- invariants -------------------------------------------------------------------------------------------------------------------
def test_image_b_of_a_batch_equals_the_image_alone(hiplib):
    for case in (S.BATCH, S.IMAGE_CASES[1]):
        ref = S.references(case)
        whole = run(case)
        for b in range(case[1][0]):
            one = run(case, x=ref["x"][b:b + 1], mask=ref["mask"][b:b + 1])
            assert torch.equal(whole[b:b + 1], one), f"{S.case_id(case)}: image {b} of the batch != the image alone"


@pytest.mark.parametrize("case", [S.MAIN_CASE, S.MAIN_VIDEO_CASE], ids=S.case_id)
def test_two_calls_and_two_streams_give_equal_bytes(hiplib, case):
    base = run(case)
    assert torch.equal(base, run(case))
    torch.cuda.synchronize()
    for _ in range(2):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            got = run(case)
        stream.synchronize()
        assert torch.equal(base, got), "another stream gave other bytes"


def test_small_call_after_the_largest_equals_a_fresh_model(hiplib):
    """The workspaces stay allocated from call to call (``DeviceBuf::ensure``): nothing of the large call shows in the small one."""
    small = S.IMAGE_CASES[0]
    used = new_model(S.IMAGE)
    run(S.BIGGEST, model=used)
    assert torch.equal(run(small, model=used), run(small, model=new_model(S.IMAGE)))
    used = new_model(S.SMALL)
    run(S.VIDEO_CASES[1], model=used)
    assert torch.equal(run(S.MAIN_VIDEO_CASE, model=used), run(S.MAIN_VIDEO_CASE, model=new_model(S.SMALL)))


@pytest.mark.parametrize("switch", S.SWITCHES, ids=lambda s: f"{s[0]}={s[1]}")
@pytest.mark.parametrize("case", [S.MAIN_CASE, S.MAIN_VIDEO_CASE], ids=S.case_id)
def test_switch_output_window_by_window(hiplib, capsys, monkeypatch, case, switch):
    """The other kernel choices (read per call), held to the same bound as the default, not to a PSNR against it."""
    base = run(case)
    monkeypatch.setenv(*switch)
    y = run(case)
    with capsys.disabled():
        print(f"\n{switch[0]}={switch[1]}: {'the same bytes as' if torch.equal(y, base) else 'other bytes than'} the default")
    check_output(y, case, f"{S.case_id(case)} {switch[0]}={switch[1]}", capsys)


def test_largest_map_on_the_resident_k192_gemm(hiplib, capsys, monkeypatch):
    """At 65 536 level-1 tokens NUNIF_GEMM_BIG_M=1 moves the level-1 proj_out (K = 192) onto the resident-weight GEMM, the form the
    4K frames use (swin_kernels.hip ``launch_gemm_t``: 32 768 rows at least); at the switches' small shapes it cannot.  Outputs and taps."""
    case = S.BIGGEST
    base = run(case)
    monkeypatch.setenv("NUNIF_GEMM_BIG_M", "1")
    y = run(case)
    with capsys.disabled():
        print(f"\nNUNIF_GEMM_BIG_M=1 at {S.case_id(case)}: {'the same bytes as' if torch.equal(y, base) else 'other bytes than'} the default")
    check_output(y, case, f"{S.case_id(case)} NUNIF_GEMM_BIG_M=1", capsys)
    check_taps(case, f"{S.case_id(case)} NUNIF_GEMM_BIG_M=1", capsys)


# ---- neighbouring entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["plain", "close"])
def test_video_infer_pads_seven_frames_to_twelve(hiplib, capsys, pre):
    case = S.MAIN_VIDEO_CASE if pre == "plain" else S.VIDEO_CASES[2]
    ref = S.references(case)
    opts = ref["pre"]
    x, mask = ref["x"][:7], ref["mask"][:7]
    y = make_model(S.SMALL).infer(x.to("cuda:0"), mask.to("cuda:0"), **opts).cpu()
    b1 = (12 - 7) // 2
    pad = lambda t: torch.cat([t[0:1]] * b1 + [t] + [t[-1:]] * (5 - b1))            # noqa: E731  (video_infer :141-150)
    E.set_threads()
    sd = S.state_dict(S.SMALL)
    y64 = E.oracle64(sd, pad(x), S.SMALL, mask=pad(mask), pre=opts)[b1:b1 + 7]
    ye = E.emulated(sd, pad(x), S.SMALL, mask=pad(mask), pre=opts)[b1:b1 + 7]
    assert y.shape == y64.shape and (OL.video_infer(sd, x, mask, **opts) - y64).abs().max().item() < 1e-4
    st = E.localised_stats(y, y64, ye, E.cells_for(S.SMALL), E.B_OUT, E.TAU_OUT)
    with capsys.disabled():
        print(f"\nerrloc small 7 of 12 frames {pre}: global {st['global']:.2f} worst {st['worst']:.2f}")
    E.assert_localised(st, E.A_OUT, E.B_OUT, E.TAU_OUT, label="7 frames")


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 7), (1, 5, 1), (1, 33, 65), (2, 64, 64)], ids=str)
def test_mask_morphology_equals_the_oracle(hiplib, shape):
    """``nunif_hip_mask_morphology`` at the edges ``test_hole_mask.py`` (one 48 x 74 mask, 1 or 2 iterations) does not reach: single
    rows / columns / pixels, n = 0 and n = 16."""
    from nunif_amd.iw3 import _ops
    b, h, w = shape
    m = (torch.rand(b, 1, h, w, generator=torch.Generator().manual_seed(h * 100 + w)) < 0.3).float()
    md = m.to("cuda:0")
    for n in (0, 1, 16):
        want = {0: m, 1: m, 2: OD.closing(m, n_iter=n), 3: OD.mask_closing(m, n_iter=n)}
        for _ in range(n):
            want[0], want[1] = OD.dilate(want[0]), OD.erode(want[1])
        for op in range(4):
            assert torch.equal(_ops.mask_morphology(md, op, n).cpu(), want[op]), (shape, op, n)
        for n_b in (0, 1, 16):
            ref = OD.dilate_outer(OD.dilate_inner(m, n), n_b)
            assert torch.equal(_ops.mask_morphology(md, 4, n, n_b).cpu(), ref), (shape, 4, n, n_b)
