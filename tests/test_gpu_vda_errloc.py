"""The Video-Depth-Anything temporal modules on the HIP engine (csrc/depth_temporal.hip, ``run_tmod`` of depth_anything.hip) pinned per
pixel against float64: one module alone through ``debug_temporal`` (``nunif_hip_depth_anything_debug_temporal``), the cases of
``tests/vda_cases.py`` — every width in use (64, 128, 192, 256, 384, 768, 1024), both attention forms for C <= 384.

Module output: every pixel of every frame (cell (1, 1)) at A_SIDE 2.1 / B_SIDE 3.6; every tap per pixel and head (hd = C / 8
channels) at A_VDA_TAP 6.5 / B_VDA_TAP 30; tau = TAP_TAU_REL x the map's rms; the yardstick is the reference's own fp16 arithmetic over the
same stream (tests/errloc.py); the ``geglu`` tap's error has no component along tanh GELU - erf GELU (``vda_cases.gelu_form``).  The measured ratios are in profiles/vda_temporal_errloc.txt.
"""
import functools

import pytest
import torch

import errloc as E
import vda_cases as VC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def engine(enc):
    """One engine handle per encoder and process (the ViT-L handle takes longest to build)."""
    from nunif_amd.iw3.video_depth_anything_net import HipVideoDepthAnythingStreaming
    return HipVideoDepthAnythingStreaming(VC.state_dict(enc))


@pytest.fixture(scope="module")
def engines(hiplib):
    return engine


def run(net, module, x, batches, taps=True):
    """x [T, P, C] through ``debug_temporal`` from a new window, ``batches`` frames per call -> (out, taps) on the CPU."""
    net.reset_state()
    outs, tps, i = [], [], 0
    for n in batches:
        r = net.debug_temporal(module, x[i:i + n], taps=taps)
        y, t = r if taps else (r, {})
        outs.append(y.cpu())
        tps.append({k: v.cpu() for k, v in t.items()})
        i += n
    assert i == x.shape[0]
    return torch.cat(outs), {k: torch.cat([t[k] for t in tps]) for k in tps[0]}


def emitter(capsys):
    def emit(line):
        with capsys.disabled():
            print("\n" + line, end="")
    return emit


def _check_case(case, engines, monkeypatch, capsys):
    enc, module, row, form = case
    monkeypatch.setenv("NUNIF_VDA_TATTN", form)
    x, y64, ye, t64, te = VC.references(enc, module, row)
    y, taps = run(engines(enc), module, x, VC.ROWS[row][1])
    label = VC.case_id(case)
    emit = emitter(capsys)
    # print both lines before either asserts
    st = VC.stats(y, y64, ye, E.B_SIDE)
    emit(f"errloc {label} out: global {st['global']:.2f} worst {st['worst']:.2f} (err {st['_gmax']:.2e} noise {st['_nmax']:.2e})")
    failures = []
    try:
        VC.check_taps(taps, t64, te, VC.WIDTHS[enc][module], label, emit)
    except AssertionError as e:
        failures.append(str(e))
    try:
        VC.check_gelu_form(taps, t64, enc, module, label, emit)
    except AssertionError as e:
        failures.append(str(e))
    try:
        E.assert_localised(st, E.A_SIDE, E.B_SIDE, VC.tau_for(y64), label=label + " out")
    except AssertionError as e:
        failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", VC.VITS_CASES, ids=VC.case_id)
def test_vits_temporal_module_per_pixel_vs_float64(case, engines, monkeypatch, capsys):
    _check_case(case, engines, monkeypatch, capsys)


@pytest.mark.parametrize("case", VC.WIDE_CASES, ids=VC.case_id)
def test_wide_temporal_module_per_pixel_vs_float64(case, engines, monkeypatch, capsys):
    """C = 128, 256, 768, 1024 (and ViT-B's 384): the widths of VDA_Stream_B / _L."""
    _check_case(case, engines, monkeypatch, capsys)


@pytest.mark.parametrize("enc,module", [("vits", 0), ("vits", 2), ("vitb", 1)])
def test_reset_state_after_40_frames_gives_a_fresh_handles_bits(enc, module, engines):
    """40 frames (the ring is full of another stream's K0 / V0 and ``start`` has moved), ``reset_state``, then the first 3 frames of
    the 1x5 row: ``torch.equal`` to the first run on the new window — stale slots are never read."""
    net = engines(enc)
    x = VC.references(enc, module, "1x5")[0]
    fresh, _ = run(net, module, x[:3], (1, 1, 1), taps=False)
    other = VC.maps(x.shape[2], 1, 5, 40, 77, 3.0)
    run(net, module, other, (1,) * 40, taps=False)
    again, _ = run(net, module, x[:3], (1, 1, 1), taps=False)
    assert torch.equal(fresh, again)
    # ... and the history matters: frame 2 alone is not frame 2 after frames 0, 1
    alone, _ = run(net, module, x[2:3], (1,), taps=False)
    assert float((alone[0] - fresh[2]).abs().max()) > 0.02 * float(fresh[2].std())


def test_a_changed_pixel_count_starts_a_new_window(engines, capsys):
    """3 frames at P = 33, then the 1x1 row (P = 1) WITHOUT ``reset_state``: the bound against float64 of a stream that starts there."""
    enc, module = "vits", 0
    net = engines(enc)
    run(net, module, VC.references(enc, module, "3x11")[0], (3,), taps=False)
    x, y64, ye, _, _ = VC.references(enc, module, "1x1")
    y = torch.cat([net.debug_temporal(module, x[i:i + 1]).cpu() for i in range(3)])
    VC.check_output(y, y64, ye, "vits-m0 1x1 after 3x11", emitter(capsys))
    # another module on the same handle starts a new window as well
    x2, y642, ye2, _, _ = VC.references(enc, 2, "1x1")
    y2 = torch.cat([net.debug_temporal(2, x2[i:i + 1]).cpu() for i in range(3)])
    VC.check_output(y2, y642, ye2, "vits-m2 1x1 after m0", emitter(capsys))
