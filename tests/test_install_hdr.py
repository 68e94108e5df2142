"""``nunif_amd.install()`` and the HDR -> SDR tone mapping: ``nunif.utils.video.hdr2sdr`` is rebound (the reference's
``process_video`` finds it as a global of its own module) and restored; with a host ``device`` the engine's function hands the call
to the reference's own while installed, and raises when there is nothing to hand it to."""
import os
import sys

import numpy as np
import pytest

import hdr_ref as R
from conftest import GOLDEN
from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="/root/reference is not mounted here")
ENTRY = ("nunif.utils.video", "hdr2sdr")


@pytest.fixture()
def inst():
    R.reference_hdr2sdr_recording()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    yield inst
    inst.uninstall()


def test_rebinding_and_restoring(inst):
    from nunif_amd.nunif.utils.video import hdr2sdr
    assert ENTRY in inst.PATCHES
    VU = sys.modules["nunif.utils.video"]
    original = VU.hdr2sdr
    assert original is not hdr2sdr and original.__module__ == "nunif.utils.video"
    report = inst.install()
    assert report["patched"]["nunif.utils.video.hdr2sdr"] >= 1
    assert VU.hdr2sdr is hdr2sdr and VU.process_video.__globals__["hdr2sdr"] is hdr2sdr
    assert inst.original(*ENTRY) is original
    inst.uninstall()
    assert VU.hdr2sdr is original


def test_host_device_reaches_the_reference_while_installed(inst):
    from nunif_amd.nunif.utils.video import hdr2sdr
    fixture = np.load(os.path.join(GOLDEN, "hdr2sdr.npz"))
    inst.install()
    for name in ("ramp_pq_bt709", "noise_hlg_bt601_gain05"):
        inp, trc, cs, params = R.CASES[name]
        frame = R.FakeFrame(R.make_input(inp))
        out = hdr2sdr(frame, trc, cs, device="cpu", **params)
        assert isinstance(out, R.RecordingVideoFrame) and np.array_equal(out.array, fixture[name])
        assert (out.pts, out.dts, out.time_base, out.opaque) == (frame.pts, frame.dts, frame.time_base, frame.opaque)


def test_host_device_raises_when_not_installed(inst):
    from nunif_amd.nunif.utils.video import hdr2sdr
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr2sdr(R.FakeFrame(R.make_input("dark")), R.PQ, "bt709", device="cpu")
    with pytest.raises(AssertionError):
        hdr2sdr(R.FakeFrame(R.make_input("dark")), 1, "bt709", device="cpu")
