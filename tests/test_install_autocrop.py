"""``nunif_amd.install()`` over the LIVE reference, --autocrop: the three names of ``nunif.utils.autocrop`` are in ``PATCHES``;
after ``install()`` the reference's ``iw3.utils.AutoCrop`` (bound by name, iw3/utils.py:26) is the engine's class, and
``uninstall()`` restores it.  And the host-tensor route while installed: a CPU frame goes through the reference's own class and
gives what tests/golden/autocrop.npz records."""
import os
import sys

import numpy as np
import pytest
import torch

import autocrop_cases as C
from conftest import GOLDEN

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")

ENTRIES = [("nunif.utils.autocrop", "AutoCropDetector"), ("nunif.utils.autocrop", "AutoCrop"),
           ("nunif.utils.autocrop", "autocrop_analyze_video")]


@pytest.fixture()
def reference():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    import iw3.utils    # noqa: F401
    import nunif.utils.autocrop as ref
    yield inst, {name: getattr(ref, name) for _, name in ENTRIES}
    if inst.is_installed():
        inst.uninstall()


def test_the_three_entries_are_in_patches():
    import nunif_amd.install as inst
    for e in ENTRIES:
        assert e in inst.PATCHES


def test_install_rebinds_the_consumer_and_uninstall_restores(reference):
    inst, originals = reference
    import nunif_amd.nunif.utils.autocrop as ours
    report = inst.install()
    ref_mod, consumer = sys.modules["nunif.utils.autocrop"], sys.modules["iw3.utils"]
    for _, name in ENTRIES:
        assert getattr(ref_mod, name) is getattr(ours, name)
        assert report["patched"][f"nunif.utils.autocrop.{name}"] >= 1
    assert consumer.AutoCrop is ours.AutoCrop
    assert report["patched"]["nunif.utils.autocrop.AutoCrop"] >= 2          # the defining module and iw3.utils
    assert inst.original("nunif.utils.autocrop", "AutoCrop") is originals["AutoCrop"]
    inst.uninstall()
    for _, name in ENTRIES:
        assert getattr(ref_mod, name) is originals[name]
    assert consumer.AutoCrop is originals["AutoCrop"]


def test_host_tensors_go_through_the_reference_while_installed(reference):
    inst, originals = reference
    import nunif_amd.nunif.utils.autocrop as ours
    golden = dict(np.load(os.path.join(GOLDEN, "autocrop.npz")))
    enc = lambda sl: C.enc_slice(sl[0]) + C.enc_slice(sl[1])      # noqa: E731
    inst.install()
    for mode in C.MODES:
        kind = mode.split("_")[0]
        x = C.case_frame("s37x67", kind)
        for mod in C.MODS:
            key = f"s37x67/{mode}/{mod}"
            ac = ours.AutoCrop.from_image(x, mode=mode, mod=mod, pad_value=0.5)
            assert enc(ac.get_slice()) == golden[key + "/slices"].tolist(), key
            assert list(ac.get_pad()) == golden[key + "/pad"].tolist() and list(ac.get_crop()) == golden[key + "/crop"].tolist()
            cropped = ac.crop(x)
            assert torch.equal(cropped, x[:, ac.slice_h, ac.slice_w])
            assert torch.equal(ac.uncrop(cropped), torch.nn.functional.pad(cropped, ac.get_pad(), value=0.5))
            det = ours.AutoCropDetector(mode=mode, mod=mod)
            seq = C.seq_frames(kind)
            det.update(seq[:7])
            for f in seq[7:]:
                det.update(f)
            assert det.frame_count == C.SEQ_FRAMES and enc(det.get_crop()) == golden[f"seq/{mode}/{mod}/slices"].tolist()
            if mode == kind and mod == 1:
                assert det.border_count_tb.device.type == "cpu"
                assert np.array_equal(det.border_count_tb.flatten().numpy(), golden[f"seq/{kind}/count_tb"])
                assert np.array_equal(det.border_count_lr.flatten().numpy(), golden[f"seq/{kind}/count_lr"])
        black = kind == "black"
        assert np.array_equal(ours.AutoCropDetector.detect_tb(x, black_only=black).flatten().numpy(),
                              golden[f"s37x67/{kind}/mask_tb"].astype(bool))
    inst.uninstall()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ours.AutoCrop.from_image(C.case_frame("s37x67", "black"))
