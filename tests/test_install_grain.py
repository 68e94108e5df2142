"""``nunif_amd.install()`` over the LIVE reference, the film-grain and waifu2x-video names: after ``install()``
``waifu2x.ui_utils`` holds the engine's ``rgb_noise_like``, ``apply_rgb_noise`` and ``process_video``
(``waifu2x/ui_utils.py:15,104``), their signatures equal the reference's, ``uninstall()`` restores them.  Nothing is computed."""
import inspect
import sys

import pytest

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")

NAMES = [("nunif.utils.rgb_noise", "rgb_noise_like"), ("nunif.utils.rgb_noise", "apply_rgb_noise"),
         ("waifu2x.ui_utils", "process_video")]


@pytest.fixture()
def reference():
    refstub.install()
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    import nunif.utils.rgb_noise    # noqa: F401
    import waifu2x.ui_utils         # noqa: F401
    originals = {(m, a): getattr(sys.modules[m], a) for m, a in NAMES}
    yield inst, originals
    if inst.is_installed():
        inst.uninstall()


def test_signatures_equal_the_live_reference(reference):
    import importlib
    _, originals = reference
    for (mod, attr), orig in originals.items():
        ours = getattr(importlib.import_module("nunif_amd." + mod), attr)
        assert inspect.signature(orig) == inspect.signature(ours), (mod, attr)


def test_install_rebinds_grain_and_process_video_and_uninstall_restores(reference):
    inst, originals = reference
    import nunif_amd.nunif.utils.rgb_noise as R
    import nunif_amd.waifu2x.ui_utils as U
    for entry in NAMES:
        assert entry in inst.PATCHES
    assert inst.original("waifu2x.ui_utils", "process_video") is None           # nothing installed yet
    report = inst.install()
    ui, rn = sys.modules["waifu2x.ui_utils"], sys.modules["nunif.utils.rgb_noise"]
    assert rn.rgb_noise_like is R.rgb_noise_like and rn.apply_rgb_noise is R.apply_rgb_noise
    assert ui.rgb_noise_like is R.rgb_noise_like and ui.apply_rgb_noise is R.apply_rgb_noise      # ui_utils.py:15 copies
    assert ui.process_video is U.process_video
    assert report["patched"]["nunif.utils.rgb_noise.rgb_noise_like"] >= 2
    assert report["patched"]["nunif.utils.rgb_noise.apply_rgb_noise"] >= 2
    assert report["patched"]["waifu2x.ui_utils.process_video"] >= 1
    # the engine's process_video reaches the reference's own function for everything but the frame callback
    assert inst.original("waifu2x.ui_utils", "process_video") is originals[("waifu2x.ui_utils", "process_video")]
    inst.uninstall()
    for (mod, attr), orig in originals.items():
        assert getattr(sys.modules[mod], attr) is orig
    assert ui.rgb_noise_like is originals[("nunif.utils.rgb_noise", "rgb_noise_like")]


def test_process_video_runs_the_references_code_around_the_engines_callbacks(reference, tmp_path):
    """``--resume`` with the output present returns before any frame is touched (ui_utils.py:186-187), through the engine's
    entry: output naming and the early return are the reference's code.  Then the full path with a recording stand-in for
    ``VU.process_video``: it receives the stream's callbacks, not the closure the reference built."""
    import types
    inst, _ = reference
    inst.install()
    ui = sys.modules["waifu2x.ui_utils"]
    out = tmp_path / "out.mp4"
    out.write_bytes(b"x")
    args = types.SimpleNamespace(pix_fmt="yuv420p", compile=False, resume=True, yes=True, state={"device": "cuda:0"})
    assert ui.process_video(None, "in.mp4", str(out), args) is None and out.read_bytes() == b"x"

    import nunif_amd.waifu2x.ui_utils as U
    seen = {}

    class FakeStream:
        def __init__(self, ctx, a, device=None, use_16bit=None):
            seen["device"], seen["use_16bit"] = device, use_16bit

        def av_callback(self, to_frame):
            return "engine-frame-callback"

        def test_callback(self, to_frame):
            return "engine-test-callback"

    class FakeVU:
        to_frame = staticmethod(lambda x: x)
        pix_fmt_requires_16bit = staticmethod(lambda p: False)

        @staticmethod
        def process_video(input_path, output_path, **kw):
            seen.update(kw, input_path=input_path, output_path=output_path)

    orig = inst.original("waifu2x.ui_utils", "process_video")
    saved_vu, saved_stream = orig.__globals__["VU"], U.Waifu2xVideoStream
    orig.__globals__["VU"], U.Waifu2xVideoStream = FakeVU, FakeStream
    try:
        args = types.SimpleNamespace(pix_fmt="yuv420p", compile=False, resume=False, yes=True, vf="", start_time=None,
                                     end_time=None, state={"device": "cuda:0", "stop_event": None, "tqdm_fn": None})
        ui.process_video(None, "in.mp4", str(tmp_path / "new" / "o.mp4"), args)
    finally:
        orig.__globals__["VU"], U.Waifu2xVideoStream = saved_vu, saved_stream
    assert seen["frame_callback"] == "engine-frame-callback" and seen["test_callback"] == "engine-test-callback"
    assert seen["use_16bit"] is False
    assert seen["device"] == "cuda:0" and seen["output_path"].endswith("o.mp4") and callable(seen["config_callback"])


def test_process_video_refuses_a_reference_that_stopped_calling_vu_process_video(reference):
    """The engine's process_video substitutes ``VU`` in the reference function's globals; a reference that no longer spells its
    call ``VU.process_video(..., frame_callback=...)`` must fail loudly instead of running its torch callback again."""
    import types
    inst, _ = reference
    inst.install()
    ui = sys.modules["waifu2x.ui_utils"]
    orig = inst.original("waifu2x.ui_utils", "process_video")
    args = types.SimpleNamespace(pix_fmt="yuv420p", compile=False, resume=False, yes=True, state={"device": "cuda:0"})
    saved = orig.__globals__.pop("VU")
    try:
        with pytest.raises(RuntimeError, match="does not fit this reference"):
            ui.process_video(None, "in.mp4", "out.mp4", args)
    finally:
        orig.__globals__["VU"] = saved
    from nunif_amd.waifu2x.ui_utils import _VideoUtilsProxy
    with pytest.raises(RuntimeError, match="does not fit this reference"):
        _VideoUtilsProxy(saved, lambda: None).process_video("in.mp4", "out.mp4")
