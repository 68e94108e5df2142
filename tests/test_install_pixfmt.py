"""``nunif_amd.install()`` and the two pixel-format conversions of the video loop: ``nunif.utils.video.configure_colorspace`` is
rebound (the reference's ``process_video`` finds it as a global of its own module) and restored.  The engine's function runs the
LIVE reference's own first and takes the conversions over only for planar formats on both ends, a known source matrix and range
and a frame callback that declared itself the engine's; in every other case the state is what the reference built.

Streams and codec contexts are ``SimpleNamespace`` stand-ins.  Where the reference imports over the stubbed PyAV its two enums are
inert placeholders, so the test gives the reference module integer enums with libav's values (AVCOL_RANGE_*, AVCOL_SPC_*)."""
import enum
import sys
from types import SimpleNamespace as NS

import pytest

from oracle import refstub

pytestmark = pytest.mark.skipif(not refstub.reference_available(), reason="the reference checkout is not mounted here")
ENTRY = ("nunif.utils.video", "configure_colorspace")
UNSPEC = 2          # AVCOL_SPC_UNSPECIFIED


class ColorRange(enum.IntEnum):
    UNSPECIFIED, MPEG, JPEG = 0, 1, 2


class Colorspace(enum.IntEnum):
    ITU709, ITU601 = 1, 5


@pytest.fixture()
def live(monkeypatch):
    refstub.install()
    try:
        import nunif.utils.video as VU
    except Exception as e:                                   # a reference whose module cannot import PyAV
        pytest.skip(f"the reference's nunif.utils.video does not import here: {e!r}")
    if getattr(sys.modules.get("av"), "__version__", "") == "0.0.0+stub":
        monkeypatch.setattr(VU, "ColorRange", ColorRange)
        monkeypatch.setattr(VU, "Colorspace", Colorspace)
        monkeypatch.setattr(VU, "KNOWN_COLORSPACES", {1, 5, 6, 7, 9})
    import nunif_amd.install as inst
    if inst.is_installed():
        inst.uninstall()
    original = VU.configure_colorspace
    inst.install()
    yield inst, VU, original
    inst.uninstall()


def source(pix_fmt="yuv420p", height=1080, space=1, color_range=1, trc=1, bits=8):
    return NS(pix_fmt=pix_fmt, height=height, format=NS(components=[NS(bits=bits)]),
              codec_context=NS(color_range=color_range, colorspace=space, color_trc=trc, color_primaries=space))


def target():
    return NS(codec_context=NS(color_range=None, colorspace=None, color_trc=None, color_primaries=None))


def run(VU, fn, src, pix_fmt="yuv420p", colorspace="bt709-tv", declare=True, vf="", turns=0, out=True):
    from nunif_amd.nunif.utils.video import declare_engine_callback
    config = VU.VideoOutputConfig(pix_fmt=pix_fmt, colorspace=colorspace)
    if declare:
        declare_engine_callback(config, vf=vf, turns=turns)
    dst = target() if out else None
    fn(dst, src, config)
    return config, dst


def is_identity(f):
    token = NS(reformat=lambda **kw: kw)
    return f(token) is token


# name: (source, config pix_fmt, --colorspace) -> the pix_fmt the reference settles on and the recorded plan.  ``out_format`` is that
# settled NAME (a yuvj* alias at 8-bit full range): the encoder is opened with it (video.py:1018), the returned frames must carry it
CASES = {
    "bt709_limited_to_bt709_limited": (
        dict(), "yuv420p", "bt709-tv", "yuv420p",
        dict(in_format="yuv420p", in_matrix="bt709", in_full_range=False,
             out_format="yuv420p", out_matrix="bt709", out_full_range=False)),
    "bt601_guessed_to_bt709_full": (        # no tags, 480 rows: guess_colorspace says ITU601, guess_color_range MPEG
        dict(height=480, space=UNSPEC, color_range=0), "yuv420p", "bt709-pc", "yuvj420p",
        dict(in_format="yuv420p", in_matrix="bt601", in_full_range=False,
             out_format="yuvj420p", out_matrix="bt709", out_full_range=True)),
    "yuvj444p_bt601_copy": (
        dict(pix_fmt="yuvj444p", space=6, color_range=2), "yuv444p", "auto", "yuvj444p",
        dict(in_format="yuv444p", in_matrix="bt601", in_full_range=True,
             out_format="yuvj444p", out_matrix="bt601", out_full_range=True)),
    "yuv420p10le_bt2020_copy": (
        dict(pix_fmt="yuv420p10le", space=9, color_range=1, bits=10), "yuv420p10le", "copy", "yuv420p10le",
        dict(in_format="yuv420p10le", in_matrix="bt2020", in_full_range=False,
             out_format="yuv420p10le", out_matrix="bt2020", out_full_range=False)),
    "yuv420p10le_to_8bit_bt709": (
        dict(pix_fmt="yuv420p10le", space=1, color_range=1, bits=10), "yuv420p", "bt709", "yuv420p",
        dict(in_format="yuv420p10le", in_matrix="bt709", in_full_range=False,
             out_format="yuv420p", out_matrix="bt709", out_full_range=False)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_records_matrix_and_range_and_takes_both_conversions(live, name):
    inst, VU, original = live
    src_kw, pix_fmt, colorspace, settled, plan = CASES[name]
    config, dst = run(VU, VU.configure_colorspace, source(**src_kw), pix_fmt, colorspace)
    assert config.state["engine_pixfmt"] == plan and plan["out_format"] == config.pix_fmt
    assert config.state["rgb24_options"] == {} and is_identity(config.state["reformatter"])
    # everything else is the reference's: the replaced pix_fmt, the encoder's tags, its own bookkeeping
    ref_config, ref_dst = run(VU, original, source(**src_kw), pix_fmt, colorspace)
    assert config.pix_fmt == ref_config.pix_fmt == settled
    assert vars(dst.codec_context) == vars(ref_dst.codec_context)
    for key in ("source_color_range", "output_colorspace"):
        assert config.state[key] == ref_config.state[key]
    assert ref_config.state["rgb24_options"] and not is_identity(ref_config.state["reformatter"])


FALLBACKS = {   # name: keyword arguments of run() for which the state stays exactly the reference's
    "rgb24_output": dict(src=dict(), pix_fmt="rgb24"),
    "gbrp16le_output": dict(src=dict(), pix_fmt="gbrp16le"),
    "yuv422p_output": dict(src=dict(), pix_fmt="yuv422p"),
    "colorspace_unspecified": dict(src=dict(), colorspace="unspecified"),
    "software_vf": dict(src=dict(), vf="format=rgb24,hflip"),
    "quarter_turn": dict(src=dict(), turns=1),
    "the_references_own_callback": dict(src=dict(), declare=False),
    "source_format_outside_the_three": dict(src=dict(pix_fmt="yuv422p")),
    "source_matrix_outside_the_three": dict(src=dict(space=7)),
    "hdr_source_goes_through_hdr2sdr": dict(src=dict(pix_fmt="yuv420p10le", space=9, trc=16, bits=10)),
    "hook_without_an_output_stream": dict(src=dict(), out=False),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_every_other_case_keeps_the_references_state(live, name):
    inst, VU, original = live
    kw = dict(FALLBACKS[name])
    src_kw = kw.pop("src")
    config, dst = run(VU, VU.configure_colorspace, source(**src_kw), **kw)
    ref_config, ref_dst = run(VU, original, source(**src_kw), **kw)
    assert "engine_pixfmt" not in config.state
    assert set(config.state) == set(ref_config.state)
    assert config.pix_fmt == ref_config.pix_fmt
    assert config.state["rgb24_options"] == ref_config.state["rgb24_options"]
    for key in ("source_color_range", "output_colorspace"):
        assert config.state[key] == ref_config.state[key]
    ours, refs = config.state["reformatter"], ref_config.state["reformatter"]
    assert ours.__code__ is refs.__code__ and ours.__module__ == "nunif.utils.video"      # the reference's own lambda
    if dst is not None:
        assert vars(dst.codec_context) == vars(ref_dst.codec_context)


def test_an_unknown_source_range_is_a_fall_back():
    """``guess_rgb24_options`` answers ``{}`` for a source whose range is unknown (video.py:639-640); the reference's own function
    does not get through that case (:794 indexes the empty dict), so the rule is checked where the engine applies it."""
    from nunif_amd.nunif.utils.video import ENGINE_CALLBACK, _engine_pixfmt
    config = NS(pix_fmt="yuv420p", colorspace="bt709-tv", state={ENGINE_CALLBACK: True, "rgb24_options": {}})
    dst = target()
    dst.codec_context.color_range = 1
    assert _engine_pixfmt(dst, source(), config) is None
    config.state["rgb24_options"] = dict(format="rgb24", src_color_range=1, dst_color_range=2, src_colorspace=1, dst_colorspace=1)
    assert _engine_pixfmt(dst, source(), config) is not None


def test_a_second_run_forgets_the_first_plan(live):
    inst, VU, original = live
    from nunif_amd.nunif.utils.video import declare_engine_callback
    config, _ = run(VU, VU.configure_colorspace, source())
    assert "engine_pixfmt" in config.state
    assert declare_engine_callback(config, vf="hflip") is False
    VU.configure_colorspace(target(), source(), config)
    assert "engine_pixfmt" not in config.state and config.state["rgb24_options"]


def test_rebinding_and_restoring(live):
    inst, VU, original = live
    from nunif_amd.nunif.utils.video import configure_colorspace
    assert ENTRY in inst.PATCHES
    assert original is not configure_colorspace and original.__module__ == "nunif.utils.video"
    assert VU.configure_colorspace is configure_colorspace
    assert VU.process_video.__globals__["configure_colorspace"] is configure_colorspace
    assert inst.original(*ENTRY) is original
    inst.uninstall()
    assert VU.configure_colorspace is original and VU.process_video.__globals__["configure_colorspace"] is original
    with pytest.raises(RuntimeError, match="install"):
        configure_colorspace(target(), source(), VU.VideoOutputConfig(colorspace="bt709"))


def test_the_engines_callbacks_declare_themselves_and_read_the_plan(live):
    """The waifu2x stream and the iw3 scheduler's op table: ``bind_config`` declares, the first frame reads ``engine_pixfmt``."""
    inst, VU, original = live
    from nunif_amd.iw3.frame_pipeline import PipelineOps
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    plan = CASES["bt601_guessed_to_bt709_full"][4]
    src_kw = CASES["bt601_guessed_to_bt709_full"][0]

    def configured(bind):
        config = VU.VideoOutputConfig(pix_fmt="yuv420p", colorspace="bt709-pc")
        bind(config)
        VU.configure_colorspace(target(), source(**src_kw), config)
        return config

    names = ("in_format", "in_matrix", "in_full_range", "out_format", "out_matrix", "out_full_range")
    ops = PipelineOps()
    assert configured(ops.bind_config).state["engine_pixfmt"] == plan
    ops._settle()
    resolved = dict(plan, out_format="yuv420p")                  # the layout's name; the frame's name is kept next to it
    assert {n: getattr(ops, n) for n in names} == resolved and ops.out_pix_fmt == "yuvj420p"
    args = NS(method="scale", pix_fmt="yuv420p")
    stream = Waifu2xVideoStream(None, args, device="cuda:0")
    assert configured(stream.bind_config).state["engine_pixfmt"] == plan
    stream._read_config()
    assert {n: getattr(stream, n) for n in names} == resolved and stream.out_pix_fmt == "yuvj420p"

    # not declared: a software --vf, a quarter turn, a caller's own edge functions
    for bind in (lambda c: PipelineOps().bind_config(c, vf="hflip"),
                 lambda c: PipelineOps(to_frame=lambda x, use_16bit=False: x).bind_config(c),
                 lambda c: Waifu2xVideoStream(None, NS(method="scale", rotate_left=True), device="cuda:0").bind_config(c),
                 lambda c: Waifu2xVideoStream(None, args, device="cuda:0").bind_config(c, vf="hflip")):
        state = configured(bind).state
        assert "engine_pixfmt" not in state and state["rgb24_options"]


class FakePlane(bytearray):
    line_size = 0


class FakeVideoFrame:
    """``av.VideoFrame(width, height, format)`` as far as ``pixfmt.to_av_frame`` uses it: planes with a pitch of their own."""

    def __init__(self, width, height, format):
        from nunif_amd.nunif.utils import pixfmt
        lay = pixfmt.PlaneLayout(format, width, height)
        self.width, self.height, self.format = width, height, NS(name=format)
        self.planes = []
        for w, h in zip(lay.plane_widths, lay.plane_heights):
            plane = FakePlane((w * lay.sample_bytes + 13) * h)
            plane.line_size = w * lay.sample_bytes + 13
            self.planes.append(plane)


@pytest.mark.parametrize("name", ["bt601_guessed_to_bt709_full", "yuvj444p_bt601_copy", "bt709_limited_to_bt709_limited"])
def test_the_returned_frames_carry_the_pix_fmt_the_encoder_was_opened_with(live, monkeypatch, name):
    """Full range at 8 bit: the reference renames ``config.pix_fmt`` to ``yuvj*`` (video.py:753-758, :783) and ``process_video``
    opens the encoder with that name (:1018).  A frame that called itself ``yuv420p`` would be converted again by the encoder,
    range included, so the frames the stream's ``av_callback`` returns are named ``config.pix_fmt``.  The stream's ring needs a
    GPU; its ``__call__`` is replaced by one that returns recognisable planes."""
    import numpy as np
    from nunif_amd.nunif.utils import pixfmt
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    inst, VU, original = live
    src_kw, pix_fmt, colorspace, settled, plan = CASES[name]
    monkeypatch.setitem(sys.modules, "av", NS(VideoFrame=FakeVideoFrame))

    class Stream(Waifu2xVideoStream):
        def __call__(self, frame):
            if self._config is not None:
                self._read_config()
            self.out_layout = pixfmt.PlaneLayout(self.out_format, 10, 6)
            buf = np.zeros(self.out_layout.nbytes, dtype=np.uint8)
            for i, v in enumerate(self.out_layout.views(buf)):
                v[...] = 40 + i
            return buf

    stream = Stream(None, NS(method="noise", pix_fmt=pix_fmt), device="cuda:0")
    callback = stream.av_callback(lambda x: pytest.fail("the rgb route was taken"))
    config = VU.VideoOutputConfig(pix_fmt=pix_fmt, colorspace=colorspace)
    stream.bind_config(config)
    VU.configure_colorspace(target(), source(**src_kw), config)
    frame = callback(object())
    assert isinstance(frame, FakeVideoFrame) and frame.format.name == config.pix_fmt == settled
    for i, (plane, w, h) in enumerate(zip(frame.planes, stream.out_layout.plane_widths, stream.out_layout.plane_heights)):
        rows = np.frombuffer(plane, dtype=np.uint8).reshape(h, plane.line_size)
        assert (rows[:, :w] == 40 + i).all() and (rows[:, w:] == 0).all()
    with pytest.raises(ValueError, match="not a name of"):
        pixfmt.to_av_frame(np.zeros(stream.out_layout.nbytes, dtype=np.uint8), stream.out_layout, format="yuvj444p" if "420" in settled else "yuvj420p")


def test_a_yuvj_name_with_a_limited_range_tag_is_a_fall_back():
    from nunif_amd.nunif.utils.video import ENGINE_CALLBACK, _engine_pixfmt
    options = dict(format="rgb24", src_color_range=1, dst_color_range=2, src_colorspace=1, dst_colorspace=1)
    config = NS(pix_fmt="yuvj420p", colorspace="bt709-tv", state={ENGINE_CALLBACK: True, "rgb24_options": options})
    dst = target()
    dst.codec_context.color_range = 1
    assert _engine_pixfmt(dst, source(), config) is None
    dst.codec_context.color_range = 2
    assert _engine_pixfmt(dst, source(), config)["out_format"] == "yuvj420p"


def test_the_ring_refuses_planar_slots_without_zero_copy():
    from nunif_amd.frame_ring import FrameRing
    with pytest.raises(ValueError, match="zero_copy"):
        FrameRing(lambda x: x, (4, 4, 3), (4, 4, 3), in_bytes=64, enter_fn=lambda b, device=None: b, zero_copy=False)
    with pytest.raises(ValueError, match="zero_copy"):
        FrameRing(lambda x: x, (4, 4, 3), (4, 4, 3), out_bytes=64, leave_fn=lambda y, bits, out=None: y, zero_copy=False)
