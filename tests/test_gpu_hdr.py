"""HDR -> SDR tone mapping (nunif_amd/csrc/hdr.hip) on the GPU against tests/hdr_ref.py.

Accuracy is judged before the truncation, against the float64 restatement, with the fp32 restatement's own deviation as yardstick:
``e_hip <= 2.2 * e_ref + 2^-23`` over the whole map and over each of the 16 bands of the pixel's brightest input code, no element
left out.  The three output forms are checked against one another exactly, the integers against what the live reference returned
(tests/golden/hdr2sdr.npz) within the reference's own error, then the plumbing: streams, pinned memory, the ``av_frame`` form, the
``FrameRing`` entry, ``Waifu2xVideoStream(hdr=...)`` and the refusals."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import hdr_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 2.2, 2.0 ** -23                  # the project's usual factor; one fp32 ulp at 1.0 (the values live in [0, 1])
EXTRA_SHAPES = [(1, 1), (3, 5), (7, 9), (1, 4099), (270, 480)]


@pytest.fixture(scope="module")
def hdr(hiplib):
    from nunif_amd.nunif.utils import hdr
    return hdr


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "hdr2sdr.npz"))


def _dev(x16):
    return torch.from_numpy(x16.view(np.int16)).to(DEV)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _accuracy(name, hdr, x16, trc, cs, params):
    """Asserts the bound for one frame; returns (worst ratio e_hip / bound, e_ref)."""
    v64, _ = R.hdr2sdr_ref(x16, trc, cs, torch.float64, **params)
    v32, _ = R.hdr2sdr_ref(x16, trc, cs, torch.float32, **params)
    got = hdr.hdr2sdr_tensor(_dev(x16), trc, cs, form="debug", **params).cpu()
    assert got.shape == v64.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    e_hip = (got.double() - v64).abs().amax(dim=2).numpy()
    e_ref = (v32.double() - v64).abs().amax(dim=2).numpy()
    band = R.brightest_band(x16)
    worst = e_hip.max() / (FACTOR * e_ref.max() + FLOOR)
    lines = [f"whole {e_hip.max():.3g} / {e_ref.max():.3g}"]
    for b in range(16):
        m = band == b
        if m.any():
            worst = max(worst, e_hip[m].max() / (FACTOR * e_ref[m].max() + FLOOR))
            lines.append(f"b{b} {e_hip[m].max():.2g}/{e_ref[m].max():.2g}")
    print(f"{name}: worst e_hip / bound {worst:.3f} | e_hip / e_ref: " + " ".join(lines))
    assert e_hip.max() <= FACTOR * e_ref.max() + FLOOR, name
    for b in range(16):
        m = band == b
        if m.any():
            assert e_hip[m].max() <= FACTOR * e_ref[m].max() + FLOOR, (name, b, e_hip[m].max(), e_ref[m].max())
    return worst, e_ref.max()


# ---- accuracy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_debug_form_against_float64_on_the_fixture_cases(hdr, name):
    inp, trc, cs, params = R.CASES[name]
    _accuracy(name, hdr, R.make_input(inp), trc, cs, params)


@pytest.mark.parametrize("trc", [R.PQ, R.HLG])
@pytest.mark.parametrize("shape", EXTRA_SHAPES)
def test_debug_form_against_float64_on_odd_shapes(hdr, shape, trc):
    h, w = shape
    x16 = R.make_input("noise", h, w)
    if h * w >= 4096:
        x16[0, : w // 2] = R.make_input("ramp", 1, w // 2)[0]                    # the dark bands, the toe, code 0
    _accuracy(f"{h}x{w} trc{trc}", hdr, x16, trc, "bt601" if trc == R.PQ else "bt709", {})


# ---- the forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trc", [R.PQ, R.HLG])
@pytest.mark.parametrize("shape", [(R.H, R.W)] + EXTRA_SHAPES)
def test_forms_are_consistent(hdr, shape, trc):
    h, w = shape
    for inp in ("noise", "ramp"):
        x = _dev(R.make_input(inp, h, w))
        debug = hdr.hdr2sdr_tensor(x, trc, "bt709", form="debug")
        u16 = hdr.hdr2sdr_tensor(x, trc, "bt709", form="u16")
        chw = hdr.hdr2sdr_tensor(x, trc, "bt709", form="chw")
        assert u16.dtype == torch.int16 and u16.shape == (h, w, 3) and chw.shape == (3, h, w) and chw.dtype == torch.float32
        q = u16.to(torch.int32) & 0xFFFF
        assert torch.equal(q, (debug * 65535).to(torch.int32))
        # IEEE division of the integers, computed where torch's division by a number is one (the host)
        assert torch.equal(chw.cpu(), q.cpu().float().permute(2, 0, 1) / 65535)


@pytest.mark.parametrize("trc", [R.PQ, R.HLG])
@pytest.mark.parametrize("cs", ["bt709", "bt601"])
def test_exact_codes(hdr, trc, cs):
    zeros = torch.zeros((5, 16, 3), dtype=torch.int16, device=DEV)
    ones = torch.full((5, 16, 3), -1, dtype=torch.int16, device=DEV)             # 65535
    assert not hdr.hdr2sdr_tensor(zeros, trc, cs, form="u16").any()
    assert not hdr.hdr2sdr_tensor(zeros, trc, cs, form="chw").any()
    assert bool((hdr.hdr2sdr_tensor(ones, trc, cs, form="u16") == -1).all())
    assert bool((hdr.hdr2sdr_tensor(ones, trc, cs, form="chw") == 1.0).all())


# ---- against the reference's integers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_integers_against_the_reference(hdr, fixture, name):
    inp, trc, cs, params = R.CASES[name]
    x16 = R.make_input(inp)
    v64, _ = R.hdr2sdr_ref(x16, trc, cs, torch.float64, **params)
    v32, _ = R.hdr2sdr_ref(x16, trc, cs, torch.float32, **params)
    e_ref_counts = float((v32.double() - v64).abs().max()) * 65535
    got = _u16(hdr.hdr2sdr_tensor(_dev(x16), trc, cs, form="u16", **params)).astype(np.int64)
    diff = np.abs(got - fixture[name].astype(np.int64))
    print(f"{name}: {100.0 * (diff == 0).mean():.2f} % of elements equal the reference's, largest difference {diff.max()} "
          f"(reference fp32 error {e_ref_counts:.2f} counts)")
    assert diff.max() <= math.ceil(e_ref_counts) + 1


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def test_two_calls_and_two_streams_are_bit_equal(hdr):
    x = _dev(R.make_input("noise", 270, 480))
    for trc in (R.PQ, R.HLG):
        a = hdr.hdr2sdr_tensor(x, trc, "bt709", form="debug")
        b = hdr.hdr2sdr_tensor(x, trc, "bt709", form="debug")
        torch.cuda.synchronize()
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            c = hdr.hdr2sdr_tensor(x, trc, "bt709", form="debug")
        side.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("shape", [(R.H, R.W), (7, 9)])
def test_pinned_source_and_destination_equal_the_device_ones(hdr, shape):
    x16 = R.make_input("noise", *shape)
    want = hdr.hdr2sdr_tensor(_dev(x16), R.PQ, "bt709", form="u16")
    src = torch.from_numpy(x16.view(np.int16)).pin_memory()
    dst = torch.empty(shape + (3,), dtype=torch.int16).pin_memory()
    out = hdr.hdr2sdr_tensor(src, R.PQ, "bt709", form="u16", out=dst, device=DEV)
    torch.cuda.synchronize()
    assert out is dst and torch.equal(dst, want.cpu())
    assert torch.equal(hdr.hdr2sdr_tensor(src, R.PQ, "bt709", form="chw", device=DEV),
                       hdr.hdr2sdr_tensor(_dev(x16), R.PQ, "bt709", form="chw"))


def test_av_frame_form(hdr, monkeypatch):
    from nunif_amd.nunif.utils.video import hdr2sdr
    for name, mod in R.fake_av_modules().items():
        monkeypatch.setitem(sys.modules, name, mod)
    reformatter = sys.modules["av.video.reformatter"]
    for name, trc, cs in (("noise", R.HLG, "bt601"), ("ramp", R.PQ, "bt709"), ("dark", R.PQ, "bt709")):
        x16 = R.make_input(name)
        frame = R.FakeFrame(x16)
        out = hdr2sdr(frame, trc, cs, device=DEV)
        assert isinstance(out, R.RecordingVideoFrame) and out.format == "rgb48le" and out.array.dtype == np.uint16
        assert np.array_equal(out.array, _u16(hdr.hdr2sdr_tensor(_dev(x16), trc, cs, form="u16")))
        assert (out.pts, out.dts, out.time_base, out.opaque) == (frame.pts, frame.dts, frame.time_base, frame.opaque)
        assert out.colorspace == (reformatter.Colorspace.ITU709 if cs == "bt709" else reformatter.Colorspace.ITU601)
        assert out.color_range == reformatter.ColorRange.JPEG
        assert frame.to_ndarray_kwargs == dict(format="rgb48le", src_color_range=frame.color_range,
                                               dst_color_range=reformatter.ColorRange.JPEG)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr2sdr(R.FakeFrame(x16), R.PQ, "bt709", device="cpu")


def test_frame_ring_with_the_hdr_entry(hdr):
    from nunif_amd.frame_ring import FrameRing
    from nunif_amd.iw3 import _ops
    frames = [R.make_input(n, 40, 56) for n in R.INPUTS]
    ring = FrameRing(lambda x: x, (40, 56, 3), (40, 56, 3), device=DEV, depth=2, bits=16, in_bits=16,
                     enter_fn=hdr.hdr_entry(R.HLG, "bt709", hlg_saturation_gain=0.5))
    outs = [o for o in [ring.submit(f) for f in frames] if o is not None] + ring.drain()
    assert len(outs) == 3
    for f, o in zip(frames, outs):
        chw = hdr.hdr2sdr_tensor(_dev(f), R.HLG, "bt709", form="chw", hlg_saturation_gain=0.5)
        assert o.dtype == np.uint16 and o.tobytes() == _u16(_ops.to_frame(chw, 16)).tobytes()


def test_waifu2x_video_stream_with_hdr(hdr, tmp_path):
    from nunif_amd.nunif.models import save_model
    from nunif_amd.synthetic import cunet_state_dict
    from nunif_amd.waifu2x.models.cunet import CUNet
    from nunif_amd.waifu2x.utils import Waifu2x
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    m = CUNet()
    m.load_state_dict(cunet_state_dict(312))
    save_model(m, str(tmp_path / "noise1.pth"))
    ctx = Waifu2x(str(tmp_path), [0])
    ctx.load_model("noise", 1)

    def args(**kw):
        base = dict(method="noise", noise_level=1, tile_size=64, batch_size=4, tta=False, disable_amp=False, rotate_left=False,
                    rotate_right=False, grain=False, grain_strength=0.2, grain_speed=0.8, pix_fmt="yuv420p10le")
        base.update(kw)
        return types.SimpleNamespace(**base)

    def run(stream, frames):
        outs = []
        for f in frames + [None]:
            r = stream(f)
            outs += r if isinstance(r, list) else [] if r is None else [r]
        return outs

    frames = [R.make_input(n, 64, 64) for n in ("noise", "ramp", "dark", "noise")]
    got = run(Waifu2xVideoStream(ctx, args(), DEV, hdr=hdr.hdr_entry(R.PQ, "bt709")), frames)
    mapped = [_u16(hdr.hdr2sdr_tensor(_dev(f), R.PQ, "bt709", form="u16")).copy() for f in frames]
    want = run(Waifu2xVideoStream(ctx, args(), DEV), mapped)
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == np.uint16 and np.array_equal(g, w)
    with pytest.raises(ValueError, match="rotate"):
        Waifu2xVideoStream(ctx, args(rotate_left=True), DEV, hdr=hdr.hdr_entry(R.PQ, "bt709"))
    with pytest.raises(ValueError, match="rgb48"):
        Waifu2xVideoStream(ctx, args(), DEV, hdr=hdr.hdr_entry(R.PQ, "bt709"))(np.zeros((64, 64, 3), dtype=np.uint8))


def test_refusals(hdr):
    import ctypes
    from nunif_amd import _hip
    x = torch.zeros((4, 8, 3), dtype=torch.int16, device=DEV)
    out = torch.empty_like(x)
    p = _hip.Hdr2SdrParams(110.0, 5.0, 0.9)

    def call(h, w, trc, cs, form=0):
        return _hip.lib().nunif_hip_hdr2sdr(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), h, w, trc, cs,
                                            ctypes.byref(p), form, _hip.current_stream_ptr(DEV))
    assert call(4, 8, 16, 709) == 0
    assert call(4, 8, 17, 709) == -1 and call(4, 8, 16, 2020) == -1             # NUNIF_HIP_EINVAL, nothing is launched
    assert call(1, 8193, 16, 709) == -1 and call(8193, 1, 18, 601) == -1 and call(4, 8, 16, 709, form=3) == -1
    with pytest.raises(ValueError):
        hdr.hdr2sdr_tensor(x, 1, "bt709")
    with pytest.raises(ValueError):
        hdr.hdr2sdr_tensor(x, R.PQ, "bt2020")
    with pytest.raises(ValueError, match="8192"):
        hdr.hdr2sdr_tensor(torch.zeros((1, 8193, 3), dtype=torch.int16, device=DEV), R.PQ, "bt709")
    with pytest.raises(ValueError):
        hdr.hdr2sdr_tensor(x.to(torch.uint8), R.PQ, "bt709")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr.hdr2sdr_tensor(x.cpu(), R.PQ, "bt709")
