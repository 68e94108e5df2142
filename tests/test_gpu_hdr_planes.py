"""The fused HDR planar entry (nunif_amd/csrc/hdr_planes.hip) on the GPU.

The main contract is bit-equality with the two-launch chain it replaces — ``pixfmt.yuv_to_tensor(..., frame_out=rgb48)`` followed by
``hdr.hdr2sdr_tensor(rgb48, ...)`` — over every case of tests/hdr_planes_ref.py and all three forms.  Independently of the chain's
first half, the debug form equals the map of the fp32 restatement's codes bit for bit and obeys the rule of tests/test_gpu_hdr.py
against float64, ``e_hip <= 2.2 * e_ref + 2^-23`` over the whole map and over each of the 16 bands of the brightest input code.  Then
memory (pinned planes, odd and padded pitches between guard bytes, streams) and the plumbing: ``FrameRing`` with ``hdr_yuv_entry``,
``Waifu2xVideoStream``, ``PipelineOps`` and the refusals that need a device."""
import ctypes
import types

import numpy as np
import pytest
import torch

import hdr_planes_ref as R
import hdr_ref
import pixfmt_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 2.2, 2.0 ** -23                  # tests/test_gpu_hdr.py's rule, unchanged
GUARD, FILL = 64, 0xA5
ACCURACY_SHAPES = [(5, 7), (18, 33), (64, 96), (8, 8192)]


@pytest.fixture(scope="module")
def hdr(hiplib):
    from nunif_amd.nunif.utils import hdr
    return hdr


@pytest.fixture(scope="module")
def pixfmt(hiplib):
    from nunif_amd.nunif.utils import pixfmt
    return pixfmt


def _layout(pixfmt, h, w, mode="pad64"):
    return pixfmt.PlaneLayout(R.FMT, w, h, pitches=P.padded_pitches(R.FMT, w, mode))


def _upload(planes, lay):
    return torch.from_numpy(lay.pack(planes, fill=FILL)).to(DEV)


def _rgb48(pixfmt, buf, lay, full):
    """The chain's first launch: the rgb48 side frame of the planar entry."""
    frame = torch.empty((lay.height, lay.width, 3), dtype=torch.int16, device=DEV)
    pixfmt.yuv_to_tensor(buf, lay, R.MATRIX, full, frame_out=frame)
    return frame


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


# ---- 1. bit-equality with the chain -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,axis,mode", R.CASES, ids=R.IDS)
def test_fused_launch_is_bit_equal_to_the_two_launch_chain(hdr, pixfmt, shape, axis, mode):
    (h, w), (trc, cs, full) = shape, axis
    lay = _layout(pixfmt, h, w, mode)
    for kind in R.KINDS:
        buf = _upload(R.make_planes(kind, h, w), lay)
        rgb48 = _rgb48(pixfmt, buf, lay, full)
        for form in R.FORMS:
            got = hdr.hdr2sdr_planes(buf, lay, full, trc, cs, form=form)
            want = hdr.hdr2sdr_tensor(rgb48, trc, cs, form=form)
            assert got.shape == want.shape and got.dtype == want.dtype
            assert torch.equal(got, want), (kind, form)


def test_chain_equality_holds_for_other_parameters(hdr, pixfmt):
    lay = _layout(pixfmt, 18, 33)
    buf = _upload(R.make_planes("noise", 18, 33), lay)
    rgb48 = _rgb48(pixfmt, buf, lay, False)
    for trc, params in ((R.HLG, {"hlg_saturation_gain": 1.0}), (R.HLG, {"hlg_saturation_gain": 0.5, "hlg_exposure": 1.0}),
                        (R.PQ, {"pq_exposure": 60.0, "pq_white_point": 3.0})):
        for form in R.FORMS:
            assert torch.equal(hdr.hdr2sdr_planes(buf, lay, False, trc, "bt601", form=form, **params),
                               hdr.hdr2sdr_tensor(rgb48, trc, "bt601", form=form, **params))


# ---- 2. independently of the chain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", R.AXES, ids=[i.split("-", 1)[1].rsplit("-", 1)[0] for i in R.IDS[:8]])
@pytest.mark.parametrize("shape", ACCURACY_SHAPES)
def test_debug_form_against_the_restatement_and_float64(hdr, pixfmt, shape, axis):
    (h, w), (trc, cs, full) = shape, axis
    lay = _layout(pixfmt, h, w)
    for kind in R.KINDS:
        name = f"{kind} {h}x{w} trc{trc} {cs} full={full}"
        planes = R.make_planes(kind, h, w)
        v64, _, codes = R.hdr_planes_ref(planes, full, trc, cs, torch.float64)
        v32, _, _ = R.hdr_planes_ref(planes, full, trc, cs, torch.float32)
        got = hdr.hdr2sdr_planes(_upload(planes, lay), lay, full, trc, cs, form="debug")
        # the codes the kernel maps are the restatement's, exactly: the map of THOSE codes (hdr.hip, a kernel that never saw the
        # planes) gives the same bits
        mapped = hdr.hdr2sdr_tensor(torch.from_numpy(codes.view(np.int16)).to(DEV), trc, cs, form="debug")
        assert torch.equal(got, mapped), name
        got = got.cpu()
        assert got.shape == v64.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        e_hip = (got.double() - v64).abs().amax(dim=2).numpy()
        e_ref = (v32.double() - v64).abs().amax(dim=2).numpy()
        band = hdr_ref.brightest_band(codes)
        worst = e_hip.max() / (FACTOR * e_ref.max() + FLOOR)
        assert e_hip.max() <= FACTOR * e_ref.max() + FLOOR, name
        for b in range(16):
            m = band == b
            if m.any():
                worst = max(worst, e_hip[m].max() / (FACTOR * e_ref[m].max() + FLOOR))
                assert e_hip[m].max() <= FACTOR * e_ref[m].max() + FLOOR, (name, b, e_hip[m].max(), e_ref[m].max())
        print(f"{name}: worst e_hip / bound {worst:.3f} (e_hip {e_hip.max():.3g}, e_ref {e_ref.max():.3g})")


@pytest.mark.parametrize("trc", [R.PQ, R.HLG])
@pytest.mark.parametrize("shape,mode", [((5, 7), "odd"), ((18, 33), "packed"), ((64, 96), "pad64"), ((16, 8), "pad64")])
def test_forms_follow_from_the_debug_form(hdr, pixfmt, shape, mode, trc):
    h, w = shape
    lay = _layout(pixfmt, h, w, mode)
    for kind in R.KINDS:
        buf = _upload(R.make_planes(kind, h, w), lay)
        debug = hdr.hdr2sdr_planes(buf, lay, False, trc, "bt709", form="debug")
        u16 = hdr.hdr2sdr_planes(buf, lay, False, trc, "bt709", form="u16")
        chw = hdr.hdr2sdr_planes(buf, lay, False, trc, "bt709")
        assert u16.dtype == torch.int16 and u16.shape == (h, w, 3) and chw.shape == (3, h, w) and chw.dtype == torch.float32
        q = u16.to(torch.int32) & 0xFFFF
        assert torch.equal(q, (debug * 65535).to(torch.int32))
        assert torch.equal(chw.cpu(), q.cpu().float().permute(2, 0, 1) / 65535)


# ---- 3. memory --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (64, 96)])
def test_pinned_planes_equal_device_planes(hdr, pixfmt, shape):
    h, w = shape
    lay = _layout(pixfmt, h, w)
    host = torch.from_numpy(lay.pack(R.make_planes("noise", h, w), fill=FILL)).pin_memory()
    for form in R.FORMS:
        want = hdr.hdr2sdr_planes(host.to(DEV), lay, False, R.PQ, "bt709", form=form)
        assert torch.equal(hdr.hdr2sdr_planes(host, lay, False, R.PQ, "bt709", form=form, device=DEV), want)
    dst = torch.empty((h, w, 3), dtype=torch.int16).pin_memory()
    out = hdr.hdr2sdr_planes(host, lay, False, R.PQ, "bt709", form="u16", out=dst, device=DEV)
    torch.cuda.synchronize()
    assert out is dst and torch.equal(dst, hdr.hdr2sdr_planes(host.to(DEV), lay, False, R.PQ, "bt709", form="u16").cpu())


@pytest.mark.parametrize("mode", R.PITCH_MODES)
@pytest.mark.parametrize("shape", [(5, 7), (18, 33), (64, 96)])
def test_guard_bytes_around_planes_and_output_stay_intact(hdr, pixfmt, shape, mode):
    h, w = shape
    lay, planes = _layout(pixfmt, h, w, mode), R.make_planes("wild", h, w)
    src = torch.full((lay.nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    src[GUARD:GUARD + lay.nbytes] = _upload(planes, lay)
    before = src.clone()
    ref_lay = _layout(pixfmt, h, w)
    for form, dtype, shp in (("u16", torch.int16, (h, w, 3)), ("chw", torch.float32, (3, h, w)), ("debug", torch.float32, (h, w, 3))):
        n = h * w * 3 * (2 if form == "u16" else 4)
        whole = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
        out = whole[GUARD:GUARD + n].view(dtype).view(shp)
        ret = hdr.hdr2sdr_planes(src[GUARD:GUARD + lay.nbytes], lay, True, R.HLG, "bt601", form=form, out=out)
        assert ret is out
        assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + n:] == FILL).all()), (form, mode)
        # the wide path, the one-sample path and packed rows compute the same
        assert torch.equal(out, hdr.hdr2sdr_planes(_upload(planes, ref_lay), ref_lay, True, R.HLG, "bt601", form=form)), (form, mode)
    assert torch.equal(src, before)


def test_two_calls_and_two_streams_are_bit_equal(hdr, pixfmt):
    lay = _layout(pixfmt, 270, 480)
    buf = _upload(R.make_planes("noise", 270, 480), lay)
    for trc in (R.PQ, R.HLG):
        a = hdr.hdr2sdr_planes(buf, lay, False, trc, "bt709", form="debug")
        b = hdr.hdr2sdr_planes(buf, lay, False, trc, "bt709", form="debug")
        torch.cuda.synchronize()
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            c = hdr.hdr2sdr_planes(buf, lay, False, trc, "bt709", form="debug")
        side.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c)


# ---- 4. FrameRing -------------------------------------------------------------------------------------------------------------
def _five_frames(h, w):
    planes = [R.make_planes(k, h, w) for k in R.KINDS]
    return planes + [[np.roll(p, 1, axis=1) for p in planes[0]]]


def test_frame_ring_with_the_planar_hdr_entry(hdr, pixfmt):
    from nunif_amd.frame_ring import FrameRing
    h, w = 18, 34
    lay = _layout(pixfmt, h, w)
    params = dict(hlg_saturation_gain=0.5)
    frames = [lay.pack(p) for p in _five_frames(h, w)]
    ring = FrameRing(lambda x: x, None, (h, w, 3), device=DEV, depth=3, bits=16, in_bytes=lay,
                     enter_fn=hdr.hdr_yuv_entry(lay, False, R.HLG, "bt709", **params))
    got = [o for o in [ring.submit(f) for f in frames] if o is not None] + ring.drain()
    rgb = [_u16(_rgb48(pixfmt, torch.from_numpy(f).to(DEV), lay, False)).copy() for f in frames]
    ref = FrameRing(lambda x: x, (h, w, 3), (h, w, 3), device=DEV, depth=3, bits=16, in_bits=16,
                    enter_fn=hdr.hdr_entry(R.HLG, "bt709", **params))
    want = [o for o in [ref.submit(f) for f in rgb] if o is not None] + ref.drain()
    assert len(got) == len(want) == 5
    for g, t in zip(got, want):
        assert g.dtype == np.uint16 and g.shape == (h, w, 3) and g.tobytes() == t.tobytes()
    assert len({g.tobytes() for g in got}) == 5                                  # five distinct frames: the order is observable


# ---- 5. Waifu2xVideoStream ------------------------------------------------------------------------------------------------
def _run(stream, frames):
    outs = []
    for f in frames + [None]:
        r = stream(f)
        outs += r if isinstance(r, list) else [] if r is None else [r]
    return outs


@pytest.fixture(scope="module")
def waifu2x_ctx(hiplib, tmp_path_factory):
    from nunif_amd.nunif.models import save_model
    from nunif_amd.synthetic import cunet_state_dict
    from nunif_amd.waifu2x.models.cunet import CUNet
    from nunif_amd.waifu2x.utils import Waifu2x
    d = tmp_path_factory.mktemp("cunet")
    m = CUNet()
    m.load_state_dict(cunet_state_dict(312))
    save_model(m, str(d / "noise1.pth"))
    ctx = Waifu2x(str(d), [0])
    ctx.load_model("noise", 1)
    return ctx


@pytest.mark.parametrize("out_format", [None, "yuv420p"])
@pytest.mark.parametrize("pix_fmt", ["yuv420p10le", "yuv420p"])
def test_waifu2x_video_stream_with_hdr_planes(hdr, pixfmt, waifu2x_ctx, pix_fmt, out_format):
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    args = types.SimpleNamespace(method="noise", noise_level=1, tile_size=64, batch_size=4, tta=False, disable_amp=False,
                                 rotate_left=False, rotate_right=False, grain=False, grain_strength=0.2, grain_speed=0.8, pix_fmt=pix_fmt)
    feed, rgb = [], []
    for (h, w), kind in (((64, 96), "noise"), ((64, 96), "ramp"), ((64, 64), "wild"), ((64, 64), "noise")):   # a shape change midway
        lay = _layout(pixfmt, h, w)
        buf = lay.pack(R.make_planes(kind, h, w))
        feed.append((buf, lay))
        rgb.append(_u16(_rgb48(pixfmt, torch.from_numpy(buf).to(DEV), lay, False)).copy())
    kw = {} if out_format is None else dict(out_format=out_format, out_matrix="bt709")
    entry = hdr.hdr_entry(R.PQ, "bt709")
    planar = Waifu2xVideoStream(waifu2x_ctx, args, DEV, in_format="yuv420p10le", in_matrix="bt2020", hdr=entry, **kw)
    got = _run(planar, feed)
    want = _run(Waifu2xVideoStream(waifu2x_ctx, args, DEV, hdr=hdr.hdr_entry(R.PQ, "bt709"), **kw), rgb)
    assert len(got) == len(want) == 4 and planar.frames_in == planar.frames_out == 4
    g_w, seen = [lay.width for _, lay in feed], []             # method "noise": the output has the input's size
    for g, t in zip(got, want):
        assert g.dtype == t.dtype == (np.uint8 if out_format or pix_fmt == "yuv420p" else np.uint16)
        assert g.shape == t.shape
        if out_format is None:
            assert g.tobytes() == t.tobytes()
        else:                                                  # planes: the samples; pitch padding is never written
            lout = pixfmt.PlaneLayout(out_format, g_w[len(seen)], 64)
            assert all(np.array_equal(a, b) for a, b in zip(lout.views(g), lout.views(t)))
        seen.append(g)


# ---- 6. PipelineOps ---------------------------------------------------------------------------------------------------------
class _Plane(bytearray):
    line_size = 0


def _decoded(layout, planes, pts):
    """A decoded ``av.VideoFrame`` as far as the planar entry uses it: planes with the buffer protocol at a pitch of their own."""
    out = []
    for arr, w, h in zip(planes, layout.plane_widths, layout.plane_heights):
        pitch = w * layout.sample_bytes + 24
        rows = np.full((h, pitch), FILL, dtype=np.uint8)
        rows[:, :w * layout.sample_bytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(h, -1)
        plane = _Plane(rows.tobytes())
        plane.line_size = pitch
        out.append(plane)
    return types.SimpleNamespace(format=types.SimpleNamespace(name=layout.format), width=layout.width, height=layout.height,
                                 planes=out, pts=pts)


def test_pipeline_ops_with_hdr_planes(hdr, pixfmt):
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.frame_pipeline import HostFrame, PipelineOps, bind_single_frame_callback
    h, w = 64, 96
    lay = pixfmt.PlaneLayout(R.FMT, w, h)
    params = dict(hlg_saturation_gain=0.7)
    planes = [R.make_planes(k, h, w) for k in ("noise", "ramp", "wild")]
    frames = [lay.pack(p) for p in planes]
    want = [hdr.hdr2sdr_planes(torch.from_numpy(f).to(DEV), lay, True, R.HLG, "bt601", form="chw", **params) for f in frames]

    def ops():
        return PipelineOps(in_format="yuv420p10le", in_matrix="bt2020", in_full_range=True, hdr=hdr.hdr_entry(R.HLG, "bt601", **params))
    o = ops()
    for f, p, t in zip(frames, planes, want):
        pinned = torch.from_numpy(f).pin_memory()
        assert torch.equal(o.to_tensor(HostFrame((pinned, lay), 0), device=DEV), t)          # a pinned tensor, read where it is
        assert torch.equal(o.to_tensor(HostFrame((f, lay), 0), device=DEV), t)               # a numpy buffer, staged
        assert torch.equal(o.to_tensor(_decoded(lay, p, 0), device=DEV), t)                  # a decoded frame's planes
    torch.cuda.synchronize()
    assert o._staging and all(slot[0].is_pinned() for slot in o._staging)

    net = lambda t: t.mean(1) + 0.3 * t[:, 0]                              # noqa: E731
    args = types.SimpleNamespace(mapper="mul_1", convergence=0.5, divergence=3.0, method="forward_fill", synthetic_view="both",
                                 edge_dilation=2, tta=False, pix_fmt="yuv420p")

    def run(ops, feed):
        model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
        cb = bind_single_frame_callback(model, None, [], args, ops=ops)
        outs = []
        for i, f in enumerate(feed):
            outs += cb(HostFrame(f, i))
        return outs + cb(None)
    got = run(ops(), [(f, lay) for f in frames])
    chain = [hdr.hdr2sdr_tensor(_rgb48(pixfmt, torch.from_numpy(f).to(DEV), lay, True), R.HLG, "bt601", form="chw", **params)
             for f in frames]
    ref = run(PipelineOps(to_tensor=lambda frame, device=None: frame.data), chain)
    assert len(got) == len(ref) == 3
    for g, r in zip(got, ref):
        assert g.shape == r.shape == (h, 2 * w, 3) and g.dtype == r.dtype and torch.equal(g, r)


# ---- 7. the refusals that need a device -------------------------------------------------------------------------------------
def test_refusals(hdr, pixfmt, waifu2x_ctx):
    from nunif_amd import _hip
    from nunif_amd.iw3.frame_pipeline import HostFrame, PipelineOps
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    lay = pixfmt.PlaneLayout(R.FMT, 16, 8)
    buf = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    out = torch.zeros((3, 8, 16), device=DEV)
    planes, prm = lay._c_planes(buf), _hip.Hdr2SdrParams(110.0, 5.0, 0.9)
    lib, s = _hip.lib(), _hip.current_stream_ptr(DEV)

    def call(fmt=2, h=8, w=16, full=0, trc=16, cs=709, form=1, p=planes):
        return lib.nunif_hip_yuv_hdr_to_tensor(ctypes.byref(p), fmt, h, w, full, trc, cs, ctypes.byref(prm), form,
                                               ctypes.c_void_p(out.data_ptr()), s)
    assert call() == 0
    assert call(fmt=0) == -1 and call(fmt=1) == -1 and call(trc=17) == -1 and call(cs=2020) == -1 and call(form=3) == -1
    assert call(h=8193) == -1 and call(w=8193) == -1 and call(h=0) == -1 and call(full=2) == -1
    short = lay._c_planes(buf)
    short.pitch[0] = 30
    null = lay._c_planes(buf)
    null.data[1] = None
    assert call(p=short) == -1 and call(p=null) == -1
    torch.cuda.synchronize()
    assert torch.equal(out, hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709"))      # the one accepted call ran
    with pytest.raises(ValueError, match="out must"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709", out=torch.zeros((3, 8, 8), device=DEV))
    with pytest.raises(ValueError, match="out must"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709", form="u16", out=out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr.hdr2sdr_planes(buf, lay, False, R.PQ, "bt709", out=torch.zeros((3, 8, 16)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdr.hdr2sdr_planes(buf.cpu(), lay, False, R.PQ, "bt709", device=DEV)         # host memory that is not pinned
    entry = hdr.hdr_entry(R.PQ, "bt709")
    args = types.SimpleNamespace(method="noise", noise_level=1, tile_size=64, batch_size=4, tta=False, disable_amp=False,
                                 rotate_left=False, rotate_right=False, grain=False, pix_fmt="yuv420p10le")
    stream = Waifu2xVideoStream(waifu2x_ctx, args, DEV, in_format="yuv420p10le", in_matrix="bt2020", hdr=entry)
    with pytest.raises(ValueError, match="pair"):
        stream(np.zeros((8, 16, 3), dtype=np.uint16))                                # an rgb48 frame where planes are expected
    other = pixfmt.PlaneLayout("yuv420p", 16, 8)
    with pytest.raises(ValueError, match="layout"):
        stream((np.zeros(other.nbytes, dtype=np.uint8), other))
    ops = PipelineOps(in_format="yuv420p10le", in_matrix="bt2020", hdr=entry)
    with pytest.raises(ValueError, match="layout"):
        ops.to_tensor(HostFrame((np.zeros(other.nbytes, dtype=np.uint8), other), 0), device=DEV)
