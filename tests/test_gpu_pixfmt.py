"""Planar YUV <-> the CHW tensor (nunif_amd/csrc/pixfmt.hip) on the GPU against tests/pixfmt_ref.py.

Way in: the unclamped ``debug`` tensor against the float64 restatement with the fp32 restatement's own deviation as yardstick,
``e_hip <= 2.2 * e_ref + 2^-23`` over the whole map and per colour plane.  Way out: the integer codes equal float64's rounding
outside the tie band (4 x the fp32 restatement's deviation, the rule of tests/test_gpu_jpeg.py), differ by at most 1 inside it, and
at most 1 % of a case's samples lie inside it; guard and padding bytes keep their fill.  Then what the two share: the rgb side
frame, streams, pinned memory, the planar ``FrameRing``, ``Waifu2xVideoStream``, the iw3 scheduler and the refusals."""
import ctypes
import types

import numpy as np
import pytest
import torch

import pixfmt_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR = 2.2, 2.0 ** -23
GUARD, FILL = 64, 0xA5
PITCH_MODES = ["pad64", "odd", "packed"]
CASES = [(shape, combo, PITCH_MODES[(i + j) % 3]) for i, shape in enumerate(R.SHAPES) for j, combo in enumerate(R.COMBOS)]
IDS = [f"{h}x{w}-{fmt}-{m}-{'full' if fr else 'limited'}-{p}" for (h, w), (fmt, m, fr), p in CASES]


@pytest.fixture(scope="module")
def pixfmt(hiplib):
    from nunif_amd.nunif.utils import pixfmt
    return pixfmt


def _layout(pixfmt, fmt, h, w, mode):
    return pixfmt.PlaneLayout(fmt, w, h, pitches=R.padded_pitches(fmt, w, mode))


def _guarded(n):
    """A device buffer of n bytes between two guards, everything filled; returns (whole, the n bytes in the middle)."""
    whole = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _upload(pixfmt, planes, lay):
    return torch.from_numpy(lay.pack(planes, fill=FILL)).to(DEV)


def _check_entry(pixfmt, name, planes, fmt, matrix, full, lay):
    v64 = R.yuv_to_rgb(planes, fmt, matrix, full, torch.float64)
    v32 = R.yuv_to_rgb(planes, fmt, matrix, full, torch.float32)
    buf = _upload(pixfmt, planes, lay)
    got = pixfmt.yuv_to_tensor(buf, lay, matrix, full, debug=True).cpu()
    assert got.shape == v64.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    e_hip, e_ref = (got.double() - v64).abs(), (v32.double() - v64).abs()
    print(f"{name}: e_hip {float(e_hip.max()):.3g} e_ref {float(e_ref.max()):.3g} bit-equal to the fp32 restatement: "
          f"{bool(torch.equal(got, v32))}")
    assert e_hip.max() <= FACTOR * e_ref.max() + FLOOR, name
    # stricter than the bound, and what the documents state: every upsampling weight is dyadic and nothing is contracted, so the
    # kernel evaluates the restatement's operations one by one
    assert torch.equal(got, v32), name
    for c in range(3):
        assert e_hip[c].max() <= FACTOR * e_ref[c].max() + FLOOR, (name, c)
    clamped = pixfmt.yuv_to_tensor(buf, lay, matrix, full)
    assert torch.equal(clamped.cpu(), got.clamp(0, 1))


def _check_exit(pixfmt, name, x, fmt, matrix, full, lay):
    whole, out = _guarded(lay.nbytes)
    ret = pixfmt.tensor_to_yuv(x.to(DEV), lay, matrix, full, out=out)
    assert ret is out
    host = whole.cpu().numpy()
    got = lay.views(host[GUARD:GUARD + lay.nbytes])
    a = R.exit_agreement(got, x, fmt, matrix, full)
    print(f"{name}: band {a['band']:.3e}, {a['in_band']} of {a['samples']} in band, {a['mismatches']} mismatches, {a['bad']} bad")
    assert a["bad"] == 0 and a["mismatches"] <= a["in_band"], (name, a)
    assert a["share"] <= R.BAND_SHARE, (name, a)
    # every byte that is not a sample kept its fill: the guards, the pitch padding, the gaps between planes
    mask = np.ones(host.size, dtype=bool)
    inner = mask[GUARD:GUARD + lay.nbytes]
    for v in lay.views(inner.view(np.uint8)):
        v[...] = 0
    assert bool((host[mask] == FILL).all()), name
    return got


# ---- accuracy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,combo,mode", CASES, ids=IDS)
def test_entry_against_float64(pixfmt, shape, combo, mode):
    (h, w), (fmt, matrix, full) = shape, combo
    lay = _layout(pixfmt, fmt, h, w, mode)
    for kind in R.INPUTS:
        _check_entry(pixfmt, f"{kind} {h}x{w} {fmt} {matrix} {full} {mode}", R.make_planes(kind, fmt, h, w), fmt, matrix, full, lay)


@pytest.mark.parametrize("shape,combo,mode", CASES, ids=IDS)
def test_exit_against_float64(pixfmt, shape, combo, mode):
    (h, w), (fmt, matrix, full) = shape, combo
    lay = _layout(pixfmt, fmt, h, w, mode)
    for kind in R.INPUTS:
        _check_exit(pixfmt, f"{kind} {h}x{w} {fmt} {matrix} {full} {mode}", R.make_tensor(kind, fmt, h, w), fmt, matrix, full, lay)


@pytest.mark.parametrize("fmt,matrix,full", [("yuv420p", "bt709", False), ("yuv444p", "bt601", True), ("yuv420p10le", "bt2020", False)])
@pytest.mark.parametrize("shape", R.LIMIT_SHAPES)
def test_both_directions_at_the_size_limits(pixfmt, shape, fmt, matrix, full):
    h, w = shape
    lay = _layout(pixfmt, fmt, h, w, "pad64")
    _check_entry(pixfmt, f"{h}x{w} {fmt}", R.make_planes("noise", fmt, h, w), fmt, matrix, full, lay)
    _check_exit(pixfmt, f"{h}x{w} {fmt}", R.make_tensor("noise", fmt, h, w), fmt, matrix, full, lay)


def test_pitch_modes_give_the_same_bits(pixfmt):
    """The wide-access path (pad64), the one-sample path (odd pitches) and packed rows compute the same."""
    for fmt, matrix, full in R.COMBOS[::4] + [R.COMBOS[3]]:
        for h, w in ((18, 33), (64, 96)):
            planes, x = R.make_planes("wild", fmt, h, w), R.make_tensor("wild", fmt, h, w).to(DEV)
            tensors, codes = [], []
            for mode in PITCH_MODES:
                lay = _layout(pixfmt, fmt, h, w, mode)
                tensors.append(pixfmt.yuv_to_tensor(_upload(pixfmt, planes, lay), lay, matrix, full, debug=True))
                codes.append([v.copy() for v in lay.views(pixfmt.tensor_to_yuv(x, lay, matrix, full).cpu().numpy())])
            assert torch.equal(tensors[0], tensors[1]) and torch.equal(tensors[0], tensors[2])
            for other in codes[1:]:
                assert all(np.array_equal(a, b) for a, b in zip(codes[0], other))


# ---- consistency ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (18, 33), (64, 96)])
@pytest.mark.parametrize("fmt,matrix,full", R.COMBOS[::4] + [R.COMBOS[3]])
def test_rgb_side_frame_is_to_frame_of_the_tensor(pixfmt, shape, fmt, matrix, full):
    from nunif_amd.iw3 import _ops
    h, w = shape
    lay = _layout(pixfmt, fmt, h, w, "pad64")
    bits = 16 if R.FORMATS[fmt][0] > 8 else 8
    for kind in ("noise", "wild"):
        buf = _upload(pixfmt, R.make_planes(kind, fmt, h, w), lay)
        frame = torch.full((h, w, 3), -1 if bits == 16 else 255, dtype=torch.int16 if bits == 16 else torch.uint8, device=DEV)
        x = pixfmt.yuv_to_tensor(buf, lay, matrix, full, frame_out=frame)
        assert torch.equal(x, pixfmt.yuv_to_tensor(buf, lay, matrix, full))
        assert frame.cpu().numpy().tobytes() == _ops.to_frame(x, bits).cpu().numpy().tobytes()
        pinned = torch.empty((h, w, 3), dtype=frame.dtype).pin_memory()
        pixfmt.yuv_to_tensor(buf, lay, matrix, full, frame_out=pinned)
        torch.cuda.synchronize()
        assert torch.equal(pinned, frame.cpu())


def test_two_calls_and_two_streams_are_bit_equal(pixfmt):
    fmt, matrix, full = "yuv420p", "bt709", False
    lay = _layout(pixfmt, fmt, 270, 480, "pad64")
    buf = _upload(pixfmt, R.make_planes("noise", fmt, 270, 480), lay)
    x = R.make_tensor("noise", fmt, 270, 480).to(DEV)
    a, b = pixfmt.yuv_to_tensor(buf, lay, matrix, full), pixfmt.yuv_to_tensor(buf, lay, matrix, full)
    p, q = pixfmt.tensor_to_yuv(x, lay, matrix, full), pixfmt.tensor_to_yuv(x, lay, matrix, full)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        c, r = pixfmt.yuv_to_tensor(buf, lay, matrix, full), pixfmt.tensor_to_yuv(x, lay, matrix, full)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(p, q) and torch.equal(p, r)


@pytest.mark.parametrize("fmt", sorted(R.FORMATS))
@pytest.mark.parametrize("shape", [(5, 7), (64, 96)])
def test_pinned_and_device_memory_are_bit_equal(pixfmt, shape, fmt):
    h, w = shape
    lay = _layout(pixfmt, fmt, h, w, "pad64")
    host = torch.from_numpy(lay.pack(R.make_planes("noise", fmt, h, w), fill=FILL)).pin_memory()
    want = pixfmt.yuv_to_tensor(host.to(DEV), lay, "bt601", False)
    assert torch.equal(pixfmt.yuv_to_tensor(host, lay, "bt601", False, device=DEV), want)
    x = R.make_tensor("noise", fmt, h, w).to(DEV)
    out = torch.full((lay.nbytes,), FILL, dtype=torch.uint8).pin_memory()
    pixfmt.tensor_to_yuv(x, lay, "bt601", False, out=out)
    torch.cuda.synchronize()
    dev = torch.full((lay.nbytes,), FILL, dtype=torch.uint8, device=DEV)
    assert torch.equal(out, pixfmt.tensor_to_yuv(x, lay, "bt601", False, out=dev).cpu())


def test_frame_ring_planar_form(pixfmt):
    from nunif_amd.frame_ring import FrameRing
    fmt, h, w = "yuv420p10le", 18, 34
    lin, lout = _layout(pixfmt, fmt, h, w, "pad64"), pixfmt.PlaneLayout("yuv444p", w, h)
    frames = [lin.pack(R.make_planes(k, fmt, h, w)) for k in ("noise", "constant", "checker", "wild", "noise", "wild")]
    frames[4], frames[5] = frames[4][::-1].copy(), frames[5][::-1].copy()       # six distinct frames
    ring = FrameRing(lambda x: x, None, None, device=DEV, depth=3, bits=8, in_bytes=lin, out_bytes=lout,
                     enter_fn=pixfmt.yuv_entry(lin, "bt2020", False), leave_fn=pixfmt.yuv_leave(lout, "bt601", True))
    outs = []
    for i, f in enumerate(frames):
        if i % 2:                                                               # both ways of handing a frame in
            for dst, src in zip(ring.input_buffer(), lin.views(f)):
                assert dst.shape == src.shape and dst.dtype == src.dtype
                np.copyto(dst, src)
            o = ring.submit(None)
        else:
            o = ring.submit(f)
        outs += [] if o is None else [o]
    outs += ring.drain()
    assert len(outs) == 6
    for f, o in zip(frames, outs):
        x = pixfmt.yuv_to_tensor(torch.from_numpy(f).to(DEV), lin, "bt2020", False)
        want = pixfmt.tensor_to_yuv(x, lout, "bt601", True).cpu().numpy()
        assert o.dtype == np.uint8 and o.shape == (lout.nbytes,)
        assert all(np.array_equal(a, b) for a, b in zip(lout.views(o), lout.views(want)))
    with pytest.raises(ValueError, match="enter_fn"):
        FrameRing(lambda x: x, None, (4, 4, 3), device=DEV, in_bytes=lin)
    # the rgb form next to it is what it was
    rgb = np.random.default_rng(1).integers(0, 256, (h, w, 3)).astype(np.uint8)
    plain = FrameRing(lambda x: x, (h, w, 3), (h, w, 3), device=DEV, depth=2)
    assert plain.submit(rgb) is None and np.array_equal(plain.drain()[0], rgb)


def _rgb_fed_bound(matrix, full, fmt, dx):
    """How far the codes of two planar exits may lie apart when the tensors going into the exit differ by at most ``dx``: a code is
    ``sum_j M_ij x_j + off`` rounded, the chroma downsample is an average with non-negative weights, so the distance is at most
    ``max_i sum_j |M_ij| * dx`` plus one code for the two roundings; one more code for the fp32 / half-precision noise of two model
    calls whose inputs differ in the last bit.  ``dx`` is the model's own answer to rounding its input to an rgb24 frame, taken on
    the restatement's tensors: nothing of the kernels under test enters the bound."""
    m, _ = R.coefficients(matrix, full, R.FORMATS[fmt][0], 1)
    gain = max(sum(abs(c) for c in row) for row in m)             # codes per unit of the [0, 1] tensor
    return int(np.ceil(gain * dx)) + 2


def _rgb24(t):
    """[3, H, W] in [0, 1] -> the HWC uint8 frame ``to_frame`` makes of it."""
    return np.ascontiguousarray(torch.floor(t.clamp(0, 1) * 255 + 0.5).permute(1, 2, 0).to(torch.uint8).numpy())


def _run(stream, frames):
    outs = []
    for f in frames + [None]:
        r = stream(f)
        outs += r if isinstance(r, list) else [] if r is None else [r]
    return outs


@pytest.mark.parametrize("grain", [False, True])
def test_waifu2x_video_stream_with_planes_in_and_out(pixfmt, tmp_path, grain):
    """The stream with planar ends against the same model fed the entry's tensor: an rgb24 / rgb48 frame cannot carry that tensor
    unquantised, so the rgb-fed stream is not the yardstick of the exit rule; the model call of the stream itself is."""
    from nunif_amd.nunif.models import save_model
    from nunif_amd.nunif.utils import rgb_noise
    from nunif_amd.synthetic import cunet_state_dict
    from nunif_amd.waifu2x.models.cunet import CUNet
    from nunif_amd.waifu2x.utils import Waifu2x
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    m = CUNet()
    m.load_state_dict(cunet_state_dict(312))
    save_model(m, str(tmp_path / "noise1.pth"))
    ctx = Waifu2x(str(tmp_path), [0])
    ctx.load_model("noise", 1)
    args = types.SimpleNamespace(method="noise", noise_level=1, tile_size=64, batch_size=4, tta=False, disable_amp=False,
                                 rotate_left=False, rotate_right=False, grain=grain, grain_strength=0.2, grain_speed=0.8,
                                 pix_fmt="yuv420p")
    h, w = 64, 64
    lin = _layout(pixfmt, "yuv420p", h, w, "pad64")
    planes = [R.make_planes(k, "yuv420p", h, w) for k in ("noise", "checker", "wild", "constant")]
    frames = [lin.pack(p) for p in planes]
    stream = Waifu2xVideoStream(ctx, args, DEV, seed=5, in_format="yuv420p", in_matrix="bt601", in_full_range=False,
                                out_format="yuvj420p", out_matrix="bt709")
    got = _run(stream, [(f, lin) for f in frames])
    assert len(got) == 4 and stream.out_layout.format == "yuv420p" and stream.out_full_range
    ref = Waifu2xVideoStream(ctx, args, DEV)
    buffer = None
    for i, (f, o) in enumerate(zip(frames, got)):
        with torch.inference_mode():
            y = ref._convert(pixfmt.yuv_to_tensor(torch.from_numpy(f).to(DEV), lin, "bt601", False)).float().contiguous()
            if grain:
                noise = rgb_noise.generate(tuple(y.shape), y.device, level=2, seed=5, counter=i)
                if buffer is None:
                    buffer = torch.empty_like(y)
                rgb_noise.blend_noise_buffer(buffer, noise, 0.8, i == 0)
                y = rgb_noise.apply_rgb_noise(y, buffer, strength=0.2)
        a = R.exit_agreement(stream.out_layout.views(o), y.cpu(), "yuv420p", "bt709", True)
        print(f"frame {i}: {a}")
        assert a["bad"] == 0 and a["mismatches"] <= a["in_band"] and a["share"] <= R.BAND_SHARE, a
    with pytest.raises(ValueError, match="pair"):
        Waifu2xVideoStream(ctx, args, DEV, in_format="yuv420p")(np.zeros((h, w, 3), dtype=np.uint8))
    if grain:
        return
    # the same stream fed the restatement's rgb24 frames: an entry that owes nothing to the kernel.  The rgb frame rounds the tensor
    # to half a code of 255, so the two streams agree within what the model makes of that rounding (_rgb_fed_bound)
    exact = [R.yuv_to_rgb(p, "yuv420p", "bt601", False, torch.float32, clamp=True) for p in planes]
    fed = _run(Waifu2xVideoStream(ctx, args, DEV, seed=5, out_format="yuvj420p", out_matrix="bt709"), [_rgb24(t) for t in exact])
    assert len(fed) == 4
    for i, (t, o, r) in enumerate(zip(exact, got, fed)):
        with torch.inference_mode():
            q = torch.from_numpy(_rgb24(t)).permute(2, 0, 1).float().div(255).contiguous().to(DEV)
            dx = float((ref._convert(t.to(DEV)).float().clamp(0, 1) - ref._convert(q).float().clamp(0, 1)).abs().max())
        bound = _rgb_fed_bound("bt709", True, "yuv420p", dx)
        worst = max(int(np.abs(a.astype(np.int64) - b.astype(np.int64)).max())
                    for a, b in zip(stream.out_layout.views(o), stream.out_layout.views(r)))
        print(f"frame {i}: rgb-fed stream within {worst} codes, bound {bound} (model dx {dx * 255:.3f} codes)")
        assert worst <= bound


def test_iw3_scheduler_with_planes_in_and_out(pixfmt):
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.frame_pipeline import HostFrame, PipelineOps, bind_single_frame_callback
    net = lambda t: t.mean(1) + 0.3 * t[:, 0]                              # noqa: E731
    args = types.SimpleNamespace(mapper="mul_1", convergence=0.5, divergence=3.0, method="forward_fill", synthetic_view="both",
                                 edge_dilation=2, tta=False, pix_fmt="yuv420p")
    h, w = 64, 96
    lin = _layout(pixfmt, "yuv420p", h, w, "pad64")
    frames = [lin.pack(R.make_planes(k, "yuv420p", h, w)) for k in ("noise", "checker", "wild")]

    def run(ops, feed):
        model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
        cb = bind_single_frame_callback(model, None, [], args, ops=ops)
        outs = []
        for i, f in enumerate(feed):
            outs += cb(HostFrame(f, i))
        return outs + cb(None)

    ops = PipelineOps(in_format="yuv420p", in_matrix="bt709", in_full_range=False, out_format="yuv420p", out_matrix="bt709")
    got = run(ops, [(f, lin) for f in frames])
    tensors = [pixfmt.yuv_to_tensor(torch.from_numpy(f).to(DEV), lin, "bt709", False) for f in frames]
    rgb = PipelineOps(to_tensor=lambda frame, device=None: frame.data, to_frame=lambda x, use_16bit=False: x.clone())
    want = run(rgb, tensors)
    assert len(got) == len(want) == 3
    lout = ops.out_layout(h, 2 * w)
    for g, sbs in zip(got, want):
        assert sbs.shape == (3, h, 2 * w) and g.dtype == torch.uint8 and g.shape == (lout.nbytes,)
        a = R.exit_agreement(lout.views(g.cpu().numpy()), sbs.cpu(), "yuv420p", "bt709", False)
        assert a["bad"] == 0 and a["mismatches"] <= a["in_band"] and a["share"] <= R.BAND_SHARE, a
    # the planes reach the kernel in pinned memory whatever they came in: pinned tensors and plain numpy give the same bytes
    pinned = [torch.from_numpy(f).pin_memory() for f in frames]
    again = run(PipelineOps(in_format="yuv420p", in_matrix="bt709", in_full_range=False, out_format="yuv420p", out_matrix="bt709"),
                [(f, lin) for f in pinned])
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert ops._staging and all(slot[0].is_pinned() for slot in ops._staging)
    # the same scheduler fed the restatement's rgb24 frames (U.to_tensor), within what its own stages make of that rounding.
    # For forward_fill this is a SMOKE CHECK, not a comparison: a depth that changes by a rounding moves whole pixels in the warp,
    # so on noise the stages' own answer, and with it the bound, is of the order of 100 codes; only a frame without such jumps
    # (the checker here: 3 codes) is held tightly.  The 3 codes of the waifu2x stream above are the meaningful figure
    planes = [R.make_planes(k, "yuv420p", h, w) for k in ("noise", "checker", "wild")]
    exact = [R.yuv_to_rgb(p, "yuv420p", "bt709", False, torch.float32, clamp=True) for p in planes]
    quant = [torch.from_numpy(_rgb24(t)).permute(2, 0, 1).float().div(255).contiguous() for t in exact]
    fed = run(PipelineOps(out_format="yuv420p", out_matrix="bt709"), [_rgb24(t) for t in exact])
    sens = zip(run(rgb, [t.to(DEV) for t in exact]), run(rgb, [t.to(DEV) for t in quant]))
    for i, (g, r, (a, b)) in enumerate(zip(got, fed, sens)):
        dx = float((a.clamp(0, 1) - b.clamp(0, 1)).abs().max())
        bound = _rgb_fed_bound("bt709", False, "yuv420p", dx)
        worst = max(int(np.abs(p.astype(np.int64) - q.astype(np.int64)).max())
                    for p, q in zip(lout.views(g.cpu().numpy()), lout.views(r.cpu().numpy())))
        print(f"frame {i}: rgb-fed scheduler within {worst} codes, bound {bound} (stages' dx {dx * 255:.3f} codes)")
        assert worst <= bound
    with pytest.raises(ValueError, match="pair"):
        ops.to_tensor(HostFrame(np.zeros((h, w, 3), dtype=np.uint8), 0), device=DEV)
    with pytest.raises(ValueError, match="to_tensor"):
        PipelineOps(in_format="yuv420p", to_tensor=lambda f, device=None: f)
    with pytest.raises(ValueError, match="out_format"):
        PipelineOps(out_format="nv12")


class _Plane(bytearray):
    line_size = 0


def _decoded(layout, planes, pts, name=None):
    """A decoded ``av.VideoFrame`` as far as the planar entry uses it: planes that expose the buffer protocol, at a pitch of their own."""
    out = []
    for arr, w, h in zip(planes, layout.plane_widths, layout.plane_heights):
        pitch = w * layout.sample_bytes + 24
        rows = np.full((h, pitch), FILL, dtype=np.uint8)
        rows[:, :w * layout.sample_bytes] = np.ascontiguousarray(arr).view(np.uint8).reshape(h, -1)
        plane = _Plane(rows.tobytes())
        plane.line_size = pitch
        out.append(plane)
    return types.SimpleNamespace(format=types.SimpleNamespace(name=name or layout.format), width=layout.width, height=layout.height,
                                 planes=out, pts=pts)


def test_iw3_av_frame_callback_takes_the_plan_and_names_its_frames(pixfmt):
    """``bind_av_frame_callback``: the scheduler behind a PyAV loop.  With ``engine_pixfmt`` on the config, decoded frames (stand-ins
    with padded planes) give the bytes the pair-fed scheduler gives, and the frames that come out carry the settled ``yuvj*`` name."""
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.frame_pipeline import HostFrame, PipelineOps, bind_av_frame_callback, bind_single_frame_callback
    from nunif_amd.nunif.utils.video import ENGINE_CALLBACK, ENGINE_PIXFMT
    net = lambda t: t.mean(1) + 0.3 * t[:, 0]                              # noqa: E731
    args = types.SimpleNamespace(mapper="mul_1", convergence=0.5, divergence=3.0, method="forward_fill", synthetic_view="both",
                                 edge_dilation=2, tta=False, pix_fmt="yuv420p")
    h, w = 30, 50
    lin = pixfmt.PlaneLayout("yuv420p", w, h)
    planes = [R.make_planes(k, "yuv420p", h, w) for k in ("noise", "checker")]
    plan = dict(in_format="yuv420p", in_matrix="bt601", in_full_range=True, out_format="yuvj420p", out_matrix="bt709",
                out_full_range=True)
    wrapped = []

    def to_planar_frame(buf, layout, format=None):
        wrapped.append(format)
        return buf, layout

    config = types.SimpleNamespace(state={})
    model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
    cb = bind_av_frame_callback(model, None, [], args, config, to_frame=None, to_planar_frame=to_planar_frame)
    assert config.state[ENGINE_CALLBACK] is True
    config.state[ENGINE_PIXFMT] = plan                                    # what the engine's configure_colorspace records
    got = []
    for i, p in enumerate(planes):
        got += cb(_decoded(lin, p, i, name="yuvj420p"))
    got += cb(None)
    model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
    ref = bind_single_frame_callback(model, None, [], args, ops=PipelineOps(**plan))
    want = []
    for i, p in enumerate(planes):
        want += ref(HostFrame((lin.pack(p), lin), i))
    want += ref(None)
    assert len(got) == len(want) == 2 and wrapped == ["yuvj420p", "yuvj420p"]
    for (buf, layout), t in zip(got, want):
        assert layout == cb.ops.out_layout(h, 2 * w) and layout.format == "yuv420p"
        assert np.array_equal(buf, t.cpu().numpy())

    # without a plan (the reference kept its state) the same binder is the rgb route: numpy HWC frames for VU.to_frame
    config = types.SimpleNamespace(state={})
    model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
    cb = bind_av_frame_callback(model, None, [], args, config, to_frame=lambda a: a)
    rgb = np.random.default_rng(3).integers(0, 256, (h, w, 3)).astype(np.uint8)
    outs = cb(HostFrame(rgb, 0)) + cb(None)
    assert len(outs) == 1 and isinstance(outs[0], np.ndarray) and outs[0].shape == (h, 2 * w, 3) and outs[0].dtype == np.uint8


def test_refusals(pixfmt):
    from nunif_amd import _hip
    lay = pixfmt.PlaneLayout("yuv420p", 16, 8)
    buf = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    x = torch.zeros((3, 8, 16), device=DEV)
    planes = lay._c_planes(buf)
    lib, s = _hip.lib(), _hip.current_stream_ptr(DEV)

    def enter(fmt=0, h=8, w=16, matrix=709, full=0, form=0, frame=None, p=planes):
        return lib.nunif_hip_yuv_to_tensor(ctypes.byref(p), fmt, h, w, matrix, full, form, ctypes.c_void_p(x.data_ptr()), frame, s)

    def leave(fmt=0, h=8, w=16, matrix=709, full=0, p=planes):
        return lib.nunif_hip_tensor_to_yuv(ctypes.c_void_p(x.data_ptr()), h, w, fmt, matrix, full, ctypes.byref(p), s)
    assert enter() == 0 and leave() == 0
    for call in (enter, leave):
        assert call(fmt=3) == -1 and call(fmt=-1) == -1 and call(matrix=240) == -1 and call(full=2) == -1
        assert call(h=8193) == -1 and call(w=8193) == -1 and call(h=0) == -1
        short = lay._c_planes(buf)
        short.pitch[1] = 7                                                     # smaller than the 8 chroma samples of a row
        assert call(p=short) == -1
        null = lay._c_planes(buf)
        null.data[2] = None
        assert call(p=null) == -1
    assert enter(form=2) == -1 and enter(form=1, frame=ctypes.c_void_p(buf.data_ptr())) == -1
    with pytest.raises(ValueError, match=r"\[3, 8, 16\]"):
        pixfmt.tensor_to_yuv(torch.zeros((3, 8, 8), device=DEV), lay, "bt709", False)
    with pytest.raises(ValueError, match="nbytes"):
        pixfmt.tensor_to_yuv(x, lay, "bt709", False, out=buf[:-1])
    with pytest.raises(ValueError, match="frame_out"):
        pixfmt.yuv_to_tensor(buf, lay, "bt709", False, frame_out=torch.zeros((8, 16, 3), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError, match="debug"):
        pixfmt.yuv_to_tensor(buf, lay, "bt709", False, frame_out=torch.zeros((8, 16, 3), dtype=torch.uint8, device=DEV), debug=True)
    with pytest.raises(ValueError, match="out must"):
        pixfmt.yuv_to_tensor(buf, lay, "bt709", False, out=torch.zeros((3, 8, 8), device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pixfmt.yuv_to_tensor(buf.cpu(), lay, "bt709", False, device=DEV)       # host memory that is not pinned
