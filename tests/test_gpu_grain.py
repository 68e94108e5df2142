"""Film grain and the waifu2x video loop on the GPU (``grain.hip``, ``nunif_amd/nunif/utils/rgb_noise.py``,
``nunif_amd/waifu2x/video.py``) against tests/golden/rgb_noise.npz (the reference's recorded fp32 results, written by
tests/golden/make_golden_grain.py) and the float64 restatement of tests/grain_ref.py.

Bounds.  The statistical bounds are 5 standard errors computed from the sample count (grain_ref.moments).  The 8-bit condition
(no value more than one step from the quantised float64 result, at most 0.1 % one step off) is fixed by the feature's
specification.  The three measured bounds follow the precedent of tests/test_gpu_swin_errloc.py — about twice the worst figure
measured on the MI355X:

    MEASURED on MI355X (gfx950) with
        python -m pytest tests/test_gpu_grain.py -m gpu -s -k "apply_parity"
    worst over the 7 apply cases of the fixture + the 4-D case (each line of the output is one case):
        linear-domain error, engine / reference fp32:   1.61  (s10_flat; 1.12 .. 1.61 over the cases)
        16 bit: share of values one step off float64:   0.00278   (s02_flat; the reference's own there: 0.00182)
        16 bit: largest step:                           1
"""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grain_ref as G
from conftest import GOLDEN, synth_image

pytestmark = pytest.mark.gpu

LINEAR_RATIO_BOUND = 3.2       # engine max linear-domain error <= this multiple of the reference fp32's
SHARE16_BOUND = 0.0056          # 16 bit: share of values one step off the quantised float64 result
STEP16_BOUND = 2            # 16 bit: largest difference in steps
SHARE8_BOUND = 1e-3                      # 8 bit: fixed by the specification, with a largest step of 1

APPLY_CASES = {"s01": (0.1, 2.2, True), "s02": (0.2, 2.2, True), "s10": (1.0, 2.2, True),
               "s01_flat": (0.1, 2.2, False), "s02_flat": (0.2, 2.2, False), "s10_flat": (1.0, 2.2, False),
               "s02_g18": (0.2, 1.8, True)}
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "rgb_noise.npz")))


@pytest.fixture(scope="module")
def R(hiplib):
    from nunif_amd.nunif.utils import rgb_noise
    return rgb_noise


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frame_np(t, bits):
    a = t.cpu().numpy()
    return a.view(np.uint16) if bits == 16 else a


# ---- apply ------------------------------------------------------------------------------------------------------------
def _parity(name, engine, reference, ref64, gamma):
    lin_e = np.abs(engine.astype(np.float64) ** gamma - ref64 ** gamma).max()
    lin_r = np.abs(reference.astype(np.float64) ** gamma - ref64 ** gamma).max()
    e8, r8 = (G.step_shares(G.quantise(v, 8), G.quantise(ref64, 8)) for v in (engine, reference))
    e16, r16 = (G.step_shares(G.quantise(v, 16), G.quantise(ref64, 16)) for v in (engine, reference))
    print(f"  {name:9s} linear: engine {lin_e:.3g} reference {lin_r:.3g} ratio {lin_e / lin_r:.2f} | output: engine "
          f"{np.abs(engine - ref64).max():.3g} reference {np.abs(reference - ref64).max():.3g} | 8 bit (share, max): engine {e8} "
          f"reference {r8} | 16 bit: engine ({e16[0]:.5f}, {e16[1]}) reference ({r16[0]:.5f}, {r16[1]})")
    return lin_e / lin_r, e8, e16


def test_apply_parity_with_the_reference_and_float64(golden, R):
    worst = [0.0, 0.0, 0]
    fails = []
    cases = [(n, "x3", "noise3", f"apply_{n}", c) for n, c in APPLY_CASES.items()] + [("4d_s02", "x4", "noise4", "apply4_s02",
                                                                                      (0.2, 2.2, True))]
    for name, kx, kn, ky, (s, gm, ld) in cases:
        x, n = golden[kx], golden[kn]
        y = R.apply_rgb_noise(_dev(x), _dev(n), strength=s, gamma=gm, light_decay=ld)
        assert y.shape == x.shape and y.dtype == torch.float32
        ratio, e8, e16 = _parity(name, y.cpu().numpy(), golden[ky], G.apply64(x, n, s, gm, ld), gm)
        worst = [max(worst[0], ratio), max(worst[1], e16[0]), max(worst[2], e16[1])]
        if not (ratio <= LINEAR_RATIO_BOUND and e8[1] <= 1 and e8[0] <= SHARE8_BOUND and e16[0] <= SHARE16_BOUND and
                e16[1] <= STEP16_BOUND):
            fails.append(name)
    print(f"  worst: linear ratio {worst[0]:.2f}  16-bit share {worst[1]:.5f}  16-bit step {worst[2]}")
    assert not fails, fails


def test_apply_keeps_exact_black_and_white_and_takes_defaults(golden, R):
    x = torch.tensor([0.0, 1.0, 0.0, 1.0], device=DEV).view(1, 2, 2).repeat(3, 1, 1)
    zero = torch.zeros_like(x)
    assert torch.equal(R.apply_rgb_noise(x, zero), x)
    y = R.apply_rgb_noise(_dev(golden["x3"]), _dev(golden["noise3"]))
    assert torch.equal(y, R.apply_rgb_noise(_dev(golden["x3"]), _dev(golden["noise3"]), 0.2, 2.2, True, 0.8))
    with pytest.raises(AssertionError):
        R.apply_rgb_noise(x, zero, light_decay_strength=1.5)


# ---- generator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2])
def test_generator_statistics(R, level):
    shape = (3, 1024, 1024)
    a = R.generate(shape, DEV, level=level, seed=20260116, counter=5)
    b = R.generate(shape, DEV, level=level, seed=20260116, counter=6)
    assert torch.isfinite(a).all()
    print(f"level {level}:")
    bad = G.check_moments(G.moments(a.cpu(), level))
    bad += G.check_moments({"channels_0_1": G.cross_moment(a[0].cpu(), a[1].cpu(), level),
                            "channels_1_2": G.cross_moment(a[1].cpu(), a[2].cpu(), level),
                            "counters_5_6": G.cross_moment(a.cpu(), b.cpu(), level)})
    if level == 2:
        n1 = R.generate(shape, DEV, level=2, seed=20260116, counter=5, component=1)
        grid = R.generate(shape, DEV, level=2, seed=20260116, counter=5, component=3)
        up = R.generate(shape, DEV, level=2, seed=20260116, counter=5, component=2)
        assert grid.shape == (3, 512, 512)
        bad += G.check_moments({f"n1_{k}": v for k, v in G.moments(n1.cpu(), 1).items()})
        bad += G.check_moments({f"grid_{k}": v for k, v in G.moments(grid.cpu(), 1).items()})
        bad += G.check_moments({"n1_vs_up": G.cross_moment(n1.cpu(), up.cpu(), 1)})
        assert torch.equal(a, n1 * 0.5 + up * 0.5)                     # noise.mul_(0.5).add_(noise2, alpha=0.5)
    assert not bad, bad


@pytest.mark.parametrize("shape", [(3, 67, 101), (2, 3, 33, 50), (3, 64, 96), (3, 5, 7)])
def test_level2_cells_follow_torchs_nearest_rule(R, shape):
    kw = dict(level=2, seed=99, counter=3)
    grid = R.generate(shape, DEV, component=3, **kw)
    up = R.generate(shape, DEV, component=2, **kw)
    n1 = R.generate(shape, DEV, component=1, **kw)
    full = R.generate(shape, DEV, component=0, **kw)
    h, w = shape[-2:]
    assert grid.shape == shape[:-2] + (h // 2, w // 2)
    want = F.interpolate(grid.reshape((-1,) + grid.shape[-3:]), size=(h, w), mode="nearest").reshape(shape)
    assert torch.equal(up, want)                                                     # torch's own device kernel
    iy, ix = G.nearest_index(h, h // 2), G.nearest_index(w, w // 2)                 # and the restated rule
    assert np.array_equal(up.cpu().numpy(), grid.cpu().numpy()[..., iy, :][..., ix])
    assert torch.equal(full, n1 * 0.5 + up * 0.5)
    assert torch.equal(R.generate(shape, DEV, level=1, seed=99, counter=3), n1)


def test_generator_is_deterministic_and_keyed(R):
    shape = (3, 270, 480)
    a = R.generate(shape, DEV, seed=7, counter=11)
    assert torch.equal(a, R.generate(shape, DEV, seed=7, counter=11))
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    with torch.cuda.stream(s1):
        b = R.generate(shape, DEV, seed=7, counter=11)
    with torch.cuda.stream(s2):
        c = R.generate(shape, DEV, seed=7, counter=11)
    s1.synchronize()
    s2.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    # a value depends on its coordinates, not on the launch: the first image of a batch of two is the single draw
    six = R.generate((2, 3) + shape[1:], DEV, seed=7, counter=11)
    assert torch.equal(six[0], a)
    for other in (R.generate(shape, DEV, seed=7, counter=12), R.generate(shape, DEV, seed=8, counter=11),
                  R.generate(shape, DEV, seed=7, counter=11 + (1 << 32)), R.generate(shape, DEV, seed=7 + (1 << 32), counter=11)):
        assert not torch.equal(a, other)
        assert abs(G.cross_moment(a.cpu(), other.cpu(), 2)[0]) < 5 * G.cross_moment(a.cpu(), other.cpu(), 2)[2]


def test_rgb_noise_like_follows_torchs_seed(R):
    base = torch.zeros(3, 40, 64, device=DEV)
    torch.manual_seed(1234)
    a1, a2 = R.rgb_noise_like(base), R.rgb_noise_like(base)
    torch.manual_seed(1234)
    b1, b2 = R.rgb_noise_like(base), R.rgb_noise_like(base, level=2)
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)
    torch.manual_seed(1235)
    assert not torch.equal(R.rgb_noise_like(base), a1)
    assert R.rgb_noise_like(torch.zeros(2, 3, 8, 12, device=DEV), level=1).shape == (2, 3, 8, 12)


# ---- the blend and the fused step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,speed", [("v08", 0.8), ("v03", 0.3)])
def test_blend_against_the_recorded_steps(golden, R, name, speed):
    buf = torch.empty(3, 24, 40, device=DEV)
    for i in range(3):
        R.blend_noise_buffer(buf, _dev(golden["video_noise"][i]), speed, first=(i == 0))
        assert np.array_equal(buf.cpu().numpy(), golden[f"video_buf_{name}"][i]), i         # the fp32 recurrence, bit for bit
        y = R.apply_rgb_noise(_dev(golden["video_x"][i]), buf, strength=0.2).cpu().numpy()
        ref64 = G.apply64(golden["video_x"][i], golden[f"video_buf_{name}"][i], 0.2)     # same fp32 buffer on all sides
        ratio, e8, _ = _parity(f"{name}[{i}]", y, golden[f"video_out_{name}"][i], ref64, 2.2)
        assert ratio <= LINEAR_RATIO_BOUND and e8[1] <= 1 and e8[0] <= SHARE8_BOUND


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("shapes", [((40, 64), (36, 52)), ((33, 50), (40, 64)), ((270, 480), (135, 242))])
def test_fused_step_equals_the_separate_launches(R, bits, shapes):
    """5 frames, the frame size changes after the second: the buffer restarts as ui_utils.py:169-171 does."""
    from nunif_amd.iw3 import _ops
    seed, speed, strength = 4242, 0.8, 0.2
    buf_s = buf_f = None
    for i in range(5):
        h, w = shapes[0] if i < 2 else shapes[1]
        x = synth_image(900 + i, 3, h, w).to(DEV)
        first = buf_s is None or buf_s.shape != x.shape
        if first:
            buf_s, buf_f = torch.empty_like(x), torch.empty_like(x)
        noise = R.generate(x.shape, DEV, level=2, seed=seed, counter=i)
        R.blend_noise_buffer(buf_s, noise, speed, first)
        want = _ops.to_frame(R.apply_rgb_noise(x, buf_s, strength=strength), bits)
        got = torch.empty((h, w, 3), dtype=torch.uint8 if bits == 8 else torch.int16, device=DEV)
        R.grain_video_step(x, buf_f, got, bits=bits, seed=seed, counter=i, speed=speed, first=first, strength=strength)
        assert torch.equal(buf_f, buf_s), (i, "noise buffer")
        assert torch.equal(got, want), (i, "frame")
        assert not torch.equal(got, _ops.to_frame(x, bits))
        again = torch.empty_like(got)
        buf_again = buf_s.clone() if first else prev_buf.clone()
        R.grain_video_step(x, buf_again, again, bits=bits, seed=seed, counter=i, speed=speed, first=first, strength=strength)
        assert torch.equal(again, got) and torch.equal(buf_again, buf_f)
        prev_buf = buf_f.clone()


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("which", ["rgb", "buffer", "frame"])
def test_fused_step_with_an_unaligned_view_takes_the_scalar_instance(R, bits, which):
    """A width that is a multiple of 4 but a pointer off its 16 / 8 byte alignment (a view into a larger allocation): the host
    dispatches the one-pixel-per-access instance, and the bytes are the same."""
    h, w = 40, 64
    x = synth_image(31, 3, h, w).to(DEV)
    old = torch.randn(3, h, w, device=DEV)
    f_dtype = torch.uint8 if bits == 8 else torch.int16

    def off(t):                                   # the same values one element into a larger allocation
        big = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        view = big[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % (16 if t.dtype == torch.float32 else 8) != 0
        return view

    want, buf = torch.empty((h, w, 3), dtype=f_dtype, device=DEV), old.clone()
    R.grain_video_step(x, buf, want, bits=bits, seed=3, counter=9, first=False)
    xx = off(x) if which == "rgb" else x
    bb = off(old) if which == "buffer" else old.clone()
    got = off(torch.zeros((h, w, 3), dtype=f_dtype, device=DEV)) if which == "frame" else torch.empty_like(want)
    R.grain_video_step(xx, bb, got, bits=bits, seed=3, counter=9, first=False)
    assert torch.equal(got, want) and torch.equal(bb, buf)
    assert torch.equal(R.apply_rgb_noise(off(x), off(old)), R.apply_rgb_noise(x, old))
    nb = off(old)
    R.blend_noise_buffer(nb, off(x), 0.3, False)
    assert torch.equal(nb, R.blend_noise_buffer(old.clone(), x, 0.3, False))


def test_fused_step_writes_a_pinned_host_frame(R):
    from nunif_amd.iw3 import _ops
    x = synth_image(5, 3, 48, 64).to(DEV)
    buf_a, buf_b = torch.empty_like(x), torch.empty_like(x)
    dev_out = torch.empty((48, 64, 3), dtype=torch.uint8, device=DEV)
    host_out = torch.empty((48, 64, 3), dtype=torch.uint8).pin_memory()
    R.grain_video_step(x, buf_a, dev_out, seed=1, counter=0, first=True)
    R.grain_video_step(x, buf_b, host_out, seed=1, counter=0, first=True)
    torch.cuda.synchronize()
    assert torch.equal(dev_out.cpu(), host_out)


# ---- rotation at the entry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("hw", [(45, 70), (64, 96), (1, 33)])
def test_frame_to_tensor_with_a_quarter_turn(hiplib, bits, hw):
    from nunif_amd.iw3 import _ops
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256 if bits == 8 else 65536, size=hw + (3,)).astype(np.uint8 if bits == 8 else np.uint16)
    t = torch.from_numpy(frame.view(np.int16) if bits == 16 else frame).to(DEV)
    plain = _ops.frame_to_tensor(t)
    assert torch.equal(_ops.frame_to_tensor(t, turns=0), plain)
    for turns in (1, 3):
        got = _ops.frame_to_tensor(t, turns=turns)
        assert got.shape == (3, hw[1], hw[0])
        assert torch.equal(got, torch.rot90(plain, turns, (-2, -1))), turns
    pinned = torch.from_numpy(frame.view(np.int16) if bits == 16 else frame).pin_memory()
    assert torch.equal(_ops.frame_to_tensor(pinned, device=DEV, turns=1), torch.rot90(plain, 1, (-2, -1)))


# ---- the stream -------------------------------------------------------------------------------------------------------
def _args(method, noise_level, **kw):
    base = dict(method=method, noise_level=noise_level, tile_size=64, batch_size=4, tta=False, disable_amp=False,
                rotate_left=False, rotate_right=False, grain=False, grain_strength=0.2, grain_speed=0.8, pix_fmt="yuv420p")
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.fixture(scope="module", params=["swin_unet_2x", "cunet"])
def ctx_case(request, tmp_path_factory, hiplib):
    from nunif_amd.nunif.models import save_model
    from nunif_amd.synthetic import cunet_state_dict, swin_unet_state_dict
    from nunif_amd.waifu2x.utils import Waifu2x
    d = tmp_path_factory.mktemp(request.param)
    if request.param == "swin_unet_2x":
        from nunif_amd.waifu2x.models.swin_unet import SwinUNet2x
        m = SwinUNet2x()
        m.load_state_dict(swin_unet_state_dict(311, 2))
        save_model(m, str(d / "scale2x.pth"))
        method, noise_level, scale = "scale", -1, 2
    else:
        from nunif_amd.waifu2x.models.cunet import CUNet
        m = CUNet()
        m.load_state_dict(cunet_state_dict(312))
        save_model(m, str(d / "noise1.pth"))
        method, noise_level, scale = "noise", 1, 1
    ctx = Waifu2x(str(d), [0])
    ctx.load_model(method, noise_level)
    return ctx, method, noise_level, scale


def _frames(n, h, w, bits=8):
    maxv = 255 if bits == 8 else 65535
    return [(synth_image(500 + i, 3, h, w).permute(1, 2, 0) * maxv).round().numpy().astype(np.uint8 if bits == 8 else np.uint16)
            for i in range(n)]


def _run(stream, frames):
    outs = []
    for f in frames:
        r = stream(f)
        outs += r if isinstance(r, list) else [] if r is None else [r]
    assert len(outs) < len(frames)                     # the ring holds frames in flight
    r = stream(None)
    outs += r if isinstance(r, list) else [] if r is None else [r]
    assert stream(None) is None
    return outs


@pytest.mark.parametrize("bits", [8, 16])
def test_stream_without_grain_equals_convert_frame_by_frame(ctx_case, bits):
    from nunif_amd.iw3 import _ops
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    ctx, method, noise_level, scale = ctx_case
    frames = _frames(12, 48, 72, bits)
    args = _args(method, noise_level, pix_fmt="yuv420p10le" if bits == 16 else "yuv420p")
    stream = Waifu2xVideoStream(ctx, args, DEV)
    outs = _run(stream, frames)
    assert len(outs) == 12 and stream.frames_in == stream.frames_out == 12
    for i, (f, o) in enumerate(zip(frames, outs)):
        t = torch.from_numpy(f.view(np.int16) if bits == 16 else f).to(DEV)
        y, _ = ctx.convert(_ops.frame_to_tensor(t), None, method, noise_level, 64, 4, False, enable_amp=True, output_device=DEV)
        want = _frame_np(_ops.to_frame(y, bits), bits)
        assert o.shape == (48 * scale, 72 * scale, 3) and o.dtype == f.dtype
        assert np.array_equal(o, want), i


@pytest.mark.parametrize("in_bits,out_bits", [(16, 8), (8, 16)])
def test_stream_keeps_the_sources_depth_when_the_output_depth_differs(ctx_case, in_bits, out_bits):
    """A 10-bit source written to an 8-bit pixel format (and the reverse): the model sees x / 65535 (x / 255), as in the
    reference's callback — only the output is quantised to the pixel format's depth.  The depth may change mid-stream."""
    from nunif_amd.iw3 import _ops
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    ctx, method, noise_level, scale = ctx_case
    frames = _frames(5, 48, 72, in_bits) + _frames(2, 48, 72, out_bits)
    stream = Waifu2xVideoStream(ctx, _args(method, noise_level, pix_fmt="yuv420p10le" if out_bits == 16 else "yuv420p"), DEV)
    outs = _run(stream, frames)
    assert len(outs) == 7
    for i, (f, o) in enumerate(zip(frames, outs)):
        t = torch.from_numpy(f.view(np.int16) if f.dtype == np.uint16 else f).to(DEV)
        y, _ = ctx.convert(_ops.frame_to_tensor(t), None, method, noise_level, 64, 4, False, enable_amp=True, output_device=DEV)
        assert o.dtype == (np.uint16 if out_bits == 16 else np.uint8)
        assert np.array_equal(o, _frame_np(_ops.to_frame(y, out_bits), out_bits)), i
    assert Waifu2xVideoStream(ctx, _args(method, noise_level), DEV, use_16bit=True).bits == 16


def test_stream_with_grain_is_repeatable_and_differs(ctx_case):
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    ctx, method, noise_level, scale = ctx_case
    frames = _frames(12, 48, 72)
    plain = _run(Waifu2xVideoStream(ctx, _args(method, noise_level), DEV), frames)
    torch.manual_seed(77)
    a = _run(Waifu2xVideoStream(ctx, _args(method, noise_level, grain=True), DEV), frames)
    torch.manual_seed(77)
    b = _run(Waifu2xVideoStream(ctx, _args(method, noise_level, grain=True), DEV), frames)
    torch.manual_seed(78)
    c = _run(Waifu2xVideoStream(ctx, _args(method, noise_level, grain=True), DEV), frames)
    assert len(a) == len(b) == len(plain) == 12
    for i in range(12):
        assert np.array_equal(a[i], b[i]), i
        assert not np.array_equal(a[i], plain[i]) and not np.array_equal(a[i], c[i]), i
        assert np.abs(a[i].astype(np.int64) - plain[i].astype(np.int64)).mean() < 16       # grain, not garbage
    assert not np.array_equal(a[0].astype(np.int64) - plain[0], a[1].astype(np.int64) - plain[1])


def test_stream_rotation_and_a_frame_size_change(ctx_case):
    from nunif_amd.iw3 import _ops
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    ctx, method, noise_level, scale = ctx_case
    frames = _frames(5, 48, 72) + _frames(4, 40, 64)
    for key, turns in (("rotate_left", 1), ("rotate_right", 3)):
        stream = Waifu2xVideoStream(ctx, _args(method, noise_level, **{key: True}), DEV)
        outs = _run(stream, frames)
        assert len(outs) == 9
        for i, (f, o) in enumerate(zip(frames, outs)):
            h, w = f.shape[:2]
            assert o.shape == (w * scale, h * scale, 3), i
            x = torch.rot90(_ops.frame_to_tensor(torch.from_numpy(f).to(DEV)), turns, (-2, -1)).contiguous()
            y, _ = ctx.convert(x, None, method, noise_level, 64, 4, False, enable_amp=True, output_device=DEV)
            assert np.array_equal(o, _ops.to_frame(y, 8).cpu().numpy()), (key, i)
