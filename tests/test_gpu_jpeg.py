"""The baseline JPEG encoder (nunif_amd/csrc/jpeg.hip) on the GPU against tests/jpeg_ref.py:

coefficients equal the float64 statement except inside the tie band (the fp32 restatement's largest deviation of c / Q on the same
input times jpeg_ref.BAND_MARGIN), and then differ by exactly 1; the stream equals the restatement's header plus entropy coder
run on the device's own coefficients, byte for byte; PIL decodes every stream, its PSNR to the uint8 input is not below libjpeg's
by more than the restatement's own gap plus 0.1 dB and its size is within 2 % of the restatement's ratio to libjpeg's;
determinism across calls, streams and batching; workspace reuse; the capacity rule; ``to_jpeg_data``; end to end."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_ref as J
from conftest import synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(8, 8), (16, 16), (17, 23), (40, 56), (33, 130), (64, 96)]
QUALITIES = [1, 50, 90, 100]
RESTARTS = [1, 3, 8, "row"]


@pytest.fixture(scope="module")
def enc(hiplib):
    from nunif_amd.nunif.utils.jpeg import JpegEncoder
    return JpegEncoder(DEV)


def restart_of(r, W, ss):
    return J.whole_row(W, ss) if r == "row" else r


def check_frame(enc, x, quality, ss, restart, decode=True):
    """Every check of one frame x [3,H,W] (numpy fp32); returns the stream."""
    from nunif_amd.nunif.utils.jpeg import debug_coefficients
    _, H, W = x.shape
    xd = torch.from_numpy(x).to(DEV)
    coef = debug_coefficients(xd, quality, str(ss))[0].cpu().numpy().astype(np.int64)
    a = J.coefficient_agreement(coef, x, quality, ss)
    print(f"{H}x{W} q{quality} {ss} r{restart}: band {a['band']:.3e} (fp32 deviation {a['fp32_deviation']:.3e} x {a['margin']:g}), "
          f"{a['in_band']} of {a['coefficients']} in band, {a['mismatches']} mismatches, {a['bad']} bad")
    assert a["band"] <= J.BAND_CEILING and a["margin"] == 4.0
    assert a["bad"] == 0 and a["mismatches"] <= a["in_band"], a
    stream = enc.encode(xd, quality=quality, subsampling=str(ss), restart_mcus=restart)
    want = J.stream_from_coefficients(coef, H, W, quality, ss, restart)
    assert len(stream) == len(want) and stream == want
    assert len(stream) <= J.max_bytes(H, W, ss, restart)
    if decode:
        im = J.pil_decode(stream)
        assert im.size == (W, H) and im.mode == "RGB"
        y = J.yardstick(x, quality, ss, restart)
        got = J.psnr_u8(np.asarray(im), y["u8"])
        margin = max(y["psnr_lib"] - y["psnr_ref"], 0.0) + 0.1
        ratio, mine = y["size_ref"] / y["size_lib"], len(stream) / y["size_lib"]
        print(f"    PSNR {got:.3f} dB, libjpeg {y['psnr_lib']:.3f}, restatement {y['psnr_ref']:.3f}; size / libjpeg {mine:.4f}, "
              f"restatement {ratio:.4f}")
        assert got >= y["psnr_lib"] - margin
        assert ratio * 0.98 <= mine <= ratio * 1.02
    return stream


@pytest.mark.parametrize("ss", [420, 444])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_seeded_content(enc, si, ss):
    h, w = SHAPES[si]
    x = J.synth(20 + si, h, w)
    for k, quality in enumerate(QUALITIES):                       # every quality on every shape, the restart layouts rotating
        check_frame(enc, x, quality, ss, restart_of(RESTARTS[(k + si) % 4], w, ss))


@pytest.mark.parametrize("shape,ss,quality,restart", [((1, 8192), 420, 50, 8), ((1, 8192), 444, 90, "row"),
                                                      ((8192, 1), 420, 90, 3), ((8192, 1), 444, 100, 1)])
def test_the_limits(enc, shape, ss, quality, restart):
    x = J.synth(31, *shape)
    check_frame(enc, x, quality, ss, restart_of(restart, shape[1], ss))


@pytest.mark.parametrize("ss", [420, 444])
@pytest.mark.parametrize("name,quality", [("constant", 50), ("noise", 100), ("blocks", 100), ("pixels", 100), ("pixels", 1),
                                          ("clamp", 90)])
def test_crafted_inputs(enc, name, quality, ss):
    check_frame(enc, J.crafted(name, 40, 56), quality, ss, 3)
    check_frame(enc, J.crafted(name, 40, 56), quality, ss, 1, decode=False)


def test_refused_arguments(enc):
    from nunif_amd import _hip
    x = torch.rand(3, 16, 16, device=DEV)
    with pytest.raises(RuntimeError):
        enc.encode(x.cpu())
    with pytest.raises(ValueError):
        enc.encode(torch.rand(4, 16, 16, device=DEV))
    with pytest.raises(_hip.NunifHipError):
        enc.encode(x, quality=0)
    with pytest.raises(KeyError):
        enc.encode(x, subsampling="422")
    with pytest.raises(ValueError):
        enc.encode(x, restart_mcus=0)
    with pytest.raises(ValueError):
        enc.encode(torch.rand(17, 3, 16, 16, device=DEV))


def test_determinism_streams_and_batch(enc):
    from nunif_amd.nunif.utils.jpeg import JpegEncoder
    frames = [J.synth(40 + i, 33, 130) for i in range(3)]
    xd = [torch.from_numpy(f).to(DEV) for f in frames]
    single = [enc.encode(x, quality=90, restart_mcus=3) for x in xd]
    assert [enc.encode(x, quality=90, restart_mcus=3) for x in xd] == single
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = [JpegEncoder(DEV).encode(x, quality=90, restart_mcus=3) for x in xd]
    side.synchronize()
    assert other == single
    batch = enc.encode(torch.stack(xd), quality=90, restart_mcus=3)
    assert isinstance(batch, list) and batch == single


def test_workspace_reuse_across_sizes(enc):
    from nunif_amd.nunif.utils.jpeg import JpegEncoder
    one = JpegEncoder(DEV)
    for (h, w), ss in (((64, 96), "420"), ((17, 23), "444"), ((40, 56), "420"), ((64, 96), "444")):
        x = torch.from_numpy(J.synth(50, h, w)).to(DEV)
        assert one.encode(x, quality=50, subsampling=ss, restart_mcus=8) == \
            JpegEncoder(DEV).encode(x, quality=50, subsampling=ss, restart_mcus=8)


def raw_encode(x, quality, ss, restart, capacity, guard=64):
    """The C entry on buffers of the test's own: (slots + guard as numpy, lengths)."""
    from nunif_amd import _hip
    B, _, H, W = x.shape
    out = torch.full((B * capacity + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lens = torch.zeros(B, dtype=torch.int32, device=DEV)
    work = torch.empty(_hip.lib().nunif_hip_jpeg_workspace_bytes(B, H, W, ss, restart), dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                   # noqa: E731
    _hip.check(_hip.lib().nunif_hip_jpeg_encode(p(x), B, H, W, quality, ss, restart, p(out), capacity, p(lens), p(work),
                                                _hip.current_stream_ptr(DEV)))
    return out.cpu().numpy(), lens.cpu().tolist()


def test_capacity(enc):
    a, b = J.synth(60, 40, 56), J.crafted("noise", 40, 56)
    xa, xb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    sa, sb = (enc.encode(x, quality=90, restart_mcus=3) for x in (xa, xb))
    assert len(sa) < len(sb)
    x = torch.stack([xa, xb, xa]).contiguous()
    n = len(sb)
    out, lens = raw_encode(x, 90, 420, 3, n)                      # exactly the longest stream: all three fit
    assert lens == [len(sa), n, len(sa)]
    assert out[:len(sa)].tobytes() == sa and out[n:2 * n].tobytes() == sb and out[2 * n:2 * n + len(sa)].tobytes() == sa
    assert (out[len(sa):n] == 0xA5).all() and (out[2 * n + len(sa):] == 0xA5).all()
    out, lens = raw_encode(x, 90, 420, 3, n - 1)                  # one byte short for the middle frame alone
    assert lens == [len(sa), -1, len(sa)]
    assert out[:len(sa)].tobytes() == sa and (out[n - 1:2 * (n - 1)] == 0xA5).all()
    assert out[2 * (n - 1):2 * (n - 1) + len(sa)].tobytes() == sa and (out[2 * (n - 1) + len(sa):] == 0xA5).all()
    out, lens = raw_encode(x, 90, 420, 3, 100)                    # not even the header
    assert lens == [-1, -1, -1] and (out == 0xA5).all()


def test_to_jpeg_data(enc):
    from nunif_amd.iw3.desktop.utils import to_jpeg_data, to_uint8
    x = torch.from_numpy(J.synth(70, 64, 96)).to(DEV)
    data, tick = to_jpeg_data(x, 90, 1234)
    assert tick == 1234 and isinstance(data, bytes) and data == enc.encode(x, quality=90)
    assert J.pil_decode(data).size == (96, 64)
    host, tick = to_jpeg_data(x, 90, 5, gpu_jpeg=False)
    assert tick == 5 and b"\xff\xdd" not in host[:700] and b"\xff\xdd" in data[:700]      # libjpeg writes no DRI here
    assert to_jpeg_data(x.cpu(), 90, 5)[0] == host
    u8 = to_uint8(x).cpu().permute(1, 2, 0).numpy()
    assert np.array_equal(u8, J.u8_image(x.cpu().numpy()))
    assert J.pil_decode(host).size == (96, 64)


def test_end_to_end_process_image(enc):
    from nunif_amd.iw3.base_depth_model import CallableDepthModel
    from nunif_amd.iw3.desktop.utils import to_jpeg_data
    from nunif_amd.iw3.utils import process_image
    net = lambda t: t.mean(1) + 0.3 * t[:, 0]                              # noqa: E731
    model = CallableDepthModel(net, lower_bound=56).load(gpu=0)
    x = synth_image(97, 3, 64, 96).to(DEV)
    args = SimpleNamespace(mapper="mul_1", convergence=0.5, divergence=3.0, method="forward_fill", synthetic_view="both",
                           edge_dilation=2, tta=False)
    sbs = process_image(x, args, model)
    assert sbs.shape == (3, 64, 192)
    data, tick = to_jpeg_data(sbs, 90, 7)
    from nunif_amd.nunif.utils.jpeg import DEFAULT_RESTART_MCUS
    assert tick == 7 and data == check_frame(enc, sbs.cpu().numpy(), 90, 420, DEFAULT_RESTART_MCUS)
