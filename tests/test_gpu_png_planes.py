"""The plane forms of the PNG frame encoder (RGBA 8, grey 8, grey + alpha 8: nunif_amd/csrc/png_planes.hip and png.hip) on the GPU
against tests/png_ref_planes.py: the body equals the restatement's byte for byte and PIL decodes the file to exactly the quantised
pixels, at the shapes where lanes and 16-byte groups straddle the row end at every pixel size, across stripe boundaries, at the
longest row and the most stripes, for noise, gradient, constant colour under alpha = 1, an alpha checkerboard and out-of-range
inputs, from one and from three colour planes for the grey forms; the filtered bytes and the filter choice; batches, calls,
streams, workspace reuse across forms, the capacity rule; and the old forms through the same encoder object."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as R
import png_ref_planes as RP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (form, colour planes)
CASES = [(RP.RGBA8_F32, 3), (RP.GRAY8_F32, 3), (RP.GRAY8_F32, 1), (RP.GRAYA8_F32, 3), (RP.GRAYA8_F32, 1)]
IDS = ["rgba", "gray3", "gray1", "graya3", "graya1"]
KINDS = ["noise", "gradient", "constant_opaque", "alpha_checker", "out_of_range"]


@pytest.fixture(scope="module")
def enc(hiplib):
    from nunif_amd.nunif.utils.png import PngEncoder
    return PngEncoder(DEV)


def make_input(kind, form, channels, H, W, seed=0):
    """-> (colour f32 [channels,H,W], alpha f32 [1,H,W] or None)"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    c = channels
    alpha = rng.random((1, H, W), dtype=np.float32)
    if kind == "noise":
        x = rng.random((c, H, W), dtype=np.float32)
    elif kind == "gradient":
        x = np.stack([(xx * (k + 1) + yy * 2) / float((W * (k + 1) + H * 2)) for k in range(c)]).astype(np.float32)
        alpha = ((xx + 2 * yy) / float(W + 2 * H))[None].astype(np.float32)
    elif kind == "constant_opaque":                                       # the common case: runs of 258 at the pixel distance
        x = np.stack([np.full((H, W), v, np.float32) for v in (0.4, 0.7, 0.1)[:c]])
        alpha = np.ones((1, H, W), np.float32)
    elif kind == "alpha_checker":
        x = rng.random((c, H, W), dtype=np.float32)
        alpha = ((xx + yy) & 1)[None].astype(np.float32)
    else:                                                                 # the clamp: below 0 and above 1, no NaN
        x = (rng.random((c, H, W), dtype=np.float32) * 3 - 1).astype(np.float32)
        alpha = (rng.random((1, H, W), dtype=np.float32) * 3 - 1).astype(np.float32)
    return np.ascontiguousarray(x), (np.ascontiguousarray(alpha) if RP.HAS_ALPHA[form] else None)


def dev(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


def check_frame(enc, colour, alpha, form, stripe_rows, codes=False):
    """Every check of one frame; returns the file."""
    from nunif_amd.nunif.utils import png as P
    gray = form != RP.RGBA8_F32
    cd, ad = dev(colour), dev(alpha)
    H, W = colour.shape[1:]
    S = min(stripe_rows, H)
    want_filtered = RP.filtered(colour, alpha, form)
    got_filtered = P.debug_filtered(cd, alpha=ad, gray=gray)[0].cpu().numpy()
    assert got_filtered.shape == want_filtered.shape
    assert np.array_equal(got_filtered[:, 0], want_filtered[:, 0]), "filter choice"
    assert np.array_equal(got_filtered, want_filtered)
    if codes and colour.shape[0] == (3 if form == RP.RGBA8_F32 else 1):
        hist, lens = (t[0].cpu().numpy() for t in P.debug_codes(cd, S, alpha=ad, gray=gray))
        for k, sc in enumerate(RP.stripe_codes(colour, alpha, form, S)):
            assert hist[k].tolist() == sc.hist(), ("histogram", k)
            assert lens[k].tolist() == sc.lengths(), ("code lengths", k)
    text = {"note": "x"}
    data = enc.encode(cd, text=text, stripe_rows=S, alpha=ad, gray=gray, gamma=50000)
    head = RP.header(H, W, form, text, 50000)
    assert data[:len(head)] == head
    body, want = data[len(head):], RP.body(colour, alpha, form, S)
    assert len(body) == len(want) and body == want, (H, W, form, S)
    assert len(body) <= P.max_bytes(H, W, form, S) == RP.max_bytes(H, W, form, S)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == RP.PIL_MODE[form] and im.size == (W, H)
    assert np.array_equal(np.asarray(im), RP.pixels(colour, alpha, form))
    assert im.text == text and im.info["gamma"] == 0.5
    return data


@pytest.mark.parametrize("form,channels", CASES, ids=IDS)
def test_shapes_and_stripes_match_the_restatement(enc, form, channels):
    shapes = [(1, 1), (1, 2), (2, 1), (3, 5), (16, 16), (33, 47), (8, 63), (8, 64), (8, 65), (64, 96)]
    for H, W in shapes:
        for S in sorted({1, 3, 16, H}):
            if S <= H:
                check_frame(enc, *make_input("noise", form, channels, H, W), form, S, codes=(H, W) in ((3, 5), (33, 47)))
    for H in (15, 16, 17):                                                # H = 16 - 1, 16, 16 + 1 at stripe_rows 16
        check_frame(enc, *make_input("noise", form, channels, H, 21), form, 16)


@pytest.mark.parametrize("form,channels", CASES, ids=IDS)
def test_inputs_match_the_restatement(enc, form, channels):
    for kind in KINDS:
        for H, W, S in [(17, 33, 3), (64, 96, 16), (40, 350, 40)]:                    # the last: a stripe of several passes
            check_frame(enc, *make_input(kind, form, channels, H, W), form, S, codes=(H == 17))


def test_a_constant_opaque_frame_is_runs_of_258_at_distance_4(enc):
    colour, alpha = make_input("constant_opaque", RP.RGBA8_F32, 3, 4, 300)
    toks = R.tokens(RP.filtered(colour, alpha, RP.RGBA8_F32).reshape(-1), 4)
    assert (258, 4) in toks and all(t[1] == 4 for t in toks if len(t) == 2)
    check_frame(enc, colour, alpha, RP.RGBA8_F32, 4, codes=True)
    colour, _ = make_input("constant_opaque", RP.GRAY8_F32, 1, 4, 300)
    toks = R.tokens(RP.filtered(colour, None, RP.GRAY8_F32).reshape(-1), 1)
    assert (258, 1) in toks
    check_frame(enc, colour, None, RP.GRAY8_F32, 4, codes=True)


def test_the_size_limits(enc):
    f = RP.RGBA8_F32
    check_frame(enc, *make_input("noise", f, 3, 1, 8192), f, 1)           # the longest row: 32 769 filtered bytes
    check_frame(enc, *make_input("gradient", f, 3, 8192, 1), f, 1)        # the most stripes
    check_frame(enc, *make_input("alpha_checker", f, 3, 8192, 1), f, 8192)


def test_batch_calls_streams_and_workspace_reuse(enc):
    from nunif_amd.nunif.utils.png import PngEncoder
    for form, channels in CASES:
        gray = form != RP.RGBA8_F32
        xs = [make_input(kind, form, channels, 33, 47, seed=k) for k, kind in enumerate(["noise", "gradient", "constant_opaque"])]
        colour = dev(np.stack([c for c, _ in xs]))
        alpha = dev(np.stack([a for _, a in xs])) if RP.HAS_ALPHA[form] else None
        together = enc.encode(colour, stripe_rows=5, alpha=alpha, gray=gray)
        assert len(together) == 3
        for k, (c, a) in enumerate(xs):
            single = enc.encode(dev(c), stripe_rows=5, alpha=dev(a), gray=gray)
            assert single == together[k] == RP.encode(c, a, form, 5)
        assert enc.encode(colour, stripe_rows=5, alpha=alpha, gray=gray) == together              # a second call
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            other = PngEncoder(DEV).encode(colour, stripe_rows=5, alpha=alpha, gray=gray)
        side.synchronize()
        assert other == together
    # the same encoder and workspace across forms and shapes, larger and smaller again
    for (form, channels), (H, W) in zip(CASES, [(9, 11), (70, 130), (5, 3), (40, 20), (7, 7)]):
        check_frame(enc, *make_input("noise", form, channels, H, W), form, 4)


def test_the_old_forms_through_the_same_encoder(enc):
    """The calls of tests/test_gpu_png.py's kind between calls of the new forms: the same bytes as png_ref.encode."""
    rng = np.random.default_rng(9)
    for H, W, S in [(17, 33, 3), (64, 96, 16)]:
        check_frame(enc, *make_input("noise", RP.RGBA8_F32, 3, H, W), RP.RGBA8_F32, S)
        rgb = rng.random((3, H, W), dtype=np.float32)
        u8 = np.ascontiguousarray(R.quantise(rgb, R.RGB8_F32).reshape(H, W, 3))
        grey = rng.random((1, H, W), dtype=np.float32)
        for x, form in [(rgb, R.RGB8_F32), (u8, R.RGB8_U8), (grey, R.GRAY16_F32)]:
            text = {"iw3_min_depth_value": 0.25}
            assert enc.encode(torch.from_numpy(x).to(DEV), text=text, stripe_rows=S) == R.encode(x, form, S, text)
        check_frame(enc, *make_input("noise", RP.GRAY8_F32, 1, H, W), RP.GRAY8_F32, S)
    # gamma alone changes the header of an old form and nothing else
    x = rng.random((3, 9, 13), dtype=np.float32)
    assert enc.encode(torch.from_numpy(x).to(DEV), gamma=45455) == RP.header(9, 13, R.RGB8_F32, None, 45455) + R.body(x, R.RGB8_F32, 9)


def test_capacity_one_byte_short(enc):
    form = RP.RGBA8_F32
    colour, alpha = make_input("noise", form, 3, 20, 30)
    want = RP.body(colour, alpha, form, 8)
    cd, ad = dev(colour).unsqueeze(0).contiguous(), dev(alpha).unsqueeze(0).contiguous()
    for capacity, fits in [(len(want), True), (len(want) - 1, False)]:
        e = type(enc)(DEV)
        e._out = torch.full((capacity + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        out, cap, lens = e.encode_device(cd, form, 8, capacity=capacity, alpha=ad)
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert (host[capacity:] == 0xA5).all()                                                    # the guard bytes
        if fits:
            assert lens.cpu().tolist() == [len(want)] and host[:capacity].tobytes() == want
        else:
            assert lens.cpu().tolist() == [-1] and (host == 0xA5).all()


def test_refused_arguments(enc, hiplib):
    import ctypes
    x = torch.zeros(1, 3, 4, 4, device=DEV)
    a = torch.ones(1, 1, 4, 4, device=DEV)
    buf = torch.zeros(8192, dtype=torch.uint8, device=DEV)
    lens = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                                   # noqa: E731
    planes, single = hiplib.nunif_hip_png_encode_planes, hiplib.nunif_hip_png_encode
    assert planes(p(x), p(a), 3, 4, 1, 4, 4, 4, p(buf), 2048, p(lens), p(buf), None) == 0
    torch.cuda.synchronize()
    # form 3, an old form, a form without its alpha, alpha where the form has none, one colour plane for RGBA, two planes
    for alpha, channels, form in [(p(a), 3, 3), (p(a), 3, 0), (None, 3, 4), (p(a), 3, 5), (p(a), 1, 4), (p(a), 2, 6)]:
        assert planes(p(x), alpha, channels, form, 1, 4, 4, 4, p(buf), 2048, p(lens), p(buf), None) != 0
    for form in (3, 4, 5, 6):                                                                     # the entry with one pointer
        assert single(p(x), form, 1, 4, 4, 4, p(buf), 2048, p(lens), p(buf), None) != 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.zeros(3, 4, 4), alpha=torch.ones(1, 4, 4))
    with pytest.raises(RuntimeError):
        enc.encode(x[0], alpha=torch.ones(1, 4, 4))                                               # alpha on another device
    with pytest.raises(ValueError):
        enc.encode(x[0], alpha=torch.ones(1, 4, 5, device=DEV))                                   # another H x W
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV), alpha=a[0])               # a uint8 frame
