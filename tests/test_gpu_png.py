"""The PNG frame encoder (nunif_amd/csrc/png.hip) on the GPU against tests/png_ref.py: the body equals the restatement's byte for
byte and the file decodes with PIL to exactly the quantised input, for the three pixel forms, at the shapes where the kernels take
another path (one pixel, a row shorter than a match, several stripes, a stripe of several passes, the size limits), for
stripe_rows 1 / 3 / 16 / H and constant, noise, gradient, pixel-checker, out-of-range and crafted inputs; the filtered bytes and
the code lengths equal the restatement's; determinism across calls, streams and batching; workspace reuse; the capacity rule;
``ExportWriter`` end to end."""
import ctypes
import io
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = [R.RGB8_F32, R.RGB8_U8, R.GRAY16_F32]
SHAPES = [(1, 1), (1, 7), (3, 5), (8, 8), (17, 33), (64, 96), (15, 21), (16, 21), (17, 21)]       # the last three: H = 16 - 1, 16, 16 + 1
KINDS = ["constant", "noise", "gradient", "checker", "out_of_range"]


@pytest.fixture(scope="module")
def enc(hiplib):
    from nunif_amd.nunif.utils.png import PngEncoder
    return PngEncoder(DEV)


def make_input(kind, form, H, W, seed=0):
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    c = 1 if form == R.GRAY16_F32 else 3
    if kind == "constant":
        x = np.full((c, H, W), 0.4, np.float32)
    elif kind == "noise":
        x = rng.random((c, H, W), dtype=np.float32)
    elif kind == "gradient":
        x = np.stack([(xx * (k + 1) + yy * 2) / float((W * (k + 1) + H * 2)) for k in range(c)]).astype(np.float32)
    elif kind == "checker":
        x = np.stack([((xx + yy + k) & 1) for k in range(c)]).astype(np.float32)
    else:
        x = (rng.random((c, H, W), dtype=np.float32) * 3 - 1).astype(np.float32)
    if form == R.RGB8_U8:
        return np.ascontiguousarray(R.quantise(x, R.RGB8_F32).reshape(H, W, 3))
    return x


def check_frame(enc, x, form, stripe_rows, codes=True):
    """Every check of one frame; returns the file."""
    from nunif_amd.nunif.utils import png as P
    xd = torch.from_numpy(x).to(DEV)
    raw = R.quantise(x, form)
    H, W = raw.shape[0], raw.shape[1] // R.BPP[form]
    S = min(stripe_rows, H)
    want_filtered = R.filter_rows(raw, R.BPP[form])
    got_filtered = P.debug_filtered(xd)[0].cpu().numpy()
    assert np.array_equal(got_filtered[:, 0], want_filtered[:, 0]), "filter choice"
    assert np.array_equal(got_filtered, want_filtered)
    if codes:
        hist, lens = (t[0].cpu().numpy() for t in P.debug_codes(xd, S))
        for k, sc in enumerate(R.stripe_codes(x, form, S)):
            assert hist[k].tolist() == sc.hist(), ("histogram", k)
            assert lens[k].tolist() == sc.lengths(), ("code lengths", k)
    text = {"iw3_min_depth_value": 0.25, "note": "x"}
    data = enc.encode(xd, text=text, stripe_rows=S)
    head = R.header(H, W, form, text)
    assert data[:len(head)] == head
    body, want = data[len(head):], R.body(x, form, S)
    assert len(body) == len(want) and body == want, (H, W, form, S)
    assert len(body) <= P.max_bytes(H, W, form, S) == R.max_bytes(H, W, form, S)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (W, H) and np.array_equal(np.asarray(im), R.pixels(x, form))
    assert im.text == {k: str(v) for k, v in text.items()}
    return data


@pytest.mark.parametrize("form", FORMS)
def test_shapes_and_stripes_match_the_restatement(enc, form):
    for H, W in SHAPES:
        for S in sorted({1, 3, 16, H}):
            if S <= H:
                check_frame(enc, make_input("noise", form, H, W), form, S)


@pytest.mark.parametrize("form", FORMS)
def test_inputs_match_the_restatement(enc, form):
    for kind in KINDS:
        if kind == "out_of_range" and form == R.RGB8_U8:
            continue
        for H, W, S in [(17, 33, 3), (64, 96, 16), (40, 350, 40)]:                    # the last: a stripe of four passes
            check_frame(enc, make_input(kind, form, H, W), form, S)


@pytest.mark.parametrize("form", FORMS)
def test_the_size_limits(enc, form):
    check_frame(enc, make_input("noise", form, 1, 8192), form, 1, codes=False)
    check_frame(enc, make_input("gradient", form, 8192, 1), form, 8192, codes=False)
    check_frame(enc, make_input("checker", form, 8192, 1), form, 16, codes=False)


def test_crafted_stripes(enc):
    f = R.fibonacci_frame()
    sc = R.stripe_codes(f, R.RGB8_U8, 8)[0]
    assert max(R.unlimited_depths(sc.lit_hist).values()) > 15 and max(sc.lit_len) == 15          # the limiter runs
    check_frame(enc, f, R.RGB8_U8, 8)
    black = np.zeros((4, 9, 3), np.uint8)
    sc = R.stripe_codes(black, R.RGB8_U8, 4)[0]
    assert [s for s in range(256) if sc.lit_hist[s]] == [0]                                        # one distinct literal
    check_frame(enc, black, R.RGB8_U8, 4)
    for x, S, run in R.run_frames():
        toks = R.tokens(R.filter_rows(R.quantise(x, R.GRAY16_F32), 2)[:S].reshape(-1), 2)
        assert sum(t[0] if len(t) == 2 else 1 for t in toks[2:]) == run and toks[2] == (258, 2)
        check_frame(enc, x, R.GRAY16_F32, S)


def test_batch_calls_streams_and_workspace_reuse(enc):
    from nunif_amd.nunif.utils.png import PngEncoder
    for form in FORMS:
        xs = [make_input(kind, form, 33, 47, seed=k) for k, kind in enumerate(["noise", "gradient", "constant"])]
        batch = torch.from_numpy(np.stack(xs)).to(DEV)
        together = enc.encode(batch, stripe_rows=5)
        assert len(together) == 3
        for k, x in enumerate(xs):
            single = enc.encode(torch.from_numpy(x).to(DEV), stripe_rows=5)
            assert single == together[k] == R.encode(x, form, 5)
        assert enc.encode(batch, stripe_rows=5) == together                                       # a second call
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            other = PngEncoder(DEV).encode(batch, stripe_rows=5)
        side.synchronize()
        assert other == together
    # the same encoder across a shape change, larger and smaller again
    for H, W in [(9, 11), (70, 130), (5, 3)]:
        check_frame(enc, make_input("noise", R.RGB8_F32, H, W), R.RGB8_F32, 4, codes=False)


def test_capacity_one_byte_short(enc):
    x = make_input("noise", R.RGB8_F32, 20, 30)
    want = R.body(x, R.RGB8_F32, 8)
    xd = torch.from_numpy(x).to(DEV).unsqueeze(0).contiguous()
    for capacity, fits in [(len(want), True), (len(want) - 1, False)]:
        e = type(enc)(DEV)
        e._out = torch.full((capacity + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        out, cap, lens = e.encode_device(xd, R.RGB8_F32, 8, capacity=capacity)
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert (host[capacity:] == 0xA5).all()                                                    # the guard bytes
        if fits:
            assert lens.cpu().tolist() == [len(want)] and host[:capacity].tobytes() == want
        else:
            assert lens.cpu().tolist() == [-1] and (host == 0xA5).all()


def test_refused_arguments(enc, hiplib):
    from nunif_amd import _hip
    from nunif_amd.nunif.utils import png as P
    assert P.max_bytes(8193, 8, 0) == -1 and P.workspace_bytes(17, 8, 8, 0) == -1
    x = torch.zeros(1, 3, 4, 4, device=DEV)
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    lens = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                                   # noqa: E731
    for form, S in [(3, 1), (0, 0), (0, 5)]:
        assert hiplib.nunif_hip_png_encode(p(x), form, 1, 4, 4, S, p(buf), 1024, p(lens), p(buf), None) != 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.zeros(3, 4, 4))
    assert _hip is not None


def test_export_writer(enc, tmp_path):
    from nunif_amd.iw3 import _ops
    from nunif_amd.iw3.base_depth_model import BaseDepthModel
    from nunif_amd.iw3.export import ExportWriter, encode_normalized_depth
    from nunif_amd.iw3.mapper import get_mapper
    g = torch.Generator().manual_seed(5)
    frames = [torch.randint(0, 256, (36, 50, 3), dtype=torch.uint8, generator=g) for _ in range(5)]
    depths = [torch.rand(1, 18, 26, generator=g).to(DEV) for _ in range(5)]
    pts = [0, 512, 1024, 99999999, 123456789]

    def run(name, **flags):
        args = SimpleNamespace(export_disparity=False, mapper="pow2", export_depth_fit=False, export_depth_only=False)
        args.__dict__.update(flags)
        rgb_dir, depth_dir = tmp_path / name / "rgb", tmp_path / name / "depth"
        os.makedirs(rgb_dir)
        os.makedirs(depth_dir)
        with ThreadPoolExecutor(max_workers=2) as pool:
            w = ExportWriter(str(rgb_dir), str(depth_dir), pool, args)
            for lo, hi in [(0, 2), (2, 4), (4, 5)]:
                w.write(frames[lo:hi], depths[lo:hi], pts[lo:hi], min_depth_value=0.5, max_depth_value=20)
            w.drain()
        return rgb_dir, depth_dir, args

    def truncated(d):
        return torch.clamp((0xffff * torch.clamp(d, 0, 1)).to(torch.int32).float().cpu() / 0xffff, 0, 1)

    names = sorted(str(p).zfill(8) + ".png" for p in pts)
    rgb_dir, depth_dir, _ = run("plain")
    assert sorted(os.listdir(rgb_dir)) == names and sorted(os.listdir(depth_dir)) == names
    for k, p in enumerate(pts):
        name = str(p).zfill(8) + ".png"
        depth, meta = BaseDepthModel.load_depth(str(depth_dir / name))
        assert float(meta["iw3_min_depth_value"]) == 0.5 and float(meta["iw3_max_depth_value"]) == 20.0
        assert torch.equal(depth, truncated(depths[k]) * (20.0 - 0.5) + 0.5)
        assert np.array_equal(np.asarray(Image.open(str(rgb_dir / name))), frames[k].numpy())
    rgb_dir, depth_dir, _ = run("disparity", export_disparity=True)
    with Image.open(str(depth_dir / names[0])) as im:
        want = (0xffff * torch.clamp(get_mapper("pow2")(depths[0]), 0, 1)).to(torch.int32).cpu().numpy()[0]
        assert np.array_equal(np.asarray(im).astype(np.int32), want)
    rgb_dir, depth_dir, _ = run("fit", export_depth_fit=True)
    with Image.open(str(depth_dir / names[0])) as im:
        fit = _ops.resize_aa(depths[0].unsqueeze(0), (36, 50), mode="bilinear", align_corners=False)[0]
        want = (0xffff * torch.clamp(fit, 0, 1)).to(torch.int32).cpu().numpy()[0]
        assert im.size == (50, 36) and np.array_equal(np.asarray(im).astype(np.int32), want)
    rgb_dir, depth_dir, _ = run("depth_only", export_depth_only=True)
    assert os.listdir(rgb_dir) == [] and sorted(os.listdir(depth_dir)) == names
    one = encode_normalized_depth(depths[1], {"a": 1}, min_depth_value=0.0)
    with Image.open(io.BytesIO(one)) as im:
        assert im.text == {"a": "1", "iw3_min_depth_value": "0.0"}
        assert np.array_equal(np.asarray(im), R.pixels(depths[1].cpu().numpy(), R.GRAY16_F32))
