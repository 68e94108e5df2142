"""The PNG frame encoder without a GPU: tests/png_ref.py, the restatement the device has to equal byte for byte, is a PNG encoder
in its own right.  Its files decode with PIL to exactly the quantised pixels, its zlib body inflates to the filtered bytes, its
CRCs and Adler-32 are zlib's, its header is what PIL writes; the bound of nunif_amd/csrc/png_host.h (through the C ABI) holds on
adversarial inputs; the crafted inputs exercise what they are meant to; and its size stays at the recorded ratio to libpng's."""
import io
import os
import zlib

import numpy as np
import pytest
from PIL import Image
from PIL.PngImagePlugin import PngInfo

import png_ref as R
from conftest import synth_image
from nunif_amd.nunif.utils import png as P

FORMS = [R.RGB8_F32, R.RGB8_U8, R.GRAY16_F32]


def frame(form, H, W, seed=0, kind="noise"):
    rng = np.random.default_rng(seed)
    c = 1 if form == R.GRAY16_F32 else 3
    x = rng.random((c, H, W), dtype=np.float32) * (1.4 if kind == "wide" else 1.0) - (0.2 if kind == "wide" else 0.0)
    if form == R.RGB8_U8:
        return np.ascontiguousarray(R.quantise(x, R.RGB8_F32).reshape(H, W, 3))
    return x.astype(np.float32)


def pil_bytes(pix, level, text=None):
    info = PngInfo()
    for k, v in (text or {}).items():
        info.add_text(k, str(v))
    buf = io.BytesIO()
    Image.fromarray(pix).save(buf, format="png", compress_level=level, pnginfo=info)
    return buf.getvalue()


@pytest.mark.parametrize("form", FORMS)
def test_files_decode_to_the_quantised_pixels_and_the_body_is_zlib(form):
    for (H, W), S in [((1, 1), 1), ((1, 7), 1), ((3, 5), 2), ((17, 33), 3), ((17, 33), 17), ((64, 96), 16)]:
        for kind in ("noise", "wide"):
            x = frame(form, H, W, seed=H + W, kind=kind)
            data = R.encode(x, form, S, {"k": "v"})
            im = Image.open(io.BytesIO(data))
            im.load()
            assert np.array_equal(np.asarray(im), R.pixels(x, form)) and im.text == {"k": "v"}
            chunks = R.split_chunks(data[8:])
            assert [t for t, _, _ in chunks] == [b"IHDR", b"tEXt"] + [b"IDAT"] * -(-H // S) + [b"IEND"]
            for kind_, d, crc in chunks:
                assert crc == zlib.crc32(kind_ + d)
            z = b"".join(d for t, d, _ in chunks if t == b"IDAT")
            filtered = R.filter_rows(R.quantise(x, form), R.BPP[form]).tobytes()
            assert zlib.decompress(z) == filtered
            assert int.from_bytes(z[-4:], "big") == zlib.adler32(filtered) == R.adler32(filtered)
            assert z[:2] == b"\x78\x01"


def test_depth_quantisation_is_save_normalized_depth():
    import torch
    d = torch.rand(1, 9, 13, generator=torch.Generator().manual_seed(1)) * 1.5 - 0.25
    want = (0xffff * torch.clamp(d, 0, 1)).to(torch.int32).squeeze(0).numpy().astype("uint16")     # iw3/base_depth_model.py:203-204
    assert np.array_equal(R.pixels(d.numpy(), R.GRAY16_F32), want)
    rgb = torch.rand(3, 9, 13, generator=torch.Generator().manual_seed(2)) * 1.5 - 0.25
    want = (torch.clamp(rgb, 0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
    assert np.array_equal(R.pixels(rgb.numpy(), R.RGB8_F32), want)


def test_header_is_what_pil_writes():
    text = {"iw3_min_depth_value": 0.5, "iw3_max_depth_value": 20.0}
    for form, pix in [(R.RGB8_U8, np.zeros((5, 9, 3), np.uint8)), (R.GRAY16_F32, np.zeros((5, 9), np.uint16))]:
        for t in (None, text):
            want = pil_bytes(pix, 6, t)
            want = want[:want.index(b"IDAT") - 4]
            assert R.header(5, 9, form, t) == want
            assert P.header(5, 9, form, t) == want                                                # png_host.h through the C ABI
    assert P.header(8192, 1, R.RGB8_F32) == R.header(8192, 1, R.RGB8_F32)
    with pytest.raises(Exception):
        P.header(8193, 1, 0)
    with pytest.raises(Exception):
        P.header(4, 4, 0, {"k" * 80: "v"})


def fill_defeating_rows(H, W):
    """Rows of independent noise: no filter predicts them, every byte value occurs, matches are rare."""
    return np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)


def alternating_rows(H, W):
    """A pattern that defeats every filter: neighbouring pixels and neighbouring rows are as far apart as bytes can be."""
    yy, xx = np.mgrid[0:H, 0:W]
    v = (((xx + yy) & 1) * 255) ^ ((xx * 37 + yy * 91) & 127)
    return np.stack([v, 255 - v, v ^ 85], axis=2).astype(np.uint8)


def test_the_bound_holds_on_adversarial_inputs():
    for H, W, S in [(1, 1, 1), (7, 1, 1), (1, 9, 1), (24, 40, 1), (24, 40, 5), (24, 40, 24)]:
        for form in FORMS:
            bound = P.max_bytes(H, W, form, S)
            assert bound == R.max_bytes(H, W, form, S) > 0
            xs = [fill_defeating_rows(H, W), alternating_rows(H, W)]
            if form != R.RGB8_U8:
                c = 1 if form == R.GRAY16_F32 else 3
                xs = [np.ascontiguousarray(x.transpose(2, 0, 1)[:c]).astype(np.float32) / 255 for x in xs]
            for x in xs:
                assert len(R.body(x, form, S)) <= bound
    assert P.max_bytes(0, 4, 0, 1) == -1 and P.max_bytes(4, 8193, 0, 1) == -1 and P.max_bytes(4, 4, 3, 1) == -1
    assert P.workspace_bytes(17, 4, 4, 0, 1) == -1 and P.workspace_bytes(1, 4, 4, 0, 4) > 0
    # a worst case by construction: every literal at 15 bits cannot happen, but the bound must not depend on that
    assert R.max_bytes(8192, 8192, 0, 8192) < 2 ** 31


def test_what_the_crafted_inputs_exercise():
    f = R.fibonacci_frame()
    sc = R.stripe_codes(f, R.RGB8_U8, 8)[0]
    depth = max(R.unlimited_depths(sc.lit_hist).values())
    assert depth > 15 and max(sc.lit_len) == 15                                                   # the limiter really runs
    assert sum(2.0 ** -n for n in sc.lit_len if n) <= 1.0
    data = R.encode(f, R.RGB8_U8, 8)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), f)
    black = np.zeros((4, 9, 3), np.uint8)
    sc = R.stripe_codes(black, R.RGB8_U8, 4)[0]
    assert [s for s in range(256) if sc.lit_hist[s]] == [0] and sum(sc.dist_hist) > 0             # one distinct literal
    assert sc.dist_len[2] == 1 and sum(sc.dist_len) == 1                                          # one distance code of one bit
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(R.encode(black, R.RGB8_U8, 4)))), black)
    want_tail = {259: [(0,)], 260: [(0,), (0,)], 261: [(3, 2)]}
    for x, S, run in R.run_frames():
        filtered = R.filter_rows(R.quantise(x, R.GRAY16_F32), 2)
        toks = R.tokens(filtered[:S].reshape(-1), 2)
        assert toks == [(0,), (0,), (258, 2)] + want_tail[run]
        im = Image.open(io.BytesIO(R.encode(x, R.GRAY16_F32, S)))
        assert np.array_equal(np.asarray(im), R.pixels(x, R.GRAY16_F32))
    # a stripe without any match sends no distance code at all, and zlib accepts that
    x = np.array([[[10, 20, 30]]], np.uint8)
    sc = R.stripe_codes(x, R.RGB8_U8, 1)[0]
    assert sum(sc.dist_hist) == 0 and sc.hdist == 1
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(R.encode(x, R.RGB8_U8, 1)))), x)


def test_code_lengths_are_a_prefix_code_within_the_limit():
    rng = np.random.default_rng(11)
    for n, limit in [(286, 15), (30, 15), (19, 7)]:
        for _ in range(20):
            hist = (rng.integers(0, 2, n) * rng.integers(1, 10 ** rng.integers(1, 7), n)).tolist()
            lens = R.code_lengths(hist, limit)
            used = [k for k in range(n) if hist[k]]
            assert all(lens[k] == 0 for k in range(n) if not hist[k])
            if len(used) == 1:
                assert lens[used[0]] == 1
            elif used:
                assert all(1 <= lens[k] <= limit for k in used)
                assert sum(2.0 ** -lens[k] for k in used) == 1.0
                codes = R.canonical_codes(lens)
                assert len({(lens[k], codes[k]) for k in used}) == len(used)


# ---- size against libpng ------------------------------------------------------------------------------------------------------------
# restatement bytes / PIL bytes at compress_level 6 and 1, 256 x 256 RGB, the default stripe_rows; recorded from this test's own print
RECORDED = {"smooth_noise": (0.9742, 0.9595), "smooth": (1.1496, 0.8604), "poster_bars": (1.0564, 0.6716)}


def natural_frames():
    import torch
    base = synth_image(21, 3, 256, 256)
    low = torch.rand(1, 3, 5, 5, generator=torch.Generator().manual_seed(4))
    smooth = torch.nn.functional.interpolate(low, size=(256, 256), mode="bicubic", align_corners=False)[0].clamp(0, 1)
    poster = (smooth * 6).floor() / 6
    poster[:, :32] = 0
    poster[:, -32:] = 0
    return {"smooth_noise": base.numpy(), "smooth": smooth.numpy(), "poster_bars": poster.numpy()}


def test_size_against_libpng():
    lines = []
    for name, x in natural_frames().items():
        mine = len(R.encode(x, R.RGB8_F32, P.DEFAULT_STRIPE_ROWS))
        pix = R.pixels(x, R.RGB8_F32)
        l6, l1 = len(pil_bytes(pix, 6)), len(pil_bytes(pix, 1))
        r6, r1 = mine / l6, mine / l1
        lines.append(f"{name}: restatement {mine} bytes, libpng level 6 {l6} (ratio {r6:.4f}), level 1 {l1} (ratio {r1:.4f})")
        print(lines[-1])
        w6, w1 = RECORDED[name]
        assert w6 * 0.95 <= r6 <= w6 * 1.05 and w1 * 0.95 <= r1 <= w1 * 1.05, lines[-1]
    if os.environ.get("PNG_SIZE_REPORT"):
        with open(os.environ["PNG_SIZE_REPORT"], "w") as f:
            f.write("\n".join(lines) + "\n")


def test_derived_sizes():
    const = np.full((3, 256, 256), 0.3, np.float32)
    data = R.encode(const, R.RGB8_F32, P.DEFAULT_STRIPE_ROWS)
    assert len(data) < 0.01 * 256 * 256 * 3, len(data)
    noise = np.random.default_rng(0).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    for S in (1, 4, 16, 64):
        assert len(R.body(noise, R.RGB8_U8, S)) <= R.max_bytes(64, 64, R.RGB8_U8, S)
