"""The plane forms of the PNG frame encoder (RGBA 8, grey 8, grey + alpha 8) without a GPU: tests/png_ref_planes.py, the
restatement the device has to equal byte for byte, writes files that PIL decodes to mode RGBA / L / LA with exactly the quantised
pixels, its zlib body inflates to the filtered bytes, its grey rule is PIL's ``convert("L")``, its header with ``gAMA`` is what PIL
writes; the header, the bound and the workspace of nunif_amd/csrc/png_host.h (through the C ABI) equal the restatement's for the
new forms, form 3 stays refused, and the bound holds on adversarial inputs."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image
from PIL.PngImagePlugin import PngInfo

import png_ref as R
import png_ref_planes as RP
from nunif_amd.nunif.utils import png as P


def planes(form, channels, H, W, seed=0, wide=False):
    rng = np.random.default_rng(seed)
    scale, shift = (1.4, 0.2) if wide else (1.0, 0.0)
    colour = (rng.random((channels, H, W), dtype=np.float32) * scale - shift).astype(np.float32)
    alpha = (rng.random((1, H, W), dtype=np.float32) * scale - shift).astype(np.float32) if RP.HAS_ALPHA[form] else None
    return colour, alpha


@pytest.mark.parametrize("form", RP.FORMS)
def test_files_decode_to_the_quantised_pixels_and_the_body_is_zlib(form):
    for (H, W), S in [((1, 1), 1), ((1, 7), 1), ((3, 5), 2), ((17, 33), 3), ((17, 33), 17), ((64, 96), 16)]:
        for channels in ((3,) if form == RP.RGBA8_F32 else (1, 3)):
            for wide in (False, True):
                colour, alpha = planes(form, channels, H, W, seed=H + W, wide=wide)
                data = RP.encode(colour, alpha, form, S, {"k": "v"}, gamma=50000)
                im = Image.open(io.BytesIO(data))
                im.load()
                assert im.mode == RP.PIL_MODE[form] and im.text == {"k": "v"} and im.info["gamma"] == 0.5
                assert np.array_equal(np.asarray(im), RP.pixels(colour, alpha, form))
                chunks = R.split_chunks(data[8:])
                assert [t for t, _, _ in chunks] == [b"IHDR", b"gAMA", b"tEXt"] + [b"IDAT"] * -(-H // S) + [b"IEND"]
                for kind, d, crc in chunks:
                    assert crc == zlib.crc32(kind + d)
                z = b"".join(d for t, d, _ in chunks if t == b"IDAT")
                filtered = RP.filtered(colour, alpha, form).tobytes()
                assert zlib.decompress(z) == filtered and int.from_bytes(z[-4:], "big") == zlib.adler32(filtered)


def test_quantisation_is_quantize256():
    import torch
    x = torch.rand(3, 9, 13, generator=torch.Generator().manual_seed(1)) * 1.5 - 0.25
    want = torch.clamp((x * 255).round(), 0, 255).to(torch.uint8).numpy()          # nunif/transforms/functional.py:9-12
    assert np.array_equal(RP.quantize256(x.numpy()), want)
    half = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255], np.float32)                  # ties go to the even byte
    assert RP.quantize256(half).tolist() == np.rint(half * np.float32(255)).astype(np.uint8).tolist()


def test_the_grey_rule_is_pils_convert_l():
    g = np.arange(256, dtype=np.uint8)
    corners = np.array([[r, gg, b] for r in (0, 255) for gg in (0, 255) for b in (0, 255)], np.uint8)
    rnd = np.random.default_rng(5).integers(0, 256, (100000, 3), dtype=np.uint8)
    triples = np.concatenate([np.stack([g, g, g], axis=1), corners, rnd])
    n = len(triples)
    pil = np.asarray(Image.fromarray(triples.reshape(1, n, 3), "RGB").convert("L")).reshape(-1)
    mine = RP.pil_l(triples[:, 0], triples[:, 1], triples[:, 2])
    assert np.array_equal(mine, pil)
    assert np.array_equal(mine[:256], g)                                            # a grey triple keeps its value
    rgba = np.concatenate([triples, rnd[:n, :1] if n <= len(rnd) else np.resize(rnd[:, 0], (n, 1))], axis=1)
    la = np.asarray(Image.fromarray(rgba.reshape(1, n, 4), "RGBA").convert("LA")).reshape(n, 2)
    assert np.array_equal(la[:, 0], mine) and np.array_equal(la[:, 1], rgba[:, 3])  # alpha passes through


def test_header_with_gamma_is_what_pil_writes():
    pix = {RP.RGBA8_F32: np.zeros((5, 9, 4), np.uint8), RP.GRAY8_F32: np.zeros((5, 9), np.uint8),
           RP.GRAYA8_F32: np.zeros((5, 9, 2), np.uint8), R.RGB8_U8: np.zeros((5, 9, 3), np.uint8)}
    for form, a in pix.items():
        for text in (None, {"k": "v"}):
            info = PngInfo()
            info.add(b"gAMA", (45455).to_bytes(4, "big"))
            for k, v in (text or {}).items():
                info.add_text(k, v)
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, format="png", pnginfo=info)
            want = buf.getvalue()
            want = want[:want.index(b"IDAT") - 4]
            assert RP.header(5, 9, form, text, 45455) == want
            assert P.header(5, 9, form, text, 45455) == want                        # png_host.h and the host-built gAMA
            assert Image.open(io.BytesIO(buf.getvalue())).info["gamma"] == 0.45455
            assert P.header(5, 9, form, text) == RP.header(5, 9, form, text)
    with pytest.raises(ValueError):
        P.header(5, 9, RP.RGBA8_F32, None, -1)


def test_the_host_arithmetic_equals_the_restatement():
    for form in RP.FORMS:
        for H, W in [(1, 1), (2, 17), (17, 2), (64, 96), (1, 8192), (8192, 1), (8192, 8192)]:
            for S in sorted({1, min(16, H), H}):
                assert P.max_bytes(H, W, form, S) == RP.max_bytes(H, W, form, S) > 0
                for B in (1, 3, 16):
                    assert P.workspace_bytes(B, H, W, form, S) == RP.workspace_bytes(B, H, W, form, S) > 0
        assert P.max_bytes(8193, 4, form, 1) == -1 and P.max_bytes(4, 8193, form, 1) == -1 and P.max_bytes(0, 4, form, 1) == -1
        assert P.workspace_bytes(17, 4, 4, form, 1) == -1
    assert RP.max_bytes(8192, 8192, RP.RGBA8_F32, 8192) < 2 ** 31                   # the offsets are 32 bits: the longest body fits
    assert 8192 * (1 + 4 * 8192) < 2 ** 31                                          # and so does a stripe's byte count
    # 3 names no form
    assert P.max_bytes(4, 4, 3, 1) == -1 and P.workspace_bytes(1, 4, 4, 3, 1) == -1
    with pytest.raises(Exception):
        P.header(4, 4, 3)
    for form in (0, 1, 2):                                                          # the old forms: unchanged
        assert P.max_bytes(17, 33, form, 3) == R.max_bytes(17, 33, form, 3)
        assert P.workspace_bytes(2, 17, 33, form, 3) == RP.workspace_bytes(2, 17, 33, form, 3)


def test_the_bound_holds_on_adversarial_inputs():
    yy, xx = np.mgrid[0:24, 0:40]
    v = ((((xx + yy) & 1) * 255) ^ ((xx * 37 + yy * 91) & 127)).astype(np.float32) / 255
    noise = np.random.default_rng(3).integers(0, 256, (4, 24, 40)).astype(np.float32) / 255
    alternating = np.stack([v, 1 - v, np.roll(v, 1, axis=1), np.roll(1 - v, 1, axis=0)])
    for src in (noise, alternating):
        for H, W, S in [(1, 1, 1), (7, 1, 1), (1, 9, 1), (24, 40, 1), (24, 40, 5), (24, 40, 24)]:
            for form in RP.FORMS:
                channels = 3 if form == RP.RGBA8_F32 else 1
                colour = np.ascontiguousarray(src[:channels, :H, :W])
                alpha = np.ascontiguousarray(src[3:4, :H, :W]) if RP.HAS_ALPHA[form] else None
                assert len(RP.body(colour, alpha, form, S)) <= P.max_bytes(H, W, form, S)
