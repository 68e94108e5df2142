"""The host side of the JPEG encoder and the CPU restatement tests/jpeg_ref.py, without a GPU: the library's quantisation tables
against libjpeg's (through PIL), its header against the restatement's byte for byte, the restatement's streams against PIL's decoder
and libjpeg's own encoding (the two gaps the GPU test uses as yardsticks), the stream bound on adversarial inputs, and the
conditions that keep tests/test_gpu_jpeg.py honest: what its crafted inputs exercise, and how rare rounding ties are on the
inputs whose coefficients it compares."""
import numpy as np
import pytest

import jpeg_ref as J

SHAPES = [(8, 8), (16, 16), (17, 23), (40, 56), (33, 130), (64, 96)]
CRAFTED = [("constant", 50), ("noise", 100), ("blocks", 100), ("pixels", 100), ("pixels", 1), ("clamp", 90)]


def test_quant_tables_equal_libjpeg_for_every_quality(hiplib):
    from PIL import Image
    from nunif_amd.nunif.utils.jpeg import quant_tables
    im = Image.new("RGB", (8, 8))
    for quality in range(1, 101):
        luma, chroma = quant_tables(quality)
        ref = J.pil_decode(J.pil_encode(np.asarray(im), quality, 420, 0)).quantization
        # PIL >= 8.3 hands the tables out in natural order; its own streams hold them in zigzag order
        assert list(ref[0]) == luma and list(ref[1]) == chroma, quality
        mine = J.quant_tables(quality)
        assert luma == mine[0].tolist() and chroma == mine[1].tolist()
    from nunif_amd import _hip
    for quality in (0, 101, -3):
        with pytest.raises(_hip.NunifHipError):
            quant_tables(quality)


def _segments(data):
    """marker -> list of payloads, up to SOS."""
    out, i = {}, 2
    while True:
        assert data[i] == 0xFF
        marker, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.setdefault(marker, []).append(data[i + 4:i + 2 + n])
        i += 2 + n
        if marker == 0xDA:
            return out


def test_huffman_tables_are_the_ones_libjpeg_writes():
    """Annex K as typed into jpeg_ref.py (and, through the header test, into jpeg_host.h) against the DHT segments of a stream
    that libjpeg wrote without optimisation."""
    lib = _segments(J.pil_encode(np.zeros((16, 16, 3), np.uint8), 75, 420, 0))
    mine = _segments(J.header(16, 16, 75, 420, 1))

    def tables(segments):
        return {p[i]: p[i + 1:i + 17 + sum(p[i + 1:i + 17])] for p in segments[0xC4] for i in _dht_starts(p)}

    assert tables(lib) == tables(mine) and sorted(tables(mine)) == [0x00, 0x01, 0x10, 0x11]


def _dht_starts(p):
    i = 0
    while i < len(p):
        yield i
        i += 17 + sum(p[i + 1:i + 17])


@pytest.mark.parametrize("ss", [420, 444])
@pytest.mark.parametrize("shape", [(1, 1), (17, 23), (8192, 4321)])
def test_header_equals_the_restatement(hiplib, shape, ss):
    from nunif_amd.nunif.utils.jpeg import header
    for quality, restart in ((1, 1), (75, 16), (100, 65535)):
        got = header(shape[0], shape[1], quality, ss, restart)
        assert len(got) == J.HEADER_BYTES and got == J.header(shape[0], shape[1], quality, ss, restart)


def test_refused_shapes(hiplib):
    from nunif_amd import _hip
    from nunif_amd.nunif.utils import jpeg
    for args in ((0, 8, 420, 1), (8, 8193, 420, 1), (8, 8, 420, 0), (8, 8, 420, 65536)):
        assert jpeg.max_bytes(*args) == -1 and jpeg.workspace_bytes(1, *args) == -1
        with pytest.raises(_hip.NunifHipError):
            jpeg.header(args[0], args[1], 75, args[2], args[3])
    assert hiplib.nunif_hip_jpeg_max_bytes(8, 8, 422, 1) == -1 and hiplib.nunif_hip_jpeg_workspace_bytes(1, 8, 8, 422, 1) == -1
    with pytest.raises(KeyError):
        jpeg.max_bytes(8, 8, "422", 1)
    assert jpeg.workspace_bytes(17, 8, 8, 420, 1) == -1 and jpeg.workspace_bytes(16, 8, 8, 420, 1) > 0


@pytest.mark.parametrize("ss", [420, 444])
def test_restatement_against_pil(ss):
    """PIL opens the restatement's streams; its PSNR to the uint8 input and its size next to libjpeg's own encoding at the same
    quality, subsampling and restart layout are printed: the two gaps are what tests/test_gpu_jpeg.py allows the device."""
    for si, (h, w) in enumerate(SHAPES):
        x = J.synth(20 + si, h, w)
        for quality, restart in ((1, 1), (50, 3), (90, 8), (100, J.whole_row(w, ss))):
            y = J.yardstick(x, quality, ss, restart)
            im = J.pil_decode(y["ref"])
            assert im.size == (w, h) and im.mode == "RGB"
            print(f"{h}x{w} {ss} q{quality} r{restart}: PSNR restatement {y['psnr_ref']:.3f} libjpeg {y['psnr_lib']:.3f} dB, "
                  f"size {y['size_ref']} / {y['size_lib']} = {y['size_ref'] / y['size_lib']:.4f}")


@pytest.mark.parametrize("ss", [420, 444])
def test_max_bytes_covers_adversarial_inputs(hiplib, ss):
    from nunif_amd.nunif.utils.jpeg import max_bytes
    rng = np.random.default_rng(1)
    for h, w in ((8, 8), (17, 23), (40, 56)):
        for restart in (1, 3, J.whole_row(w, ss)):
            assert max_bytes(h, w, ss, restart) == J.max_bytes(h, w, ss, restart)
            for name, quality in CRAFTED:
                assert len(J.encode(J.crafted(name, h, w), quality, ss, restart)) <= max_bytes(h, w, ss, restart)
            # the worst the coder can be given: every coefficient at +-1023 with the longest codes, DC swinging end to end
            my, mx = J.geometry(h, w, ss)
            q = rng.choice([-1023, 1023, -600, 513], size=(my * mx * J.blocks_per_mcu(ss), 64))
            q[:, 0] = np.where(np.arange(q.shape[0]) % 2, -1024, 1023)
            worst = J.stream_from_coefficients(q, h, w, 100, ss, restart)
            assert len(worst) <= max_bytes(h, w, ss, restart)
            assert len(worst) > 0.4 * max_bytes(h, w, ss, restart)          # and the bound is not idle: within 2.5 x of it


def test_crafted_cases_exercise_the_coder():
    seen = {"stuffed": 0, "zrl": 0, "no_eob": 0, "dc": set(), "ac": set()}
    for ss in (420, 444):
        for name, quality in CRAFTED:
            st = {}
            J.encode(J.crafted(name, 40, 56), quality, ss, 3, stats=st)
            seen["stuffed"] += st["stuffed"]
            seen["zrl"] += st["zrl"]
            seen["no_eob"] += st["no_eob"]
            seen["dc"] |= st["dc_categories"]
            seen["ac"] |= st["ac_categories"]
            if name == "noise":
                assert st["stuffed"] > 0
            if name == "blocks":
                assert 11 in st["dc_categories"]
            if name == "pixels":
                assert st["no_eob"] > 0 and (quality != 1 or st["zrl"] > 0) and (quality != 100 or 10 in st["ac_categories"])
            if name == "constant":
                assert st["dc_categories"] == {0} and not st["ac_categories"]
    assert seen["stuffed"] and seen["zrl"] and seen["no_eob"] and {0, 11} <= seen["dc"] and 10 in seen["ac"]


@pytest.mark.parametrize("ss", [420, 444])
def test_ties_are_rare_on_the_compared_inputs(ss):
    """On every input whose coefficients the GPU test compares, at most 1 % of the float64 quotients lie inside the tie band (the
    fp32 restatement's deviation times the margin), and the fp32 restatement itself passes the comparison."""
    inputs = [(J.synth(20 + si, h, w), q) for si, (h, w) in enumerate(SHAPES) for q in (1, 50, 90, 100)]
    inputs += [(J.crafted(name, 40, 56), q) for name, q in CRAFTED]
    inputs += [(J.synth(31, 1, 8192), 50), (J.synth(31, 8192, 1), 90)]
    for x, quality in inputs:
        q32, _ = J.coefficients(x, quality, ss, np.float32)
        a = J.coefficient_agreement(q32, x, quality, ss)
        assert a["band"] <= J.BAND_CEILING
        assert a["in_band"] <= 0.01 * a["coefficients"], a
        assert a["bad"] == 0, a
