"""Planar YUV <-> rgb, the parts that need no GPU: the host-side constants of the C ABI are the restatement's (tests/pixfmt_ref.py)
bit for bit, the restatement agrees with an independent implementation (PIL's JFIF YCbCr) where one exists, the resampling kernels
have the properties their definition promises, the Python layer's signatures, layout arithmetic and refusals, and the inputs of
tests/test_gpu_pixfmt.py keep the restatement itself inside the tie-band budget."""
import inspect
import itertools

import numpy as np
import pytest
import torch

import pixfmt_ref as R
from nunif_amd.nunif.utils import pixfmt


# ---- constants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full,bits,direction", list(itertools.product(R.KR_KB, (False, True), (8, 10), (0, 1))))
def test_constants_are_the_restatements_bit_for_bit(matrix, full, bits, direction):
    m, off = pixfmt.constants(matrix, full, bits, direction)
    want_m, want_off = R.coefficients(matrix, full, bits, direction)
    want_m = np.asarray(want_m, dtype=np.float64).astype(np.float32).reshape(-1)
    assert np.asarray(m, dtype=np.float32).tobytes() == want_m.tobytes()
    assert np.asarray(off, dtype=np.float32).tobytes() == np.asarray(want_off, dtype=np.float32).tobytes()


@pytest.mark.parametrize("matrix,full,bits", list(itertools.product(R.KR_KB, (False, True), (8, 10))))
def test_forward_and_inverse_matrices_multiply_to_the_identity(matrix, full, bits):
    a = np.asarray(R.coefficients(matrix, full, bits, 0)[0])
    b = np.asarray(R.coefficients(matrix, full, bits, 1)[0])
    assert np.abs(a @ b - np.eye(3)).max() <= 1e-12 and np.abs(b @ a - np.eye(3)).max() <= 1e-12
    assert R.coefficients(matrix, full, bits, 0)[1] == R.coefficients(matrix, full, bits, 1)[1]


def test_code_ranges():
    for bits in (8, 10):
        s = 1 << (bits - 8)
        white, black = torch.ones(3, 2, 2), torch.zeros(3, 2, 2)
        for matrix in R.KR_KB:
            fmt = "yuv444p" if bits == 8 else "yuv420p10le"
            assert [int(p[0, 0]) for p in R.rgb_to_yuv(white, fmt, matrix, False, torch.float64)] == [235 * s, 128 * s, 128 * s]
            assert [int(p[0, 0]) for p in R.rgb_to_yuv(black, fmt, matrix, False, torch.float64)] == [16 * s, 128 * s, 128 * s]
            assert [int(p[0, 0]) for p in R.rgb_to_yuv(white, fmt, matrix, True, torch.float64)] == [256 * s - 1, 128 * s, 128 * s]
            red = torch.tensor([1.0, 0.0, 0.0]).view(3, 1, 1).expand(3, 2, 2)
            blue = torch.tensor([0.0, 0.0, 1.0]).view(3, 1, 1).expand(3, 2, 2)
            assert int(R.rgb_to_yuv(red, fmt, matrix, False, torch.float64)[2][0, 0]) == 240 * s          # Cr at its top
            assert int(R.rgb_to_yuv(blue, fmt, matrix, False, torch.float64)[1][0, 0]) == 240 * s         # Cb at its top


# ---- the independent pin: PIL's JFIF YCbCr is bt601, full range, 8 bit, 4:4:4 ------------------------------------------------
def _pil_images():
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2).repeat(4, axis=0)
    return {"noise": noise, "grey ramp": ramp}


@pytest.mark.parametrize("name", ["noise", "grey ramp"])
def test_restatement_is_within_one_code_of_pil(name):
    Image = pytest.importorskip("PIL.Image")
    rgb = _pil_images()[name]
    ycc = np.asarray(Image.fromarray(rgb, "RGB").convert("YCbCr")).astype(np.int64)
    x = torch.from_numpy(rgb.astype(np.float64) / 255.0).permute(2, 0, 1)
    ours = np.stack(R.rgb_to_yuv(x, "yuv444p", "bt601", True, torch.float64), axis=2)
    d_out = np.abs(ours - ycc).max()
    back = np.asarray(Image.fromarray(ycc.astype(np.uint8), "YCbCr").convert("RGB")).astype(np.int64)
    planes = [ycc[:, :, i] for i in range(3)]
    v = R.yuv_to_rgb(planes, "yuv444p", "bt601", True, torch.float64, clamp=True)
    ours_back = torch.floor(v * 255.0 + 0.5).permute(1, 2, 0).numpy().astype(np.int64)
    d_in = np.abs(ours_back - back).max()
    print(f"{name}: rgb -> YCbCr differs from PIL by at most {d_out} code, YCbCr -> rgb by at most {d_in}")
    assert d_out <= 1 and d_in <= 1


# ---- the resampling kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.SHAPES)
def test_a_constant_chroma_plane_upsamples_to_a_constant(h, w):
    ch, cw = R.chroma_size(h, w)
    for dtype in (torch.float64, torch.float32):
        up = R.upsample(torch.full((ch, cw), 171.0, dtype=dtype), h, w)
        assert up.shape == (h, w) and bool((up == 171.0).all())


def test_upsampled_codes_are_exact_in_fp32():
    c = torch.from_numpy(np.random.default_rng(3).integers(0, 65536, (9, 17)).astype(np.float64))
    assert torch.equal(R.upsample(c.float(), 18, 33).double(), R.upsample(c, 18, 33))


def test_downsample_of_upsample_is_not_the_identity():
    """Down(up(c)) smooths: measured on seeded 8-bit noise (33 x 47 chroma samples) the largest deviation is 80.9 codes, the mean
    26.0; on a plane that is linear in x and y it is exact away from the clamped border (0.625 code on it).  Nothing requires the identity: the two
    kernels are each the linear filter of their own direction, not each other's inverse."""
    rng = np.random.default_rng(11)
    c = torch.from_numpy(rng.integers(16, 241, (33, 47)).astype(np.float64))
    d = (R.downsample(R.upsample(c, 66, 94)) - c).abs()
    print(f"down(up(noise)): largest deviation {float(d.max()):.3f} codes, mean {float(d.mean()):.3f}")
    assert d.max() > 1.0
    yy, xx = torch.meshgrid(torch.arange(33.0, dtype=torch.float64), torch.arange(47.0, dtype=torch.float64), indexing="ij")
    lin = 20.0 + 2.0 * xx + 3.0 * yy
    dl = (R.downsample(R.upsample(lin, 66, 94)) - lin).abs()
    print(f"down(up(linear)): interior {float(dl[1:-1, 1:-1].max()):.3g}, border {float(dl.max()):.3g}")
    assert dl[1:-1, 1:-1].max() <= 1e-9


@pytest.mark.parametrize("matrix,full", list(itertools.product(R.KR_KB, (False, True))))
def test_float64_round_trip_at_444(matrix, full):
    x = torch.from_numpy(np.random.default_rng(5).random((3, 17, 23)))
    vals = R.rgb_to_yuv_values(x, "yuv444p", matrix, full, torch.float64)
    m, off = R._coef_t(matrix, full, 8, 0, torch.float64)
    a, b, d = vals[0] - off[0], vals[1] - off[1], vals[2] - off[2]
    back = torch.stack([(m[e, 0] * a + m[e, 1] * b) + m[e, 2] * d for e in range(3)])
    assert (back - x).abs().max() <= 1e-12


# ---- the inputs of the GPU test keep the restatement inside the tie-band budget -------------------------------------------
def test_tie_band_share_of_the_case_inputs():
    """The fp32 restatement against float64's rounding on every case tests/test_gpu_pixfmt.py runs on the way out.  Measured: the
    band (4 x the fp32 deviation) is at most 4.6e-4 code (10 bit: a deviation of 1.1e-4 code, about two ulp of 1023), the largest
    share of samples inside it is 0.22 % (18 x 33 yuv420p10le bt601 limited, noise: 2 of 900), and the fp32 restatement itself
    never differs from float64 outside the band or by more than 1."""
    worst_share, worst_band, worst = 0.0, 0.0, None
    for (h, w), (fmt, matrix, full), kind in itertools.product(R.SHAPES, R.COMBOS, R.INPUTS):
        x = R.make_tensor(kind, fmt, h, w)
        a = R.exit_agreement(R.rgb_to_yuv(x, fmt, matrix, full, torch.float32), x, fmt, matrix, full)
        assert a["bad"] == 0, (h, w, fmt, matrix, full, kind, a)
        assert a["share"] <= R.BAND_SHARE, (h, w, fmt, matrix, full, kind, a)
        if a["share"] > worst_share:
            worst_share, worst = a["share"], (h, w, fmt, matrix, full, kind, a["in_band"], a["samples"])
        worst_band = max(worst_band, a["band"])
    print(f"largest band {worst_band:.3e} code, largest share in band {100 * worst_share:.3f} % at {worst}")
    assert worst_band < 0.01


# ---- the Python layer -----------------------------------------------------------------------------------------------------
def test_signatures():
    def names(f):
        return list(inspect.signature(f).parameters)
    assert names(pixfmt.PlaneLayout.__init__)[1:] == ["format", "width", "height", "pitches"]
    assert names(pixfmt.yuv_to_tensor)[:7] == ["planes", "layout", "matrix", "full_range", "device", "out", "frame_out"]
    assert names(pixfmt.tensor_to_yuv) == ["x", "layout", "matrix", "full_range", "out"]
    assert names(pixfmt.yuv_entry) == names(pixfmt.yuv_leave) == ["layout", "matrix", "full_range"]
    assert names(pixfmt.from_av_frame)[0] == "frame" and names(pixfmt.to_av_frame) == ["planes", "layout", "template", "format"]
    lay = pixfmt.PlaneLayout("yuv420p", 8, 8)
    assert names(pixfmt.yuv_entry(lay, "bt709", False)) == ["buf", "device"]
    assert names(pixfmt.yuv_leave(lay, "bt709", False)) == ["y", "bits", "out"]
    from nunif_amd.frame_ring import FrameRing
    from nunif_amd.iw3.frame_pipeline import PipelineOps
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    six = ["in_format", "in_matrix", "in_full_range", "out_format", "out_matrix", "out_full_range"]
    assert names(Waifu2xVideoStream.__init__)[-6:] == six and names(PipelineOps.__init__)[-6:] == six
    ring = inspect.signature(FrameRing.__init__).parameters
    assert ring["in_bytes"].default is None and ring["out_bytes"].default is None
    assert names(FrameRing.__init__)[:13] == ["self", "process_fn", "in_shape", "out_shape", "device", "depth", "bits", "zero_copy",
                                              "out_mode", "edge_streams", "enter_fn", "leave_fn", "in_bits"]


def test_plane_layout_arithmetic():
    lay = pixfmt.PlaneLayout("yuv420p", 33, 5)
    assert (lay.chroma_width, lay.chroma_height, lay.bits, lay.sample_bytes) == (17, 3, 8, 1)
    assert lay.pitches == (64, 64, 64) and lay.offsets == (0, 320, 512) and lay.nbytes == 704
    lay = pixfmt.PlaneLayout("yuv420p10le", 7, 1, pitches=[14, 10, 12])
    assert (lay.chroma_width, lay.chroma_height, lay.bits, lay.sample_bytes) == (4, 1, 10, 2)
    assert lay.offsets == (0, 64, 128) and lay.nbytes == 192
    lay = pixfmt.PlaneLayout("yuvj444p", 5, 3, pitches=[5, 7, 9])
    assert lay.format == "yuv444p" and (lay.chroma_width, lay.chroma_height) == (5, 3) and lay.offsets == (0, 64, 128)
    planes = R.make_planes("noise", "yuv420p", 5, 33)
    lay = pixfmt.PlaneLayout("yuv420p", 33, 5, pitches=R.padded_pitches("yuv420p", 33, "odd"))
    buf = lay.pack(planes, fill=0xA5)
    for got, want in zip(lay.views(buf), planes):
        assert np.array_equal(got, want)
    assert int((buf == 0xA5).sum()) >= lay.nbytes - sum(p.size for p in planes) - 3       # the padding kept its fill
    assert pixfmt.PlaneLayout("yuv420p", 33, 5) == pixfmt.PlaneLayout("yuv420p", 33, 5, pitches=[64, 64, 64])


def test_refusals_on_the_host():
    import ctypes
    from nunif_amd import _hip
    m, off = (ctypes.c_float * 9)(), (ctypes.c_float * 3)()
    lib = _hip.lib()
    assert lib.nunif_hip_pixfmt_constants(709, 0, 8, 0, m, off) == 0
    for bad in ((470, 0, 8, 0), (709, 2, 8, 0), (709, 0, 12, 0), (709, 0, 8, 2)):
        assert lib.nunif_hip_pixfmt_constants(*bad, m, off) == -1
    assert lib.nunif_hip_pixfmt_constants(709, 0, 8, 0, None, off) == -1
    for fmt in ("yuv422p", "nv12", "p010le", "yuv420p12le", "gbrp", "rgb24"):
        with pytest.raises(ValueError, match="format"):
            pixfmt.PlaneLayout(fmt, 8, 8)
    with pytest.raises(ValueError, match="8192"):
        pixfmt.PlaneLayout("yuv420p", 8193, 8)
    with pytest.raises(ValueError, match="8192"):
        pixfmt.PlaneLayout("yuv420p", 8, 0)
    with pytest.raises(ValueError, match="pitch"):
        pixfmt.PlaneLayout("yuv420p", 8, 8, pitches=[7, 4, 4])
    with pytest.raises(ValueError, match="pitch"):
        pixfmt.PlaneLayout("yuv420p10le", 8, 8, pitches=[17, 8, 8])
    lay = pixfmt.PlaneLayout("yuv420p", 8, 8)
    buf = torch.zeros(lay.nbytes, dtype=torch.uint8)
    with pytest.raises(ValueError, match="matrix"):
        pixfmt.yuv_to_tensor(buf, lay, "bt470", False)
    with pytest.raises(ValueError, match="matrix"):
        pixfmt.constants("smpte240m", False, 8, 0)
    with pytest.raises(ValueError):
        pixfmt.constants("bt709", False, 12, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pixfmt.yuv_to_tensor(buf, lay, "bt709", False)                               # neither on the device nor pinned
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pixfmt.tensor_to_yuv(torch.zeros(3, 8, 8), lay, "bt709", False)
    with pytest.raises(ValueError, match="nbytes"):
        pixfmt.yuv_to_tensor(buf[:-1], lay, "bt709", False)
    with pytest.raises(ValueError, match="matrix"):
        pixfmt.yuv_entry(lay, "bt470", False)
    from nunif_amd.waifu2x.video import Waifu2xVideoStream
    import types
    ctx = types.SimpleNamespace(device="cuda:0")
    with pytest.raises(ValueError, match="rotate"):
        Waifu2xVideoStream(ctx, types.SimpleNamespace(rotate_left=True, pix_fmt="yuv420p"), in_format="yuv420p")
    with pytest.raises(ValueError, match="hdr"):
        Waifu2xVideoStream(ctx, types.SimpleNamespace(pix_fmt="yuv420p"), in_format="yuv420p", hdr=lambda *a, **k: None)
    with pytest.raises(ValueError, match="in_format"):
        Waifu2xVideoStream(ctx, types.SimpleNamespace(pix_fmt="yuv420p"), in_format="nv12")
    with pytest.raises(ValueError, match="out_matrix"):
        Waifu2xVideoStream(ctx, types.SimpleNamespace(pix_fmt="yuv420p"), out_format="yuv420p", out_matrix="bt470")
