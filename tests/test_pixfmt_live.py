"""The engine's pixel-format arithmetic next to libswscale's, where PyAV is installed (skipped everywhere else).

Both directions of the fp32 restatement (tests/pixfmt_ref.py, which the kernels are pinned to in tests/test_gpu_pixfmt.py) are
compared with ``VideoFrame.reformat`` on the case inputs.  The two are NOT the same arithmetic: the engine uses the ITU definitions
in floating point and linear chroma resampling, swscale fixed-point tables and its own scaler ("Pixel formats").  The
test prints the PSNR and the largest code difference of every case and asserts only PSNR >= 40 dB: a detector for a wrong matrix or
a wrong range, not a parity claim.  The figures are unmeasured until this file runs somewhere that has PyAV."""
import numpy as np
import pytest
import torch

import pixfmt_ref as R

av = pytest.importorskip("av")
if str(getattr(av, "__version__", "")).endswith("+stub"):           # oracle/refstub.py's inert placeholder, not PyAV
    pytest.skip("PyAV is not installed", allow_module_level=True)

SPACE = {"bt601": 5, "bt709": 1, "bt2020": 9}        # AVCOL_SPC_BT470BG, _BT709, _BT2020_NCL
MPEG, JPEG = 1, 2                                    # AVCOL_RANGE_*
H, W = 64, 96
MIN_PSNR = 40.0


def psnr(a, b, peak):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    mse = np.mean((a - b) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse), int(np.abs(a - b).max())


def yuv_frame(planes, fmt):
    from nunif_amd.nunif.utils import pixfmt
    layout = pixfmt.PlaneLayout(fmt, W, H)
    return pixfmt.to_av_frame(layout.pack(planes), layout)


def frame_planes(frame, fmt):
    from nunif_amd.nunif.utils import pixfmt
    layout = pixfmt.PlaneLayout(fmt, W, H)
    buf = np.zeros(layout.nbytes, dtype=np.uint8)
    pixfmt.copy_av_planes(frame, layout, layout.views(buf))
    return [v.astype(np.int64) for v in layout.views(buf)]


@pytest.mark.parametrize("kind", R.INPUTS)
@pytest.mark.parametrize("fmt,matrix,full", R.COMBOS)
def test_going_in_against_reformat(fmt, matrix, full, kind):
    bits = R.FORMATS[fmt][0]
    planes = R.make_planes(kind, fmt, H, W)
    peak = 65535 if bits > 8 else 255
    rgb = yuv_frame(planes, fmt).reformat(format="rgb48le" if bits > 8 else "rgb24",
                                          src_colorspace=SPACE[matrix], dst_colorspace=SPACE[matrix],
                                          src_color_range=JPEG if full else MPEG, dst_color_range=JPEG)
    theirs = rgb.to_ndarray().astype(np.int64)                                                   # HWC
    ours = R.yuv_to_rgb(planes, fmt, matrix, full, dtype=torch.float32, clamp=True)
    ours = torch.floor(ours * peak + 0.5).permute(1, 2, 0).to(torch.int64).numpy()
    db, worst = psnr(ours, theirs, peak)
    print(f"in  {fmt} {matrix} {'full' if full else 'limited'} {kind}: PSNR {db:.2f} dB, max |diff| {worst} of {peak}")
    assert db >= MIN_PSNR


@pytest.mark.parametrize("kind", R.INPUTS)
@pytest.mark.parametrize("fmt,matrix,full", R.COMBOS)
def test_going_out_against_reformat(fmt, matrix, full, kind):
    bits = R.FORMATS[fmt][0]
    peak = 65535 if bits > 8 else 255
    codes = torch.floor(R.make_tensor(kind, fmt, H, W).clamp(0, 1) * peak + 0.5).permute(1, 2, 0).numpy()
    codes = np.ascontiguousarray(codes.astype(np.uint16 if bits > 8 else np.uint8))
    rgb = av.VideoFrame.from_ndarray(codes, format="rgb48le" if bits > 8 else "rgb24")
    out = rgb.reformat(format=fmt, src_colorspace=SPACE[matrix], dst_colorspace=SPACE[matrix],
                       src_color_range=JPEG, dst_color_range=JPEG if full else MPEG)
    theirs = frame_planes(out, fmt)
    x = torch.from_numpy(codes.astype(np.float32) / np.float32(peak)).permute(2, 0, 1)       # the frame both sides see
    ours = R.rgb_to_yuv(x, fmt, matrix, full, dtype=torch.float32)
    top = (1 << bits) - 1
    for name, a, b in zip("YUV", ours, theirs):
        db, worst = psnr(a, b, top)
        print(f"out {fmt} {matrix} {'full' if full else 'limited'} {kind} {name}: PSNR {db:.2f} dB, max |diff| {worst} of {top}")
        assert db >= MIN_PSNR
