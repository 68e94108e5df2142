"""The fused HDR planar entry (``nunif_amd/csrc/hdr_planes.hip``) restated from its two pinned halves, for
tests/test_hdr_planes_cpu.py and tests/test_gpu_hdr_planes.py.  Three steps, nothing of the kernel in them:

1. ``pixfmt_ref.yuv_to_rgb(planes, "yuv420p10le", "bt2020", full_range, dtype, clamp=True)``;
2. ``torch.round(v * 65535)`` taken in fp32: the rgb48 codes (the intermediate the reference's route has too);
3. ``hdr_ref.hdr2sdr_ref(codes, trc, colorspace, dtype, **params)``.

The codes are always the fp32 ones — they are integers, the kernel's contract is to hit them exactly — so ``dtype`` chooses the
precision of step 3 only: float64 is the truth of the map on those codes, fp32 the yardstick.  Also the case table."""
import numpy as np
import torch

import hdr_ref as H
import pixfmt_ref as P

FMT, MATRIX = "yuv420p10le", "bt2020"
PQ, HLG = H.PQ, H.HLG
SHAPES = list(P.SHAPES) + list(P.LIMIT_SHAPES)                 # (H, W); the last two are the size limits
PITCH_MODES = ["pad64", "odd", "packed"]                       # pixfmt_ref.padded_pitches
KINDS = ["noise", "wild", "constant", "ramp"]
AXES = [(trc, cs, full) for trc in (PQ, HLG) for cs in ("bt709", "bt601") for full in (False, True)]
# every shape with every axis; the pitch mode rotates so that each shape and each axis meets all three
CASES = [(shape, axis, PITCH_MODES[(i + j) % 3]) for i, shape in enumerate(SHAPES) for j, axis in enumerate(AXES)]
IDS = [f"{h}x{w}-{'pq' if trc == PQ else 'hlg'}-{cs}-{'full' if full else 'limited'}-{mode}"
       for (h, w), (trc, cs, full), mode in CASES]
FORMS = ["u16", "chw", "debug"]


def make_planes(kind, h, w):
    """Three uint16 planes of a yuv420p10le frame.  ``noise`` / ``wild`` / ``constant`` are pixfmt_ref's.  ``ramp``: luma walks all
    1024 codes (flat index mod 1024); chroma is neutral (512) over the upper half of the chroma rows, so that r = g = b sweeps the
    whole PQ / HLG curve, and one code above neutral over the lower half: only 877 luma codes lie inside the limited range, and
    the offset puts a second set of rgb codes between the first's."""
    if kind != "ramp":
        return P.make_planes(kind, FMT, h, w)
    ch, cw = P.chroma_size(h, w)
    y = (np.arange(h * w, dtype=np.int64) % 1024).reshape(h, w).astype(np.uint16)
    c = np.full((ch, cw), 512, dtype=np.uint16)
    c[(ch + 1) // 2:] = 513
    return [y, c, c.copy()]


def rgb48_codes(planes, full_range):
    """Steps 1 and 2: uint16 [H, W, 3]."""
    v = P.yuv_to_rgb(planes, FMT, MATRIX, full_range, torch.float32, clamp=True)
    return np.ascontiguousarray(torch.round(v * 65535).to(torch.int32).permute(1, 2, 0).numpy().astype(np.uint16))


def hdr_planes_ref(planes, full_range, trc, colorspace, dtype=torch.float32, **params):
    """(the value before ``* 65535`` as [H, W, 3] of ``dtype``, the uint16 frame [H, W, 3], the rgb48 codes that were mapped)."""
    codes = rgb48_codes(planes, full_range)
    v, u16 = H.hdr2sdr_ref(codes, trc, colorspace, dtype, **params)
    return v, u16, codes
