"""Planar YUV <-> CHW rgb restated in torch for the tests of ``nunif_amd/csrc/pixfmt.hip``, written from the definitions, not from
the kernel: ITU matrix coefficients, limited / full range code scaling, and linear chroma resampling for the MPEG-2 / H.264 default
chroma position (horizontally on the even luma column, vertically midway between the two rows).  ``dtype=torch.float64`` is the
truth, ``torch.float32`` evaluates the same expressions operation by operation in fp32 (the tests' yardstick).  Also the seeded
case inputs that tests/test_pixfmt_cpu.py and tests/test_gpu_pixfmt.py share."""
import numpy as np
import torch

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
FORMATS = {"yuv420p": (8, True), "yuv444p": (8, False), "yuv420p10le": (10, True)}      # name -> (bits, 4:2:0)
SHAPES = [(2, 2), (1, 1), (5, 7), (16, 8), (18, 33), (64, 96)]                          # (H, W)
LIMIT_SHAPES = [(8, 8192), (8192, 2)]
# (format, matrix, full_range): every matrix and both ranges with every format, not the full cross product
COMBOS = [("yuv420p", "bt709", False), ("yuv420p", "bt601", True), ("yuv420p", "bt2020", False),
          ("yuv444p", "bt601", False), ("yuv444p", "bt709", True), ("yuv444p", "bt2020", True),
          ("yuv420p10le", "bt2020", False), ("yuv420p10le", "bt709", True), ("yuv420p10le", "bt601", False)]
INPUTS = ["noise", "constant", "checker", "wild"]       # wild: codes outside the nominal range / tensor values outside [0, 1]


def coefficients(matrix, full_range, bits, direction):
    """(3 x 3 matrix, 3 offsets) as Python floats (float64).  direction 0: rgb = M (yuv - off); 1: yuv = M rgb + off."""
    Kr, Kb = KR_KB[matrix]
    Kg = 1.0 - Kr - Kb
    step, top = float(1 << (bits - 8)), float((1 << bits) - 1)
    sy, sc = (top, top) if full_range else (219.0 * step, 224.0 * step)
    yoff, coff = (0.0 if full_range else 16.0 * step), 128.0 * step
    if direction == 0:
        m = [[1.0 / sy, 0.0, 2.0 * (1.0 - Kr) / sc],
             [1.0 / sy, -(2.0 * (1.0 - Kb) * Kb / Kg) / sc, -(2.0 * (1.0 - Kr) * Kr / Kg) / sc],
             [1.0 / sy, 2.0 * (1.0 - Kb) / sc, 0.0]]
    else:
        du, dv = 2.0 * (1.0 - Kb), 2.0 * (1.0 - Kr)
        m = [[Kr * sy, Kg * sy, Kb * sy],
             [-Kr / du * sc, -Kg / du * sc, (1.0 - Kb) / du * sc],
             [(1.0 - Kr) / dv * sc, -Kg / dv * sc, -Kb / dv * sc]]
    return m, [yoff, coff, coff]


def _coef_t(matrix, full_range, bits, direction, dtype):
    m, off = coefficients(matrix, full_range, bits, direction)
    return torch.tensor(m, dtype=torch.float64).to(dtype), torch.tensor(off, dtype=torch.float64).to(dtype)


def chroma_size(h, w, sub=True):
    return ((h + 1) // 2, (w + 1) // 2) if sub else (h, w)


def upsample(c, h, w):
    """[CH, CW] chroma -> [h, w]: 1 at even x, 1/2 + 1/2 at odd x; 3/4 + 1/4 vertically; indices clamped."""
    ch, cw = c.shape
    y = torch.arange(h)
    r = y // 2
    other = torch.where(y % 2 == 0, r - 1, r + 1).clamp(0, ch - 1)
    v = 0.75 * c[r] + 0.25 * c[other]
    x = torch.arange(w)
    k = x // 2
    k1 = (k + 1).clamp(max=cw - 1)
    odd = 0.5 * v[:, k] + 0.5 * v[:, k1]
    return torch.where((x % 2 == 0)[None, :], v[:, k], odd)


def downsample(p):
    """[H, W] -> [ceil(H/2), ceil(W/2)]: [1 2 1] / 4 centred on the even column, then the mean of the two rows; indices clamped."""
    h, w = p.shape
    xe = torch.arange(0, w, 2)
    hf = (0.25 * p[:, (xe - 1).clamp(min=0)] + 0.5 * p[:, xe]) + 0.25 * p[:, (xe + 1).clamp(max=w - 1)]
    ye = torch.arange(0, h, 2)
    return 0.5 * (hf[ye] + hf[(ye + 1).clamp(max=h - 1)])


def yuv_to_rgb(planes, fmt, matrix, full_range, dtype=torch.float32, clamp=False):
    """Three integer numpy planes -> [3, H, W] of ``dtype`` (unclamped unless ``clamp``)."""
    bits, sub = FORMATS[fmt]
    y, u, v = (torch.from_numpy(np.asarray(p).astype(np.int64)).to(dtype) for p in planes)
    h, w = y.shape
    if sub:
        u, v = upsample(u, h, w), upsample(v, h, w)
    m, off = _coef_t(matrix, full_range, bits, 0, dtype)
    a, b, d = y - off[0], u - off[1], v - off[2]
    out = torch.stack([(m[e, 0] * a + m[e, 1] * b) + m[e, 2] * d for e in range(3)])
    return out.clamp(0, 1) if clamp else out


def rgb_to_yuv_values(x, fmt, matrix, full_range, dtype=torch.float32):
    """[3, H, W] -> the three planes BEFORE rounding (offset added), of ``dtype``.  The input is clamped to [0, 1]."""
    bits, sub = FORMATS[fmt]
    x = torch.as_tensor(x).to(dtype).clamp(0, 1)
    m, off = _coef_t(matrix, full_range, bits, 1, dtype)
    r, g, b = x[0], x[1], x[2]
    y = ((m[0, 0] * r + m[0, 1] * g) + m[0, 2] * b) + off[0]
    u = (m[1, 0] * r + m[1, 1] * g) + m[1, 2] * b
    v = (m[2, 0] * r + m[2, 1] * g) + m[2, 2] * b
    if sub:
        u, v = downsample(u), downsample(v)
    return [y, u + off[1], v + off[2]]


def quantise(values, bits):
    """Round half up, clamp to the code range; int64 numpy."""
    return [torch.floor(v + 0.5).clamp(0, (1 << bits) - 1).to(torch.int64).numpy() for v in values]


def rgb_to_yuv(x, fmt, matrix, full_range, dtype=torch.float32):
    return quantise(rgb_to_yuv_values(x, fmt, matrix, full_range, dtype), FORMATS[fmt][0])


def tie_distance(v):
    """Distance of each value to the nearest rounding tie (k + 1/2)."""
    f = v - torch.floor(v)
    return (f - 0.5).abs()


BAND_MARGIN = 4.0              # the tie band is the fp32 restatement's deviation times this (the rule of tests/test_gpu_jpeg.py)
BAND_SHARE = 0.01              # at most this share of a case's samples may lie inside the band


def exit_agreement(got, x, fmt, matrix, full_range):
    """Compare integer planes ``got`` with float64's rounding on tensor ``x``: the figures, ``bad`` = samples that differ outside
    the tie band or by more than 1 code."""
    bits = FORMATS[fmt][0]
    v64 = rgb_to_yuv_values(x, fmt, matrix, full_range, torch.float64)
    v32 = rgb_to_yuv_values(x, fmt, matrix, full_range, torch.float32)
    q64 = quantise(v64, bits)
    dev = max(float((a.double() - b).abs().max()) for a, b in zip(v32, v64))
    band = BAND_MARGIN * dev
    n = in_band = mismatches = bad = 0
    for g, q, v in zip(got, q64, v64):
        g = np.asarray(g).astype(np.int64)
        assert g.shape == q.shape, (g.shape, q.shape)
        inb = (tie_distance(v) <= band).numpy()
        differ = g != q
        n += q.size
        in_band += int(inb.sum())
        mismatches += int(differ.sum())
        bad += int((differ & (~inb | (np.abs(g - q) != 1))).sum())
    return {"band": band, "fp32_deviation": dev, "samples": n, "in_band": in_band, "share": in_band / n, "mismatches": mismatches,
            "bad": bad}


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
def _seed(kind, fmt, h, w):
    return [INPUTS.index(kind), list(FORMATS).index(fmt), h, w, 20261019]


def make_planes(kind, fmt, h, w):
    """Three numpy planes (uint8 / uint16) of a frame going in."""
    bits, sub = FORMATS[fmt]
    ch, cw = chroma_size(h, w, sub)
    dt = np.uint16 if bits > 8 else np.uint8
    top, step = (1 << bits) - 1, 1 << (bits - 8)
    rng = np.random.default_rng(_seed(kind, fmt, h, w))
    shapes = [(h, w), (ch, cw), (ch, cw)]
    if kind == "noise":
        return [rng.integers(16 * step, 236 * step, s).astype(dt) for s in shapes]
    if kind == "constant":
        return [np.full(s, c * step, dtype=dt) for s, c in zip(shapes, (90, 171, 54))]
    if kind == "checker":
        out = []
        for s, (lo, hi) in zip(shapes, ((16, 235), (16, 240), (240, 16))):
            yy, xx = np.indices(s)
            out.append(np.where((yy + xx) % 2 == 0, lo * step, hi * step).astype(dt))
        return out
    if kind == "wild":                                   # the whole code range, below black and above white included
        return [rng.integers(0, top + 1, s).astype(dt) for s in shapes]
    raise ValueError(kind)


def make_tensor(kind, fmt, h, w):
    """[3, H, W] fp32 tensor of a frame going out.  The constant and the checker use values that land away from the rounding ties
    of every combination (tests/test_pixfmt_cpu.py checks the share of samples near a tie for all of them)."""
    rng = np.random.default_rng(_seed(kind, fmt, h, w) + [1])
    if kind == "noise":
        x = rng.random((3, h, w), dtype=np.float32)
    elif kind == "constant":
        x = np.broadcast_to(np.array([0.31372, 0.60781, 0.12943], dtype=np.float32)[:, None, None], (3, h, w)).copy()
    elif kind == "checker":
        yy, xx = np.indices((h, w))
        m = ((yy + xx) % 2 == 0)[None]
        x = np.where(m, np.array([0.9137, 0.0831, 0.4719], dtype=np.float32)[:, None, None],
                     np.array([0.0413, 0.8893, 0.6127], dtype=np.float32)[:, None, None]).astype(np.float32)
    elif kind == "wild":
        # a tenth beyond each end.  (A saturated primary at full range is an exact tie by definition — Cr of pure red is
        # 255.5 — so a wider overshoot, which clamps more pixels onto primaries, spends the tie-band budget on them.)
        x = (rng.random((3, h, w), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    else:
        raise ValueError(kind)
    return torch.from_numpy(np.ascontiguousarray(x))


def padded_pitches(fmt, w, mode):
    """Byte pitches of the three planes: ``packed``, ``pad64`` (rows padded to 64 bytes) or ``odd`` (row + an odd number of samples:
    no wide access is possible)."""
    bits, sub = FORMATS[fmt]
    s = 2 if bits > 8 else 1
    widths = [w, (w + 1) // 2 if sub else w, (w + 1) // 2 if sub else w]
    if mode == "packed":
        return [x * s for x in widths]
    if mode == "pad64":
        return [-(-x * s // 64) * 64 for x in widths]
    if mode == "odd":
        return [(x + 3 + 2 * i) * s for i, x in enumerate(widths)]
    raise ValueError(mode)
