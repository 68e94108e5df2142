"""Restatement of the statistics behind ``AutoCropDetector.detect_tb`` / ``detect_lr`` (nunif/utils/autocrop.py:117-170, reference)
in plain torch at a chosen dtype: float64 is the yardstick of tests/test_gpu_autocrop.py, the float32 run is what
tests/golden/autocrop.npz records.  Same expressions, same order; nothing here is shared with nunif_amd."""
import torch

LO, HI = 16.0 / 255.0, 235.0 / 255.0
DARK, DEV, FRAC = 32.0 / 255.0, 16.0 / 255.0, 0.99
# (first statistic's threshold, second statistic's threshold) of a kind; None: the statistic is compared with nothing
THRESHOLDS = {"black": (DARK, DEV), "flat": (None, FRAC)}


def rgb_to_y(x, tv_range):
    r, g, b = x[..., 0:1, :, :], x[..., 1:2, :, :], x[..., 2:3, :, :]
    y = r * 0.299 + g * 0.587 + b * 0.114
    if tv_range:
        y = y.clamp(min=LO, max=HI)
    return y


def stats(x, kind, dtype=torch.float64):
    """``x`` [3,H,W] or [B,3,H,W] -> dict of ``row_a``, ``row_b`` [B,H] and ``col_a``, ``col_b`` [B,W] at ``dtype``: the mean and
    max |y - mean| of the black modes, the lower median and the fraction of |y - median| < 16/255 of the flat modes."""
    if x.ndim == 3:
        x = x.unsqueeze(0)
    y = rgb_to_y(x.to(dtype), tv_range=kind == "black")
    out = {}
    for name, dim in (("row", -1), ("col", -2)):
        if kind == "black":
            a = y.mean(dim=dim, keepdim=True)
            b = (y - a).abs().amax(dim=dim, keepdim=True)
        else:
            a = y.median(dim=dim, keepdim=True).values
            b = ((y - a).abs() < DEV).to(dtype).mean(dim=dim, keepdim=True)
        out[name + "_a"], out[name + "_b"] = a.flatten(1), b.flatten(1)
    return out


def masks(st, kind):
    """The decisions of :func:`stats` output: bool ``tb`` [B,H] and ``lr`` [B,W]."""
    res = {}
    for name, key in (("row", "tb"), ("col", "lr")):
        a, b = st[name + "_a"], st[name + "_b"]
        res[key] = ((a <= DARK) & (b < DEV)) if kind == "black" else (b > FRAC)
    return res


def margin(st, kind):
    """The smallest distance of a statistic of ``st`` from the threshold it is compared with."""
    ta, tb = THRESHOLDS[kind]
    m = float("inf")
    for name in ("row", "col"):
        if ta is not None:
            m = min(m, float((st[name + "_a"].double() - ta).abs().min()))
        m = min(m, float((st[name + "_b"].double() - tb).abs().min()))
    return m


def mask_to_slice(mask):
    """``mask_to_slice_tb`` / ``_lr`` (:172-207) on a flat bool mask."""
    keep = torch.nonzero(~mask.flatten()).flatten()
    if keep.numel() == mask.numel() or keep.numel() == 0:
        return slice(None, None)
    first, last = int(keep[0]), int(keep[-1]) + 1
    return slice(first if first > 0 else None, last if last < mask.numel() else None)


def apply_mod(s, mod):
    start, stop = s.start, s.stop
    if start is not None and start % mod != 0:
        start = start + (mod - start % mod)
    if stop is not None and stop % mod != 0:
        stop = stop - stop % mod
    return slice(start, stop)


def slices(mask_tb, mask_lr, mode, mod):
    """``AutoCropDetector.detect`` :86-100 from the two masks of one frame."""
    tb = apply_mod(mask_to_slice(mask_tb), mod) if not mode.endswith("_lr") else slice(None)
    lr = apply_mod(mask_to_slice(mask_lr), mod) if not mode.endswith("_tb") else slice(None)
    return tb, lr
