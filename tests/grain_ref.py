"""Helpers of the film-grain tests (tests/test_grain_cpu.py, tests/test_gpu_grain.py): a float64 restatement of the reference's
``nunif/utils/rgb_noise.py`` and of the video loop's noise-buffer blend (``waifu2x/ui_utils.py:167-175``), torch's nearest-resize
index rule, and the moment statistics of a noise field with the standard errors that follow from the sample count.

No engine code is imported here: the CPU tests run these on ``torch.randn`` to prove the arithmetic, the GPU tests on the engine."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def apply64(rgb, noise, strength=0.2, gamma=2.2, light_decay=True, light_decay_strength=0.8):
    """apply_rgb_noise (rgb_noise.py:21-39) in float64 on numpy arrays."""
    rgb, noise = np.asarray(rgb, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    out = rgb ** gamma
    weight = ((1.0 - out) * light_decay_strength + (1.0 - light_decay_strength)) ** gamma if light_decay else 1.0
    out = out + noise * out * (weight * strength)
    return np.clip(out, 0.0, 1.0) ** (1.0 / gamma)


def blend64(buf, noise, speed):
    """ui_utils.py:169-174 in float64; ``buf`` None: the first frame (or a shape change)."""
    noise = np.asarray(noise, dtype=np.float64)
    return noise.copy() if buf is None else np.asarray(buf, dtype=np.float64) * (1.0 - speed) + noise * speed


def blend32(buf, noise, speed):
    """The same step with the reference's fp32 roundings (mul_ by the fp32 scalars, then add_)."""
    noise = np.asarray(noise, dtype=np.float32)
    if buf is None:
        return noise.copy()
    return (np.asarray(buf, dtype=np.float32) * np.float32(1.0 - speed) + noise * np.float32(speed)).astype(np.float32)


def quantise(x, bits):
    """video.py:236-245 `(x * max).round()` on an fp32 or float64 array (numpy rounds half to even, as torch does)."""
    maxv = 255.0 if bits == 8 else 65535.0
    x = np.asarray(x)
    return np.rint(np.clip(x, 0, 1) * x.dtype.type(maxv)).astype(np.int64)


def step_shares(a, b):
    """(share of values that differ by exactly one step, largest step) between two quantised arrays."""
    d = np.abs(np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64))
    return float((d == 1).mean()), int(d.max())


def nearest_index(out_size, in_size):
    """torch's `nearest` source index: min(floor(dst * scale), in - 1), scale = fp32(in / out), product in fp32."""
    scale = np.float32(in_size) / np.float32(out_size)
    idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def rgb_noise_like_torch(shape, level=2, generator=None, parts=False):
    """rgb_noise_like (rgb_noise.py:5-18) on torch.randn; parts=True also returns (n1, n2 grid)."""
    shape = tuple(shape)
    n1 = torch.randn(shape, generator=generator)
    if level == 1:
        return (n1, n1, None) if parts else n1
    n2 = torch.randn(shape[:-2] + (shape[-2] // 2, shape[-1] // 2), generator=generator)
    up = F.interpolate(n2.reshape((-1,) + n2.shape[-3:]), size=shape[-2:], mode="nearest").reshape(shape)
    noise = n1 * 0.5 + up * 0.5
    return (noise, n1, n2) if parts else noise


def _pairs(field, axis, inside):
    """Products of neighbours along `axis` (-1 or -2) of a [..., H, W] field: pairs inside one 2x2 cell (even index, +1) or
    across a cell border (odd index, +1).  Even sizes only."""
    f = field if axis == -1 else field.transpose(-1, -2)
    n = f.shape[-1]
    if inside:
        a, b = f[..., 0:n:2], f[..., 1:n:2]
    else:
        a, b = f[..., 1:n - 1:2], f[..., 2:n:2]
    return a * b


def moments(field, level):
    """{name: (value, expectation, standard error)} for a [C, H, W] float64 field of rgb_noise_like(level), H and W even.

    With a, a' ~ N(0,1) per pixel and b ~ N(0,1) per 2x2 cell, level 2 is x = (a + b) / 2.  All terms of the products below are
    uncorrelated (odd moments vanish), so variances add; a term in b alone is shared by the pixels (4) or the pairs (2) of a cell
    and counts once per cell.  N = samples, M = pairs.
      mean:      level 1  1/N;             level 2  (1/4)(1/N) + (1/4)(4/N)                       = 1.25/N
      variance:  level 1  2/N (E x^4 - 1); level 2  x^2 = (a^2 + 2ab + b^2)/4: (1/16)(2/N + 4/N + 2*4/N)   = 0.875/N
      inside:    E = 1/4; xy = (aa' + ab + a'b + b^2)/4: (1/16)(3/M + 2*2/M)                     = 0.4375/M
      across:    E = 0;   xy = (aa' + ab' + a'b + bb')/4: (1/16)(3/M + 2/M)                      = 0.3125/M
      kurtosis (level 1 only, i.i.d.): excess m4/m2^2 - 3, variance 24/N."""
    f = torch.as_tensor(field, dtype=torch.float64)
    n = f.numel()
    out = {}
    if level == 1:
        out["mean"] = (f.mean().item(), 0.0, math.sqrt(1.0 / n))
        out["variance"] = ((f * f).mean().item(), 1.0, math.sqrt(2.0 / n))
        m2, m4 = (f ** 2).mean().item(), (f ** 4).mean().item()
        out["excess_kurtosis"] = (m4 / m2 ** 2 - 3.0, 0.0, math.sqrt(24.0 / n))
        return out
    assert f.shape[-1] % 2 == 0 and f.shape[-2] % 2 == 0
    out["mean"] = (f.mean().item(), 0.0, math.sqrt(1.25 / n))
    out["variance"] = ((f * f).mean().item(), 0.5, math.sqrt(0.875 / n))
    for name, axis in (("h", -1), ("v", -2)):
        p = _pairs(f, axis, True)
        out[f"cov_inside_{name}"] = (p.mean().item(), 0.25, math.sqrt(0.4375 / p.numel()))
        p = _pairs(f, axis, False)
        out[f"cov_across_{name}"] = (p.mean().item(), 0.0, math.sqrt(0.3125 / p.numel()))
    return out


def cross_moment(x, y, level):
    """(mean(x * y), 0, standard error) for two independent fields of the same level: level 1  1/N; level 2
    xy = (aa' + ab' + ba' + bb')/4: (1/16)(3/N + 4/N) = 0.4375/N."""
    x, y = torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64)
    n = x.numel()
    return (x * y).mean().item(), 0.0, math.sqrt((1.0 if level == 1 else 0.4375) / n)


def check_moments(stats, k=5.0):
    """Names of the statistics further than k standard errors from their expectation (empty = pass); prints every figure."""
    bad = []
    for name, (value, expect, se) in stats.items():
        z = (value - expect) / se
        print(f"    {name:18s} {value:+.6f}  expect {expect:+.4f}  se {se:.2e}  z {z:+.2f}")
        if not abs(z) <= k:
            bad.append((name, value, expect, se))
    return bad
