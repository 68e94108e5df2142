"""Writes tests/golden/rgb_noise.npz from the LIVE reference (imported through oracle/refstub.py): inputs, recorded noise and the
reference's fp32 results of ``nunif/utils/rgb_noise.py`` ``apply_rgb_noise``, also over three steps of the video loop's noise-buffer
blend (``waifu2x/ui_utils.py:167-175``, restated as ``grain_ref.blend32``).  Run from the repository root:  python tests/golden/make_golden_grain.py

Inputs carry a ramp, exact 0 and 1 and a dark patch (values below 0.02): ``x ** (1 / 2.2)`` has unbounded slope at 0."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refstub  # noqa: E402

refstub.install()
from nunif.utils.rgb_noise import apply_rgb_noise, rgb_noise_like  # noqa: E402

import grain_ref as G  # noqa: E402

# name: (strength, gamma, light_decay)
APPLY_CASES = {"s01": (0.1, 2.2, True), "s02": (0.2, 2.2, True), "s10": (1.0, 2.2, True),
               "s01_flat": (0.1, 2.2, False), "s02_flat": (0.2, 2.2, False), "s10_flat": (1.0, 2.2, False),
               "s02_g18": (0.2, 1.8, True)}
SPEEDS = {"v08": 0.8, "v03": 0.3}


def image(seed, c, h, w):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(c, h, w, generator=g)
    x[:, : h // 6] = torch.linspace(0, 1, w)[None, None, :]                         # ramp, ends exact
    x[:, h // 6: h // 3, : w // 2] = torch.rand(c, h // 3 - h // 6, w // 2, generator=g) * 0.02      # dark patch
    x[:, h // 3: h // 3 + 4, : w // 4] = 0.0
    x[:, h // 3: h // 3 + 4, w // 4: w // 2] = 1.0
    return x


def main():
    out = {}
    torch.manual_seed(20260116)
    x3 = image(1, 3, 48, 80)
    n3 = rgb_noise_like(x3)
    out["x3"], out["noise3"] = x3.numpy(), n3.numpy()
    for name, (s, gm, ld) in APPLY_CASES.items():
        y = apply_rgb_noise(x3.clone(), n3.clone(), strength=s, gamma=gm, light_decay=ld).numpy()
        out[f"apply_{name}"] = y
        ref = G.apply64(out["x3"], out["noise3"], s, gm, ld)
        out[f"shares_{name}"] = np.array([*G.step_shares(G.quantise(y, 8), G.quantise(ref, 8)),
                                          *G.step_shares(G.quantise(y, 16), G.quantise(ref, 16))], dtype=np.float64)
    x4 = torch.stack([image(2, 3, 24, 40), image(3, 3, 24, 40)])
    n4 = rgb_noise_like(x4)
    out["x4"], out["noise4"] = x4.numpy(), n4.numpy()
    out["apply4_s02"] = apply_rgb_noise(x4.clone(), n4.clone(), strength=0.2).numpy()
    # three consecutive frames of the video loop, the noise buffer empty at the start: the fp32 recurrence of grain_ref.blend32
    # (scale the buffer, scale the fresh noise, add) on torch tensors, then the reference's apply_rgb_noise on the buffer
    xv = torch.stack([image(10 + i, 3, 24, 40) for i in range(3)])
    nv = torch.stack([rgb_noise_like(xv[i]) for i in range(3)])
    out["video_x"], out["video_noise"] = xv.numpy(), nv.numpy()
    for name, speed in SPEEDS.items():
        buf, bufs, ys = None, [], []
        for i in range(3):
            buf = nv[i].clone() if buf is None else torch.mul(buf, 1.0 - speed) + torch.mul(nv[i], speed)
            assert np.array_equal(buf.numpy(), G.blend32(bufs[-1] if bufs else None, out["video_noise"][i], speed))
            bufs.append(buf.numpy().copy())
            ys.append(apply_rgb_noise(xv[i].clone(), buf.clone(), strength=0.2).numpy())
        out[f"video_buf_{name}"], out[f"video_out_{name}"] = np.stack(bufs), np.stack(ys)
    path = os.path.join(ROOT, "tests", "golden", "rgb_noise.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
