"""The source files of the waifu2x image-route tests: 40 x 56 images in the modes RGB, RGBA, L, LA and P with tRNS, written as PNG
from seeded noise over a gradient.  tests/golden/waifu2x_image_meta.json holds what the reference's ``pil_io.load_image`` answers
for exactly these files."""
import os

import numpy as np
from PIL import Image
from PIL.PngImagePlugin import PngInfo

H, W = 40, 56
MODES = ["RGB", "RGBA", "L", "LA", "P"]


def source_image(mode, seed=0):
    rng = np.random.default_rng(100 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = ((xx * 3 + yy * 2) % 256).astype(np.int32)
    planes = [np.clip(base + rng.integers(-20, 21, (H, W)) + 30 * k, 0, 255).astype(np.uint8) for k in range(3)]
    alpha = np.where((xx // 8 + yy // 8) % 2 == 0, 255, rng.integers(0, 256, (H, W))).astype(np.uint8)
    if mode == "RGB":
        return Image.fromarray(np.stack(planes, axis=2), "RGB")
    if mode == "RGBA":
        return Image.fromarray(np.stack(planes + [alpha], axis=2), "RGBA")
    if mode == "L":
        return Image.fromarray(planes[0], "L")
    if mode == "LA":
        return Image.fromarray(np.stack([planes[0], alpha], axis=2), "LA")
    im = Image.fromarray(np.stack(planes, axis=2), "RGB").quantize(16)
    im.info["transparency"] = 3                                          # palette entry 3 is transparent: a tRNS chunk
    return im


def write_sources(directory, gamma=None):
    """-> {mode: file}"""
    out = {}
    for k, mode in enumerate(MODES):
        name = os.path.join(str(directory), f"src_{mode.lower()}.png")
        info = PngInfo()
        if gamma is not None:
            info.add(b"gAMA", int(gamma * 100000).to_bytes(4, "big"))
        im = source_image(mode, k)
        im.save(name, pnginfo=info, **({"transparency": 3} if mode == "P" else {}))
        out[mode] = name
    return out
