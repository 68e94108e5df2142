"""Frames of DIFFERENT sizes through one swin_unet 2x handle at two levels of NUNIF_SWIN_SKIP_PAD (0 = whole tiles, 1 = the level-1
C = 96 blocks skip, 2 = every fast block): what a folder of images pays for the window lists and group tables of pad skipping
 — new ones per frame geometry the first time it is seen, cached ones after.

    python tools/time_skip_pad_sizes.py [--levels 1,2] [--rounds 3] [--out FILE]

Prints, per level, ms per frame of (a) the first pass over the sizes (every geometry new), (b) later passes (every
geometry cached), (c) a stream of never-repeating sizes, and (d) 60 frames of one 1080p geometry on a fresh handle (the
benchmark's single-stream leg, first frame included)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nunif_amd.waifu2x.models.swin_unet import SwinUNet2x  # noqa: E402

SIZES = [(1080, 1920), (720, 1280), (1000, 1500), (540, 960), (900, 1600), (768, 1024), (1200, 800), (480, 854)]


def timed(m, frames):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for x in frames:
        m.render_frame(x, tile_size=256, batch_size=64)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--levels", default="1,2", help="the two NUNIF_SWIN_SKIP_PAD levels to alternate between")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(1)
    frames = [torch.rand(3, h, w, generator=g).to("cuda:0") for h, w in SIZES]
    fresh = [torch.rand(3, 700 + 7 * i, 1100 + 11 * i, generator=g).to("cuda:0") for i in range(24)]      # 24 sizes, each seen once
    res = {}
    lo, hi = a.levels.split(",")
    for on in (lo, hi, lo, hi):
        os.environ["NUNIF_SWIN_SKIP_PAD"] = on                 # read by the library at every call
        m = SwinUNet2x().eval().to("cuda:0")
        m.render_frame(frames[-1][:, :300, :300].contiguous(), tile_size=256, batch_size=64)      # kernels loaded, workspace exists
        m.render_frame(frames[0], tile_size=256, batch_size=64)
        m2 = SwinUNet2x().eval().to("cuda:0")
        m2.render_frame(frames[-1][:, :300, :300].contiguous(), tile_size=256, batch_size=64)
        r = res.setdefault(on, {"first_pass": [], "cached_pass": [], "never_repeating": [], "one_geometry_60_cold": []})
        m3 = SwinUNet2x().eval().to("cuda:0")
        m3.render_frame(frames[1], tile_size=256, batch_size=64)                                   # largest workspace not yet there on purpose: as bench
        m3.render_frame(frames[0][:, :1079].contiguous(), tile_size=256, batch_size=64)             # workspace of 45 tiles exists, the 1080p geometry is new
        r["one_geometry_60_cold"].append(round(timed(m3, [frames[0]] * 60), 3))
        r["first_pass"].append(round(timed(m2, frames[1:]), 3))
        r["cached_pass"].append(round(min(timed(m2, frames[1:]) for _ in range(a.rounds)), 3))
        r["never_repeating"].append(round(timed(m, fresh), 3))
    line = json.dumps({"sizes": SIZES, "ms_per_frame": res})
    print(line)
    if a.out:
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
