"""Times the output step of the waifu2x image route on the HIP engine against what the reference does with the same device
tensors, and writes profiles/waifu2x_images.txt:

  a 3840 x 2160 RGBA frame with alpha = 1 and a 3840 x 2160 grey frame (three colour planes under ``meta["grayscale"]``), smooth
  content under noise, device tensors in to the bytes of a PNG file on the host;
  the engine: ``PngEncoder.encode(rgb, alpha=...)`` / ``encode(rgb, gray=True)`` (nunif_amd/nunif/utils/png.py);
  the host route in the same run: ``.cpu()``, the PIL image as ``to_image`` makes it, ``convert("L")`` for the grey frame, libpng
  at compress_level 6 into a BytesIO (nunif/utils/pil_io.py:240-323 of the reference) on one thread, and the same with the
  libpng step of 8 frames on 8 pool threads (the copy to the host stays on the calling thread, as in ``process_image``);
  the file sizes of both.

    python tools/time_waifu2x_images.py [--rounds 7 --out FILE]

Protocol of tools/time_png.py: the variants alternate round by round in one process after a warm-up; median and spread
(min .. max) over the rounds; host clock around a synchronised window.  No speed-up is asserted; the figures to compare with are
those of profiles/png.txt."""
import argparse
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nunif_amd.nunif.utils import png as P  # noqa: E402
from nunif_amd.waifu2x.ui_utils import to_image  # noqa: E402

H, W, POOL = 2160, 3840, 8


def smooth_noise(c, h, w):
    g = torch.Generator().manual_seed(7)
    low = torch.rand(1, c, h // 16 + 1, w // 16 + 1, generator=g)
    up = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
    return torch.clamp(up * 0.9 + 0.1 * torch.rand(c, h, w, generator=g), 0, 1)


def window(fn, frames):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000.0 / frames


def fmt(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def libpng(im, gray):
    if gray:
        im = im.convert("LA" if im.mode == "RGBA" else "L")
    buf = io.BytesIO()
    im.save(buf, format="png", compress_level=6)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waifu2x_images.txt"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"ms per frame: median (min .. max) of {args.rounds} rounds, the variants alternating round by round, host clock",
             f"stripe: {P.DEFAULT_STRIPE_ROWS} rows"]
    enc = P.PngEncoder("cuda:0")
    rgb = smooth_noise(3, H, W).cuda()
    ones = torch.ones(1, H, W, device="cuda:0")
    cases = [(f"{W} x {H} RGBA, alpha = 1", ones, False), (f"{W} x {H} grey from three planes", None, True)]
    with torch.inference_mode(), ThreadPoolExecutor(max_workers=POOL) as pool:
        for title, alpha, gray in cases:
            def engine():
                return enc.encode(rgb, alpha=alpha, gray=gray)

            def host_image():
                return to_image(rgb.cpu(), alpha.cpu() if alpha is not None else None)

            def host_one():
                return libpng(host_image(), gray)

            def host_pool():
                for f in [pool.submit(libpng, host_image(), gray) for _ in range(POOL)]:
                    f.result()

            data, ref = engine(), host_one()
            a, b = Image.open(io.BytesIO(data)), Image.open(io.BytesIO(ref))
            assert a.mode == b.mode and np.array_equal(np.asarray(a), np.asarray(b)), "the two routes decode to different pixels"
            variants = [("engine", engine, 1), ("host 1 thread", host_one, 1), (f"host {POOL} threads", host_pool, POOL)]
            for _, fn, _ in variants:
                fn()
            times = {name: [] for name, _, _ in variants}
            for _ in range(args.rounds):
                for name, fn, frames in variants:
                    times[name].append(window(fn, frames))
            raw = H * W * len(a.getbands())
            lines.append(f"{title}: device tensors in, file bytes out; mode {a.mode}, raw {raw} bytes")
            lines.append(f"  engine          {fmt(times['engine'])}   file {len(data)} bytes")
            lines.append(f"  host 1 thread   {fmt(times['host 1 thread'])}   D2H + to_image + libpng level 6 (PIL); file {len(ref)} bytes")
            lines.append(f"  host {POOL} threads  {fmt(times[f'host {POOL} threads'])}   per frame, {POOL} frames in flight")
            e = statistics.median(times["engine"])
            lines.append(f"  host 1 thread / engine {statistics.median(times['host 1 thread']) / e:.1f} x; "
                         f"host {POOL} threads / engine {statistics.median(times[f'host {POOL} threads']) / e:.1f} x; "
                         f"engine / libpng size {len(data) / len(ref):.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
