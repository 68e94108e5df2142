"""Times the PNG frame encoder of the HIP engine against what a ROCm user of ``iw3 --export`` has without it, and writes
profiles/png.txt:

  1920 x 1080 RGB from f32, 1920 x 1080 RGB from u8 and 518 x 924 grey 16 (smooth content under noise), and two compressible
  1920 x 1080 frames (smooth; posterised with black bars), device frame in to host bytes out;
  the baseline in the same run on the same machine: the copy to the host and one-thread libpng through PIL at compress_level 6
  into a BytesIO, on the same frames, and the file sizes of both;
  the engine's five launches alone (HIP events, no host read) and launch by launch;
  the ``stripe_rows`` table (4, 8, 16, 32, 64): launches alone and body size, from which
  ``nunif_amd.nunif.utils.png.DEFAULT_STRIPE_ROWS`` is set: the fastest setting whose size stays within 2 % of the smallest on
  every frame of the run;
  the size ratios of tests/test_png_cpu.py (restatement against libpng), which need no GPU.

    python tools/time_png.py [--rounds 7 --out FILE]

Protocol of tools/time_jpeg.py: windows of back-to-back calls after warm-up, the variants alternating round by round in one
process, median and spread (min .. max) over the rounds.  Windows that end on the host (bytes out) are timed with the host clock
around a synchronised window, windows of launches alone with HIP events."""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import png_ref as R  # noqa: E402
from nunif_amd import _hip  # noqa: E402
from nunif_amd.nunif.utils import png as P  # noqa: E402

STRIPES = (4, 8, 16, 32, 64)


def event_window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def host_window(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1000.0 / inner


def alternate(variants, window, inner, rounds):
    for _, fn in variants:
        window(fn, max(1, inner // 5))
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(window(fn, inner))
    return times


def fmt(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def smooth_noise(c, h, w):
    """Seeded noise over smooth content, as the tests use, at export size."""
    g = torch.Generator().manual_seed(7)
    low = torch.rand(1, c, h // 16 + 1, w // 16 + 1, generator=g)
    up = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
    return torch.clamp(up * 0.9 + 0.1 * torch.rand(c, h, w, generator=g), 0, 1)


def smooth(h, w):
    low = torch.rand(1, 3, 5, 9, generator=torch.Generator().manual_seed(4))
    return torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1)


def poster_bars(h, w):
    x = (smooth(h, w) * 6).floor() / 6
    x[:, :h // 8] = 0
    x[:, -(h // 8):] = 0
    return x


def pil_png(pix):
    buf = io.BytesIO()
    Image.fromarray(pix).save(buf, format="png", compress_level=6)
    return buf.getvalue()


def passes(enc, x, form, stripe_rows, calls=10):
    _hip.profile_enable(True)
    _hip.profile_read(reset=True)
    for _ in range(calls):
        enc.encode_device(x, form, stripe_rows)
    torch.cuda.synchronize()
    recs = {r["name"]: r for r in _hip.profile_read(reset=True) if r["name"].startswith("png_")}
    _hip.profile_enable(False)
    return {k: r["total_ms"] / calls for k, r in recs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png.txt"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"ms per frame: median (min .. max) of {args.rounds} rounds, the variants alternating round by round",
             f"default stripe: {P.DEFAULT_STRIPE_ROWS} rows (nunif_amd.nunif.utils.png.DEFAULT_STRIPE_ROWS)"]
    enc = P.PngEncoder("cuda:0")
    with torch.inference_mode():
        rgb = smooth_noise(3, 1080, 1920)
        cases = [("1920 x 1080 RGB from f32", rgb.cuda(), R.RGB8_F32),
                 ("1920 x 1080 RGB from u8", torch.from_numpy(R.pixels(rgb.numpy(), R.RGB8_F32).copy()).cuda(), R.RGB8_U8),
                 ("924 x 518 grey 16", smooth_noise(1, 518, 924).cuda(), R.GRAY16_F32),
                 ("1920 x 1080 RGB from f32, smooth", smooth(1080, 1920).cuda(), R.RGB8_F32),
                 ("1920 x 1080 RGB from f32, posterised with bars", poster_bars(1080, 1920).cuda(), R.RGB8_F32)]
        within, total_ms = set(STRIPES), {s: 0.0 for s in STRIPES}
        for title, x, form in cases:
            pix = R.pixels(x.cpu().numpy(), form)

            def host_route():
                if form == R.RGB8_F32:
                    a = (torch.clamp(x, 0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
                elif form == R.RGB8_U8:
                    a = x.cpu().numpy()
                else:
                    a = (0xffff * torch.clamp(x, 0, 1)).to(torch.int32).squeeze(0).cpu().numpy().astype("uint16")
                return pil_png(a)

            data = enc.encode(x)
            im = Image.open(io.BytesIO(data))
            im.load()
            assert np.array_equal(np.asarray(im), pix), "the engine's file does not decode to the input"
            n_lib = len(host_route())
            raw = pix.size * pix.itemsize
            t = alternate([("engine", lambda: enc.encode(x)), ("host", host_route)], host_window, 3, args.rounds)
            lines.append(f"{title}: device frame in, host bytes out, 3 calls per window, host clock; raw {raw} bytes")
            lines.append(f"  engine  {fmt(t['engine'])}   file {len(data)} bytes")
            lines.append(f"  host    {fmt(t['host'])}   D2H + one-thread libpng level 6 (PIL); file {n_lib} bytes")
            lines.append(f"  host / engine {statistics.median(t['host']) / statistics.median(t['engine']):.1f} x; "
                         f"engine / libpng size {len(data) / n_lib:.4f}")
            x4 = x.unsqueeze(0).contiguous()
            tt = alternate([(str(s), (lambda s=s: enc.encode_device(x4, form, s))) for s in STRIPES], event_window, 10, args.rounds)
            sizes = {s: len(enc.encode(x, stripe_rows=s)) for s in STRIPES}
            small = min(sizes.values())
            ok = [s for s in STRIPES if sizes[s] <= small * 1.02]
            pick = min(ok, key=lambda s: statistics.median(tt[str(s)]))
            within &= set(ok)
            for s in STRIPES:
                total_ms[s] += statistics.median(tt[str(s)])
            lines.append("  stripe_rows table: the five launches alone (HIP events, 10 calls per window) and the file size")
            for s in STRIPES:
                lines.append(f"    stripe_rows {s:>3} {fmt(tt[str(s)])}   {sizes[s]} bytes, {100.0 * (sizes[s] - small) / small:+.2f} % "
                             f"over the smallest{'   <- fastest within 2 %' if s == pick else ''}")
            lines.append(f"  launches at stripe_rows {P.DEFAULT_STRIPE_ROWS} (event-timed one by one, so the sum exceeds the "
                         "back-to-back figure):")
            for name, ms in sorted(passes(enc, x4, form, P.DEFAULT_STRIPE_ROWS).items(), key=lambda kv: -kv[1]):
                lines.append(f"    {name:<12} {ms:8.4f} ms")
        lines.append(f"within 2 % of the smallest on every frame: stripe_rows {sorted(within)}; the fastest of them over all frames: "
                     f"{min(within, key=lambda s: total_ms[s]) if within else 'none'}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
