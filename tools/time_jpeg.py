"""Times the JPEG frame encoder of the HIP engine against what a ROCm user of iw3.desktop has without it, and writes
profiles/jpeg.txt:

  frames of 1920 x 1080 and 3840 x 1080 (full SBS) at quality 90, 4:2:0, device frame in to host bytes out;
  the baseline in the same run on the same machine: ``to_uint8``, the copy to the host and one-thread libjpeg through PIL
  (torchvision is not installed here; its CPU route is the same library);
  the engine's four launches alone (HIP events, no host read), per pass, and the HBM fraction the DCT pass reaches;
  the bytes that cross PCIe per frame on either route;
  the ``restart_mcus`` table (8, 16, 32, 64, a whole MCU row): launches alone and stream-size overhead, from which
  ``nunif_amd.nunif.utils.jpeg.DEFAULT_RESTART_MCUS`` is set;
  the tie band of tests/test_gpu_jpeg.py on its seeded inputs (band, margin, coefficients inside it, mismatches).

    python tools/time_jpeg.py [--rounds 7 --out FILE]

Protocol of tools/time_outpaint.py: windows of back-to-back calls after warm-up, the variants alternating round by round in one
process, median and spread (min .. max) over the rounds.  Windows that end on the host (bytes out) are timed with the host clock
around a synchronised window, windows of launches alone with HIP events."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_ref as J  # noqa: E402
from nunif_amd import _hip  # noqa: E402
from nunif_amd.iw3.desktop.utils import to_jpeg_data  # noqa: E402
from nunif_amd.nunif.utils import jpeg as JP  # noqa: E402

HBM_PEAK = 8.0e12                    # bytes / s, MI355X


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
    for _ in range(2):
        for _, fn in variants:
            window(fn, max(1, inner // 10))
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(window(fn, inner))
    return times


def fmt(v):
    return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"


def frame(h, w):
    """Seeded noise over smooth content, as the tests use, at streaming size."""
    g = torch.Generator().manual_seed(7)
    low = torch.rand(1, 3, h // 16 + 1, w // 16 + 1, generator=g)
    up = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=False)[0]
    return torch.clamp(up * 0.9 + 0.1 * torch.rand(3, h, w, generator=g), 0, 1).cuda()


def passes(enc, x, restart, calls=20):
    _hip.profile_enable(True)
    _hip.profile_read(reset=True)
    for _ in range(calls):
        enc.encode_device(x, 90, 420, restart)
    torch.cuda.synchronize()
    recs = {r["name"]: r for r in _hip.profile_read(reset=True) if r["name"].startswith("jpeg_")}
    _hip.profile_enable(False)
    return {k: (r["total_ms"] / calls, r["bytes"] / calls) for k, r in recs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg.txt"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"ms per frame: median (min .. max) of {args.rounds} rounds, the variants alternating round by round; quality 90, 4:2:0",
             f"default restart interval: {JP.DEFAULT_RESTART_MCUS} MCUs (nunif_amd.nunif.utils.jpeg.DEFAULT_RESTART_MCUS)"]
    enc = JP.JpegEncoder("cuda:0")
    with torch.inference_mode():
        for h, w in ((1080, 1920), (1080, 3840)):
            x = frame(h, w)
            x4 = x.unsqueeze(0).contiguous()
            row = J.whole_row(w, 420)
            n_dev = len(to_jpeg_data(x, 90, 0)[0])
            n_host = len(to_jpeg_data(x, 90, 0, gpu_jpeg=False)[0])
            t = alternate([("engine", lambda: to_jpeg_data(x, 90, 0)), ("host", lambda: to_jpeg_data(x, 90, 0, gpu_jpeg=False))],
                          host_window, 10, args.rounds)
            lines.append(f"{w} x {h}: device frame in, host bytes out (to_jpeg_data), 10 calls per window, host clock")
            lines.append(f"  engine  {fmt(t['engine'])}   stream {n_dev} bytes; crosses PCIe: {n_dev + 4} bytes")
            lines.append(f"  host    {fmt(t['host'])}   to_uint8 + D2H + one-thread libjpeg (PIL); stream {n_host} bytes; "
                         f"crosses PCIe: {3 * h * w} bytes")
            lines.append(f"  host / engine {statistics.median(t['host']) / statistics.median(t['engine']):.2f} x")
            lines.append("  restart_mcus table: the four launches alone (HIP events, 50 calls per window) and the stream size")
            variants = [(str(r), (lambda r=r: enc.encode_device(x4, 90, 420, r))) for r in (8, 16, 32, 64, row)]
            tt = alternate(variants, event_window, 50, args.rounds)
            base = len(enc.encode(x, quality=90, restart_mcus=min(65535, row * ((h + 15) // 16)))) - 0
            for r in (8, 16, 32, 64, row):
                n = len(enc.encode(x, quality=90, restart_mcus=r))
                lines.append(f"    restart_mcus {r:>4}{' (row)' if r == row else '      '} {fmt(tt[str(r)])}   {n} bytes, "
                             f"{100.0 * (n - base) / base:+.2f} % over one interval per frame")
            lines.append(f"  passes at restart_mcus {JP.DEFAULT_RESTART_MCUS} (event-timed one by one, so the sum exceeds the "
                         "back-to-back figure):")
            for name, (ms, nbytes) in sorted(passes(enc, x4, JP.DEFAULT_RESTART_MCUS).items(), key=lambda kv: -kv[1][0]):
                extra = f"   {nbytes / 1e6:.1f} MB moved, {100.0 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s" if nbytes else ""
                lines.append(f"    {name:<13} {ms:7.4f} ms{extra}")
        lines.append("tie band of the coefficient comparison (tests/test_gpu_jpeg.py), seeded 64 x 96 frame, per quality and "
                     "subsampling: band = fp32 restatement's largest |c/Q - float64| x margin")
        xs = J.synth(25, 64, 96)
        xd = torch.from_numpy(xs).cuda()
        for ss in (420, 444):
            for q in (1, 50, 90, 100):
                coef = JP.debug_coefficients(xd, q, str(ss))[0].cpu().numpy().astype(np.int64)
                a = J.coefficient_agreement(coef, xs, q, ss)
                lines.append(f"  {ss} q{q:<3}: band {a['band']:.3e} = {a['fp32_deviation']:.3e} x {a['margin']:g}; {a['in_band']} of "
                             f"{a['coefficients']} coefficients in band; {a['mismatches']} mismatches, {a['bad']} outside the rule")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
