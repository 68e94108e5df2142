"""Time the frame edge with planar YUV ends (pixfmt.hip) against the rgb edge it replaces, on pinned host buffers.

    python tools/time_pixfmt.py [--rounds 7 --inner 10 --out profiles/pixfmt.txt]

Two routes in the same run, at 1080p and 4K, for yuv420p and yuv420p10le:
  * planar: pinned planes -> ``yuv_to_tensor`` -> CHW fp32 on the device, then ``tensor_to_yuv`` -> pinned planes;
  * rgb (the edge as it was): pinned rgb24 / rgb48 -> ``frame_to_tensor``, then ``to_frame`` -> pinned rgb24 / rgb48.
Each window is a pair of HIP events around ``--inner`` launches of one direction; the routes alternate round by round; medians with
min and max.  "Not slower" is judged against the spread between rounds that this run itself shows.  The two host ``reformat`` calls
are timed only where PyAV imports.  No end-to-end figure is derived from this."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixfmt.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pixfmt needs a ROCm device")
    from nunif_amd.iw3 import _ops
    from nunif_amd.nunif.utils import pixfmt

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner * 1e3

    lines = [f"Frame edge with planar YUV ends (pixfmt.hip) against the rgb edge, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"pinned host buffers on both routes (zero-copy over PCIe); medians of {a.rounds} alternating rounds; each window: HIP "
             f"events around {a.inner} launches", ""]
    verdicts = []
    for h, w in ((1080, 1920), (2160, 3840)):
        for fmt in ("yuv420p", "yuv420p10le"):
            lay = pixfmt.PlaneLayout(fmt, w, h)
            rng = np.random.default_rng(1)
            top = 1 << lay.bits
            planes = [rng.integers(0, top, (ph, pw)).astype(lay.numpy_dtype) for ph, pw in zip(lay.plane_heights, lay.plane_widths)]
            p_in = torch.from_numpy(lay.pack(planes)).pin_memory()
            p_out = torch.zeros(lay.nbytes, dtype=torch.uint8).pin_memory()
            bits = 16 if lay.bits > 8 else 8
            rgb = rng.integers(0, 256 if bits == 8 else 65536, (h, w, 3))
            rgb = torch.from_numpy(rgb.astype(np.uint8) if bits == 8 else rgb.astype(np.uint16).view(np.int16))
            r_in = rgb.pin_memory()
            r_out = torch.empty_like(rgb).pin_memory()
            x = torch.rand((3, h, w), device=DEV)
            runs = {
                # like for like: both entries allocate their tensor per call (caching allocator), both exits write a given buffer
                "planar in ": lambda: events(lambda: pixfmt.yuv_to_tensor(p_in, lay, "bt709", False, device=DEV)),
                "rgb in    ": lambda: events(lambda: _ops.frame_to_tensor(r_in, device=DEV)),
                "planar out": lambda: events(lambda: pixfmt.tensor_to_yuv(x, lay, "bt709", False, out=p_out)),
                "rgb out   ": lambda: events(lambda: _ops.to_frame(x, bits, out=r_out)),
            }
            for fn in runs.values():
                for _ in range(2):
                    fn()
            t = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    t[k].append(fn())
            med = {k: statistics.median(v) for k, v in t.items()}
            sample = lay.sample_bytes
            pb = sum(pw * ph for pw, ph in zip(lay.plane_widths, lay.plane_heights)) * sample
            rb = h * w * 3 * (2 if bits == 16 else 1)
            lines.append(f"{w} x {h}, {fmt}")
            for k in runs:
                lines.append(f"  {k}: median {med[k]:9.1f} us  (min {min(t[k]):.1f}, max {max(t[k]):.1f})")
            lines.append(f"  bytes over PCIe per frame and direction: planar {pb / 1e6:.2f} MB ({pb / (h * w):.1f} B/px), "
                         f"rgb {rb / 1e6:.2f} MB ({rb / (h * w):.1f} B/px)")
            planar, edge = med["planar in "] + med["planar out"], med["rgb in    "] + med["rgb out   "]
            # the spread of one route's edge: the ranges of its two directions; the comparison allows the larger of the two routes'
            spread = max(sum(max(t[k]) - min(t[k]) for k in runs if k.startswith(route)) for route in ("planar", "rgb"))
            ok = planar <= edge + spread
            verdicts.append(ok)
            lines.append(f"  edge, both directions: planar {planar:.1f} us, rgb {edge:.1f} us, spread between rounds {spread:.1f} us -> "
                         f"planar is {'not slower' if ok else 'SLOWER'} ({edge / planar:.2f} x)")
            lines.append("")
    try:
        import av
        for h, w in ((1080, 1920), (2160, 3840)):
            for fmt, rgbfmt in (("yuv420p", "rgb24"), ("yuv420p10le", "rgb48le")):
                f = av.VideoFrame(w, h, fmt)
                ts = []
                for _ in range(a.rounds + 2):
                    t0 = time.perf_counter()
                    g = f.reformat(format=rgbfmt, src_colorspace=1, dst_colorspace=1, src_color_range=1, dst_color_range=2)
                    t1 = time.perf_counter()
                    g.reformat(format=fmt, src_colorspace=1, dst_colorspace=1, src_color_range=2, dst_color_range=1)
                    t2 = time.perf_counter()
                    ts.append(((t1 - t0) * 1e6, (t2 - t1) * 1e6))
                ts = ts[2:]
                lines.append(f"swscale {w} x {h} {fmt}: reformat in median {statistics.median(x[0] for x in ts):.0f} us, out "
                             f"{statistics.median(x[1] for x in ts):.0f} us (one host thread)")
    except ImportError:
        lines.append("swscale: not measured (no PyAV)")
    lines.append("whole pipeline: not measured (no real file was run through iw3.cli or waifu2x.cli)")
    lines.append("condition (planar edge not slower than the rgb edge at either size): " + ("met" if all(verdicts) else "NOT met"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
