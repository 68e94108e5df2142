"""Time the fused HDR planar entry (hdr_planes.hip) against the two routes it stands beside, and record its accuracy.

    python tools/time_hdr_planes.py [--rounds 7 --window 0.2 --out profiles/hdr_planes.txt]

One MI355X, one process.  Per size (1920 x 1080, 3840 x 2160) and curve (PQ, HLG), the source in PINNED host memory (read zero-copy,
as the frame ring hands it over), the result the CHW fp32 tensor on the device; median (min .. max) of `rounds` alternating rounds
of HIP-event windows of at least `window` seconds:
  (a) the fused launch: ``hdr2sdr_planes`` on the yuv420p10le planes (3 B/px across PCIe);
  (b) the two-launch chain it is bit-equal to: ``pixfmt.yuv_to_tensor(planes, frame_out=rgb48)`` + ``hdr2sdr_tensor(rgb48)``;
  (c) today's HDR route as far as the engine sees it: ``hdr_entry`` on an rgb48 frame in pinned memory (6 B/px across PCIe).
      What comes before (c) on the host — libswscale's yuv420p10le -> rgb48le on one thread — is NOT in any figure here: it cannot
      be measured without PyAV.
The accuracy section is the worst ``e_hip / (2.2 * e_ref + 2^-23)`` per curve over the accuracy cases of
tests/test_gpu_hdr_planes.py (whole map and each of the 16 bands of the brightest input code)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdr_planes_ref as R  # noqa: E402
import hdr_ref  # noqa: E402

DEV = "cuda:0"
ACCURACY_SHAPES = [(5, 7), (18, 33), (64, 96), (8, 8192)]


def accuracy(hdr, pixfmt, lines):
    lines.append("accuracy, debug form against float64 on the fp32 restatement's codes; yardstick: the fp32 restatement of the map "
                 "(worst over the whole map and over each of the 16 bands of the brightest input code)")
    worst = {R.PQ: (0.0, ""), R.HLG: (0.0, "")}
    for h, w in ACCURACY_SHAPES:
        lay = pixfmt.PlaneLayout(R.FMT, w, h)
        for trc, cs, full in R.AXES:
            for kind in R.KINDS:
                planes = R.make_planes(kind, h, w)
                v64, _, codes = R.hdr_planes_ref(planes, full, trc, cs, torch.float64)
                v32, _, _ = R.hdr_planes_ref(planes, full, trc, cs, torch.float32)
                got = hdr.hdr2sdr_planes(torch.from_numpy(lay.pack(planes)).to(DEV), lay, full, trc, cs, form="debug").cpu()
                e_hip = (got.double() - v64).abs().amax(dim=2).numpy()
                e_ref = (v32.double() - v64).abs().amax(dim=2).numpy()
                band = hdr_ref.brightest_band(codes)
                ratio = e_hip.max() / (2.2 * e_ref.max() + 2.0 ** -23)
                for b in range(16):
                    m = band == b
                    if m.any():
                        ratio = max(ratio, e_hip[m].max() / (2.2 * e_ref[m].max() + 2.0 ** -23))
                if ratio > worst[trc][0]:
                    worst[trc] = (ratio, f"{kind} {h}x{w} {cs} {'full' if full else 'limited'}")
    for trc, label in ((R.PQ, "PQ"), (R.HLG, "HLG")):
        lines.append(f"  worst e_hip / bound, {label}: {worst[trc][0]:.3f} ({worst[trc][1]})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdr_planes.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_hdr_planes needs a ROCm device")
    from nunif_amd.nunif.utils import hdr, pixfmt

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3                      # seconds

    lines = [f"HDR planar entry (hdr_planes.hip), {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"source in pinned host memory (zero-copy), result CHW fp32 on the device; median (min .. max) of {a.rounds} alternating "
             f"rounds of HIP-event windows of at least {a.window} s", ""]
    for h, w in ((1080, 1920), (2160, 3840)):
        lay = pixfmt.PlaneLayout(R.FMT, w, h)
        rng = np.random.default_rng(7)
        planes = [rng.integers(64, 941, (ph, pw)).astype(np.uint16) for ph, pw in zip(lay.plane_heights, lay.plane_widths)]
        buf = torch.from_numpy(lay.pack(planes)).pin_memory()
        out = torch.empty((3, h, w), dtype=torch.float32, device=DEV)
        tensor = torch.empty((3, h, w), dtype=torch.float32, device=DEV)
        rgb48 = torch.empty((h, w, 3), dtype=torch.int16, device=DEV)
        pixfmt.yuv_to_tensor(buf, lay, R.MATRIX, False, device=DEV, out=tensor, frame_out=rgb48)
        host48 = rgb48.cpu().pin_memory()
        for trc, label in ((R.PQ, "PQ"), (R.HLG, "HLG")):
            entry = hdr.hdr_entry(trc, "bt709")

            def fused():
                hdr.hdr2sdr_planes(buf, lay, False, trc, "bt709", form="chw", out=out, device=DEV)

            def chain():
                pixfmt.yuv_to_tensor(buf, lay, R.MATRIX, False, device=DEV, out=tensor, frame_out=rgb48)
                hdr.hdr2sdr_tensor(rgb48, trc, "bt709", form="chw", out=out)

            def rgb_route():
                entry(host48, device=DEV)

            routes = {"(a) fused launch": fused, "(b) two-launch chain": chain, "(c) hdr_entry on pinned rgb48": rgb_route}
            fused()
            want = out.clone()
            chain()
            same = bool(torch.equal(want, out))
            inner = {}
            for k, fn in routes.items():
                window(fn, 3)
                inner[k] = max(3, int(a.window / (window(fn, 10) / 10)) + 1)
            t = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    t[k].append(window(fn, inner[k]) / inner[k] * 1e6)
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"{w} x {h}, {label}  (fused result bit-equal to the chain's: {same})")
            for k in routes:
                lines.append(f"  {k:30s}: median {med[k]:9.1f} us  ({min(t[k]):.1f} .. {max(t[k]):.1f}), {inner[k]} calls a window")
            ka, kb, kc = routes
            lines.append(f"  per pixel: (a) 3 B over PCIe, 12 B stored; (b) 3 B over PCIe, 12 + 6 B stored, 6 B read again, 12 B stored; "
                         f"(c) 6 B over PCIe, 12 B stored")
            lines.append(f"  (b) / (a) = {med[kb] / med[ka]:.2f}   (c) / (a) = {med[kc] / med[ka]:.2f}")
            lines.append("")
    lines.append("not measured: libswscale's host time for yuv420p10le -> rgb48le in front of route (c) (no PyAV here)")
    lines.append("")
    accuracy(hdr, pixfmt, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
