"""Times the letterbox detector of iw3 --autocrop on the HIP engine against eager torch-ROCm on the same GPU and writes
profiles/autocrop.txt: ``AutoCropDetector.update`` on batches of 2 frames at 1080p and 4K, modes ``black`` and ``flat``.

The torch side is the reference's own sequence of expressions (nunif/utils/autocrop.py:24-48, :117-170: per frame ``rgb_to_y``,
mean / amax or median / mean per axis, the counters added as int tensors) restated in tools/ so that it runs without the
reference checkout.  The file also carries the worst error ratio per statistic of tests/test_gpu_autocrop.py
(``e_hip / (2.2 * e_ref + 2^-23)`` against float64 over the shared inputs).

    python tools/time_autocrop.py [--rounds 7 --out FILE]

HIP events around ``inner`` back-to-back calls, ``inner`` chosen per variant so that a window is 0.25 s or longer, after warm-up,
the two variants alternating round by round in one process; reports the median and the spread (min, max) over the rounds."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import autocrop_cases as C  # noqa: E402
import autocrop_f64 as R  # noqa: E402
from nunif_amd.nunif.utils import autocrop as E  # noqa: E402

WINDOW_S = 0.25


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner                            # ms per call


def alternate(variants, rounds):
    inner = {}
    for name, fn in variants:
        window(fn, 3)
        inner[name] = max(3, math.ceil(WINDOW_S * 1000.0 / window(fn, 5)))
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(window(fn, inner[name]))
    return times, inner


class TorchDetector:
    """``AutoCropDetector.update`` of the reference in eager torch, mode ``black`` or ``flat``."""

    def __init__(self, kind):
        self.kind, self.tb, self.lr = kind, None, None

    def update(self, frames):
        black = self.kind == "black"
        for x in frames:
            for dim in (-1, -2):
                y = R.rgb_to_y(x, tv_range=black)             # the reference converts once per detect_* call
                if black:
                    mean = y.mean(dim=dim, keepdim=True)
                    mask = (mean <= R.DARK) & ((y - mean).abs().amax(dim=dim, keepdim=True) < R.DEV)
                else:
                    median = y.median(dim=dim, keepdim=True).values
                    mask = ((y - median).abs() < R.DEV).float().mean(dim=dim, keepdim=True) > R.FRAC
                if dim == -1:
                    self.tb = mask.int() if self.tb is None else self.tb + mask.int()
                else:
                    self.lr = mask.int() if self.lr is None else self.lr + mask.int()


def error_lines():
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "autocrop.npz")))
    lines = ["worst e_hip / (2.2 * e_ref + 2^-23) against float64 over the inputs of tests/autocrop_cases.py (bound: 1)"]
    for kind in C.KINDS:
        worst = {k: (0.0, 0.0, 0.0) for k in C.STAT_KEYS}
        for name, x in C.all_inputs(kind).items():
            got = {k: v.cpu() for k, v in E.debug_stats(x.cuda(), black_only=kind == "black").items()}
            ratios = C.error_ratios(got, R.stats(x, kind), {k: golden[f"{name}/{kind}/{k}"] for k in C.STAT_KEYS})
            for k, v in ratios.items():
                worst[k] = max(worst[k], v)
        for k, label in zip(C.STAT_KEYS, C.STAT_NAMES[kind]):
            lines.append(f"  {kind:<5} {label:<13} ratio {worst[k][0]:.3f}  (e_hip {worst[k][1]:.3e}, e_ref {worst[k][2]:.3e})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autocrop.txt"))
    args = ap.parse_args()
    with torch.inference_mode():
        prop = torch.cuda.get_device_properties(0)
        lines = [f"device: {prop.name} ({prop.gcnArchName}, {prop.multi_processor_count} CUs), --rounds {args.rounds}"] + error_lines()
        lines.append(f"AutoCropDetector.update of a batch of 2, ms per call: median (min .. max) of {args.rounds} rounds, engine and "
                     "torch alternating round by round, HIP events")
        for label, (H, W) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
            for kind in C.KINDS:
                frames = torch.stack([C.make_frame(kind, H, W, H // 8, H // 8, 0, 0, 40 + i) for i in range(2)]).cuda()
                eng, ref = E.AutoCropDetector(mode=kind), TorchDetector(kind)
                eng.update(frames)
                ref.update(frames)
                assert torch.equal(eng.border_count_tb.flatten(), ref.tb.flatten()), (label, kind)
                assert torch.equal(eng.border_count_lr.flatten(), ref.lr.flatten()), (label, kind)
                t, inner = alternate([("engine", lambda: eng.update(frames)), ("torch", lambda: ref.update(frames))], args.rounds)
                med = {k: statistics.median(v) for k, v in t.items()}
                lines.append(f"{label} ({H} x {W}), mode {kind}")
                for k, v in t.items():
                    lines.append(f"  {k:<7} {med[k]:9.4f} ({min(v):.4f} .. {max(v):.4f}), {inner[k]} calls per window")
                lines.append(f"  torch / engine {med['torch'] / med['engine']:.2f} x")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
