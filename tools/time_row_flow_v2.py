#!/usr/bin/env python3
"""Time ``sbs.row_flow_v2`` on the HIP engine: ``infer_delta`` and both eyes of ``apply_divergence_nn_LR`` at B = 4, for a
392 x 686 depth map and at ``--stereo-width 1920`` (1080 x 1920), against (a) the eager fp16-autocast torch restatement of the
same net on the same GPU in the same run and (b) the engine's ``row_flow_v3`` at the same shapes.

Medians of 7 alternating rounds of HIP-event windows of 0.2 s or more, written as ``median (min .. max)``; for the v2 kernel also
the fraction of the fp16 MFMA peak (2 x 16560 FLOP per pixel) and of HBM (16 B per pixel: 12 read, 4 written) it reaches.

    python tools/time_row_flow_v2.py [--out profiles/row_flow_v2.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nunif_amd.iw3.backward_warp import apply_divergence_nn_LR  # noqa: E402
from nunif_amd.iw3.models.row_flow_v2 import RowFlowV2  # noqa: E402
from nunif_amd.iw3.models.row_flow_v3 import RowFlowV3  # noqa: E402
from nunif_amd.synthetic import row_flow_v2_state_dict, row_flow_v3_state_dict  # noqa: E402

PEAK_FP16_FLOPS, PEAK_HBM = 2.5e15, 8.0e12          # MI355X data sheet: dense fp16 matrix, HBM3E
MAC_PER_PX = 16 * 9 + 16 + 9 * (16 * 16 + 16 * 32 + 32 * 32) + 32 * 9
ROUNDS, WINDOW = 7, 0.2


def eager_v2(sd):
    """The net as torch runs it: pad 28, the padded convs, crop 28, under fp16 autocast."""
    p = {k: v.cuda() for k, v in sd.items()}

    def conv(x, key, pad):
        return F.conv2d(F.pad(x, pad, mode="replicate"), p[key + ".weight"], p[key + ".bias"])

    def run(x):
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            x = F.pad(x, (28,) * 4, mode="replicate")
            f = F.relu(conv(x, "feature.0", (1, 1, 0, 0)))
            no = conv(f, "non_overlap", (0, 0, 0, 0))
            a = F.relu(conv(f, "overlap_residual.0", (4, 4, 0, 0)))
            a = F.relu(conv(a, "overlap_residual.2", (4, 4, 0, 0)))
            a = F.relu(conv(a, "overlap_residual.4", (4, 4, 0, 0)))
            d = no + conv(a, "overlap_residual.6", (1, 1, 1, 1))
            return F.pad(d, (-28,) * 4).float()
    return run


def window(fn):
    """seconds per call over one HIP-event window of at least WINDOW seconds"""
    n = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b) * 1e-3
        if t >= WINDOW:
            return t / n
        n = max(n + 1, int(n * WINDOW / max(t, 1e-4) * 1.2))


def measure(fns):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):                          # alternating: every candidate once per round
        for k, fn in fns.items():
            times[k].append(window(fn))
    return times


def fmt(ts, scale=1e6, unit="us"):
    return f"{statistics.median(ts) * scale:9.1f} ({min(ts) * scale:.1f} .. {max(ts) * scale:.1f}) {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()
    dev = "cuda:0"
    sd2 = row_flow_v2_state_dict(301)
    m2 = RowFlowV2().eval()
    m2.load_state_dict(sd2)
    m3 = RowFlowV3().eval()
    m3.load_state_dict(row_flow_v3_state_dict(301))
    m2, m3 = m2.to(dev), m3.to(dev)
    m2.delta_output = m3.delta_output = True
    eager = eager_v2(sd2)
    g = torch.Generator().manual_seed(1)
    B = args.batch
    c = torch.rand((B, 3, 1080, 1920), generator=g).to(dev)
    lines = [f"row_flow_v2 on {torch.cuda.get_device_name(0)}: B = {B}, median (min .. max) of {ROUNDS} alternating rounds, "
             f"HIP-event windows >= {WINDOW} s"]
    for h, w in ((392, 686), (1080, 1920)):
        depth = torch.rand((B, 1, h, w), generator=g).to(dev)
        x = torch.cat([depth, torch.full_like(depth, 0.3), torch.full_like(depth, -0.15)], dim=1).contiguous()
        err = (m2.infer_delta(x) - eager(x)).abs().max().item()
        t = measure({
            "v2 engine infer_delta": lambda: m2.infer_delta(x),
            "v2 eager fp16 autocast": lambda: eager(x),
            "v3 engine infer_delta": lambda: m3.infer_delta(x),
            "v2 engine both eyes": lambda: apply_divergence_nn_LR(m2, c, depth, 2.0, 0.5, steps=1),
            "v3 engine both eyes": lambda: apply_divergence_nn_LR(m3, c, depth, 2.0, 0.5, steps=1),
        })
        px = B * h * w
        k = statistics.median(t["v2 engine infer_delta"])
        lines.append(f"depth {h} x {w} (image 1080 x 1920); max |engine - eager| = {err:.3e}")
        for name, ts in t.items():
            lines.append(f"  {name:24s} {fmt(ts)}")
        lines.append(f"  v2 kernel: {2 * MAC_PER_PX * px / k / 1e12:.1f} TFLOP/s = {2 * MAC_PER_PX * px / k / PEAK_FP16_FLOPS:.1%} of "
                     f"the fp16 MFMA peak, {16 * px / k / 1e9:.0f} GB/s = {16 * px / k / PEAK_HBM:.1%} of HBM; "
                     f"{statistics.median(t['v2 eager fp16 autocast']) / k:.1f}x eager, "
                     f"{statistics.median(t['v3 engine infer_delta']) / k:.2f}x row_flow_v3")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
