"""Time the convergence estimator (nunif_amd.iw3.convergence_estimator.ConvergenceEstimator, sod_v1.hip) on one batch of 4 frames,
1080p rgb with a 518-wide depth, seeded weights, EMA on.

    python tools/time_sod.py [--batch 4 --rounds 20 --inner 5]
    rocprofv3 --kernel-trace --stats -- python tools/time_sod.py --rounds 2   (kernel totals, a run of its own)
    python tools/time_sod.py --eager /path/to/nunif                           (adds the reference class with fuse(), eager torch
                                                                               under autocast on the same GPU, where a checkout exists)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, rounds, inner):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--eager", default=None)
    a = ap.parse_args()
    from nunif_amd.iw3.convergence_estimator import ConvergenceEstimator
    from nunif_amd.synthetic import sod_v1_state_dict
    sd = sod_v1_state_dict(20260125)
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand(a.batch, 3, 1080, 1920, generator=g).to(dev)
    depth = torch.rand(a.batch, 1, 294, 518, generator=g).to(dev)
    est = ConvergenceEstimator(0.5, device_id=0, enable_ema=True, state_dict=sd)
    for _ in range(3):
        est(rgb, depth)
    torch.cuda.synchronize()
    t = timed(lambda: est(rgb, depth), a.rounds, a.inner)
    print(f"convergence estimator, batch {a.batch}, rgb 1080 x 1920, depth 294 x 518, {a.rounds} rounds x {a.inner} calls")
    print(f"  HIP engine   : median {statistics.median(t):9.1f} us per batch  (min {min(t):.1f}, max {max(t):.1f})")
    if a.eager:
        sys.path.insert(0, a.eager)
        from iw3.models.sod_v1 import SODV1
        from iw3.convergence_estimator import ConvergenceEstimator as Ref
        m = SODV1()
        m.load_state_dict(sd)
        m = m.to(dev).eval().fuse()

        def run():
            with torch.inference_mode(), torch.autocast(device_type="cuda"):
                s, d = m.infer(rgb, depth)
                return Ref.depth_position_from_ratio(s, d, 0.5)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        t = timed(run, a.rounds, a.inner)
        print(f"  eager torch  : median {statistics.median(t):9.1f} us per batch  (min {min(t):.1f}, max {max(t):.1f})")


if __name__ == "__main__":
    main()
