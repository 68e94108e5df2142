"""Time one TransNetV2 window (100 frames of 3 x 27 x 48) on the HIP engine against the same network in eager fp32 torch on the
same GPU: the reference-shaped module restated in tests/transnetv2_ref.py (nn.functional conv3d / batch_norm / bmm / scatter_add,
the route `--scene-detect` took before the engine had this net).

    python tools/time_transnetv2.py [--frames 100 --batch 1 --rounds 20 --inner 5]

HIP events around `inner` back-to-back forwards, after warm-up, the two variants alternating round by round in one process;
reports the median and the spread per window, windows per second, and the engine's share of the 155 TFLOP/s fp32 matrix peak for
the FLOP count printed (multiply-adds of the convolutions and fc1 x 2; the tail's small products are not counted)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP32_MATRIX_PEAK = 155e12


def window_flops(frames):
    total, h, w = 0.0, 27, 48
    for cin, f in ((3, 16), (64, 32), (128, 64)):
        for c in (cin, 4 * f):
            total += 2.0 * frames * h * w * (9 * c * 8 * f + 6 * f * 4 * f)
        h, w = h // 2, w // 2
    return total + 2.0 * frames * 4864 * 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--skip-eager", action="store_true")
    a = ap.parse_args()
    import transnetv2_ref as R
    from nunif_amd.nunif.utils.transnetv2 import TransNetV2
    from nunif_amd.synthetic import transnetv2_state_dict
    dev = "cuda:0"
    sd = transnetv2_state_dict(7)
    model = TransNetV2()
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    eager_sd = R.prepare(sd, torch.float32, dev)
    x = R.make_clip(a.frames * a.batch, 11, "cuts").view(a.batch, a.frames, 3, 27, 48).to(dev)

    def engine():
        return model.predict(x)

    @torch.inference_mode()
    def eager():
        return torch.sigmoid(R.forward(eager_sd, x, None)[0])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner / a.batch            # ms per window

    variants = [("HIP engine", engine)] + ([] if a.skip_eager else [("eager torch fp32", eager)])
    for _ in range(3):
        for _, fn in variants:
            timed(fn)
    times = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            times[name].append(timed(fn))
    flops = window_flops(a.frames)
    print(f"TransNetV2, {a.batch} window(s) of {a.frames} frames per call, {a.rounds} rounds x {a.inner} calls, alternating; "
          f"{flops / 1e9:.1f} GFLOP per window")
    med = {}
    for name, _ in variants:
        t = times[name]
        med[name] = statistics.median(t)
        print(f"  {name:17s}: median {med[name]:8.3f} ms per window (min {min(t):.3f}, max {max(t):.3f}) = {1e3 / med[name]:7.1f} windows/s, "
              f"{flops / (med[name] * 1e-3) / 1e12:6.2f} TFLOP/s = {flops / (med[name] * 1e-3) / FP32_MATRIX_PEAK * 100:4.1f} % of the fp32 matrix peak")
    if len(variants) == 2:
        print(f"  engine against eager: {med['eager torch fp32'] / med['HIP engine']:.2f} x")
    if not a.skip_eager:
        d = (engine() - eager()).abs().max().item()
        print(f"  max |sigmoid difference| between the two on this input: {d:.3g}")


if __name__ == "__main__":
    main()
