"""Times stlizer's outpaint step on the HIP engine against eager torch-ROCm on the same GPU and writes profiles/outpaint.txt:

  the network: ``LightOutpaintV1.infer(composite=False)`` on batches of 4 and 8 at 640 x 640 (the shape of the reference's own
  ``_bench``), with a per-kernel-class breakdown of the engine's time;
  the EMA buffer step of pass 4 on 4 frames at 1080p.

The torch side is the restatement tests/outpaint_f64.py under fp16 autocast (the net; the reference runs ``infer`` that way) and the
reference's expressions for the buffer loop (boolean-mask gather / scatter per frame, multipass_pipeline.py:461-471): what stlizer
runs without the engine.  Weights are seeded (nunif_amd.synthetic.light_outpaint_state_dict).

    python tools/time_outpaint.py [--rounds 7 --out FILE]

HIP events around ``inner`` back-to-back calls, after warm-up, the two variants alternating round by round in one process; reports
the median and the spread (min, max) over the rounds."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import outpaint_f64 as R  # noqa: E402
from nunif_amd import _hip  # noqa: E402
from nunif_amd.stlizer.models import LightOutpaintV1  # noqa: E402
from nunif_amd.stlizer.outpaint import buffer_step  # noqa: E402
from nunif_amd.synthetic import light_outpaint_state_dict  # noqa: E402


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner                            # ms per call


def alternate(variants, inner, rounds):
    for _ in range(2):
        for _, fn in variants:
            window(fn, max(1, inner // 10))
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(window(fn, inner))
    return times


def torch_infer(sd, x, mask):
    with torch.autocast(device_type="cuda"):
        return R.infer(sd, x, mask, 640, "raw", torch.float32)[0]


def torch_buffer(frames, coarse, buffer, d):
    z = frames.clone()
    masks = torch.isnan(z)
    z[masks] = 0
    for j in range(z.shape[0]):
        mask = masks[j]
        buffer.mul_(d)
        buffer.add_(coarse[j], alpha=1.0 - d)
        z[j][mask] = buffer[mask]
    return z.clamp_(0, 1)


def breakdown(model, x, mask, calls=20):
    _hip.profile_enable(True)
    _hip.profile_read(reset=True)
    for _ in range(calls):
        model.infer(x, mask, composite=False)
    torch.cuda.synchronize()
    recs = [r for r in _hip.profile_read(reset=True) if r["name"].startswith("outpaint_")]
    _hip.profile_enable(False)
    total = sum(r["total_ms"] for r in recs) or 1.0
    return [f"    {r['name']:<16} {r['total_ms'] / calls:7.3f} ms  {100 * r['total_ms'] / total:5.1f} %  ({r['launches'] // calls} launches)"
            for r in sorted(recs, key=lambda r: -r["total_ms"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outpaint.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    sd = light_outpaint_state_dict(R.WEIGHT_SEED)
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    model = LightOutpaintV1()
    model.load_state_dict(sd)
    model = model.eval().to("cuda")
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"ms per call: median (min .. max) of {args.rounds} rounds, engine and torch alternating round by round, HIP events"]
    with torch.inference_mode():
        for B in (4, 8):
            x = torch.rand(B, 3, 640, 640).cuda()
            mask = R.band_mask("three", 640, 640).repeat(B, 1, 1, 1).cuda()
            x = x * (~mask)
            t = alternate([("engine", lambda: model.infer(x, mask, composite=False)), ("torch", lambda: torch_infer(sd_dev, x, mask))],
                          100, args.rounds)
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"infer(composite=False), {B} x 3 x 640 x 640 ({B * 100} windows), 100 calls per window; torch = fp16 autocast, eager")
            for k, v in t.items():
                lines.append(f"  {k:<7} {med[k]:8.3f} ({min(v):.3f} .. {max(v):.3f})   {B / med[k] * 1000:8.0f} frames / s")
            lines.append(f"  torch / engine {med['torch'] / med['engine']:.2f} x")
            lines.append("  engine time by kernel class (event-timed one by one, so the sum exceeds the back-to-back figure):")
            lines.extend(breakdown(model, x, mask))
        frames = torch.rand(4, 3, 1080, 1920)
        frames[:, :, :40] = float("nan")
        frames[:, :, :, -60:] = float("nan")
        frames, coarse = frames.cuda(), torch.rand(4, 3, 1080, 1920).cuda()
        be, bt = torch.zeros(3, 1080, 1920).cuda(), torch.zeros(3, 1080, 1920).cuda()
        reset = torch.zeros(4, dtype=torch.uint8).cuda()

        def engine_buffer():
            buffer_step(frames)
            buffer_step(frames, coarse, be, reset, 0.25)

        t = alternate([("engine", engine_buffer), ("torch", lambda: torch_buffer(frames, coarse, bt, 0.25))], 200, args.rounds)
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append("pass 4 buffer step (4 x 3 x 1080 x 1920; engine = the launch before the net + the launch after it), 200 calls per window")
        for k, v in t.items():
            lines.append(f"  {k:<7} {med[k]:8.3f} ({min(v):.3f} .. {max(v):.3f})")
        lines.append(f"  torch / engine {med['torch'] / med['engine']:.2f} x")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
