"""Times stlizer's two per-frame steps on the HIP engine against eager torch-ROCm on the same GPU and writes
profiles/superpoint.txt:

  pass 1: SuperPoint (net, keypoints, descriptors) on a batch of 4 at 320 x 568 plus the matching of consecutive frames;
  pass 4: the stabilising warp of 4 frames at 1080p.

The torch side is the restatement tests/superpoint_f64.py under fp16 autocast (the net) with the reference's expressions for
matching (``d1 @ d2.t()``, argmax, gather) and for the warp (meshgrid + grid_sample): what stlizer runs without the engine.
Weights are seeded (nunif_amd.synthetic.superpoint_state_dict).

    python tools/time_superpoint.py [--rounds 7 --out FILE]

HIP events around ``inner`` back-to-back calls (pass 1: 80, warp: 2000, so that every window is 0.2 s or longer), after warm-up,
the two variants alternating round by round in one process; reports the median and the spread (min, max) over the rounds.  Pass 1
has one host read per batch on either side (the keypoint counts / ``torch.where``), which the events include."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import superpoint_f64 as R  # noqa: E402
from nunif_amd.nunif.utils import superpoint as E  # noqa: E402
from nunif_amd.synthetic import superpoint_state_dict  # noqa: E402


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


def torch_pass1(sd, x):
    with torch.autocast(device_type="cuda"):
        out = R.dense(sd, x, torch.float32)
    kps, _ = R.keypoints(out["scores"].float())
    frames = []
    for b, (xy, s) in enumerate(kps):
        g = ((xy + 0.5) / (xy.new_tensor([out["descriptors"].shape[3], out["descriptors"].shape[2]]) * 8)) * 2 - 1
        d = F.grid_sample(out["descriptors"][b:b + 1].float(), g.view(1, 1, -1, 2), mode="bilinear", align_corners=False)
        frames.append({"keypoints": xy, "descriptors": F.normalize(d.reshape(256, -1), p=2, dim=0).t()})
    for a, b in zip(frames[:-1], frames[1:]):
        sim = a["descriptors"] @ b["descriptors"].t()
        idx = torch.argmax(sim, dim=-1)
        best = torch.gather(sim, 1, idx.view(-1, 1)).view(-1)
        keep = best > 0.5
        _ = torch.arange(sim.shape[0], device=sim.device)[keep], idx[keep]


def engine_pass1(model, x):
    ret = model.infer(x)
    for a, b in zip(ret[:-1], ret[1:]):
        E.find_match_index(a, b, threshold=0.5, return_score_all=True)


def torch_warp(x, shift, scale, angle, center):
    B, _, H, W = x.shape
    center = center.reshape(B, 1, 1, -1)
    axis = torch.tensor([W - 1, H - 1], device=x.device, dtype=x.dtype).view(1, 1, 1, -1)
    shift, scale, angle = shift.neg().reshape(B, 1, 1, -1), scale.reciprocal().view(B, 1, 1, 1), angle.deg2rad().neg().reshape(B, 1, 1, 1)
    py, px = torch.meshgrid(torch.linspace(0, H - 1, H, device=x.device), torch.linspace(0, W - 1, W, device=x.device), indexing="ij")
    px = px.reshape(1, H, W, 1).expand(B, H, W, 1) - center[..., 0:1]
    py = py.reshape(1, H, W, 1).expand(B, H, W, 1) - center[..., 1:2]
    grid = torch.cat((px * angle.cos() - py * angle.sin(), px * angle.sin() + py * angle.cos()), dim=3) * scale + (shift + center)
    return F.grid_sample(x, grid / (axis * 0.5) - 1.0, mode="bilinear", padding_mode="border", align_corners=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superpoint.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    sd = superpoint_state_dict(R.WEIGHT_SEED)
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    model = E.SuperPoint(detection_threshold=R.THRESHOLD)
    model.load_state_dict(sd)
    model = model.eval().to("cuda")
    yy, xx = torch.arange(320.0).view(1, 1, 320, 1), torch.arange(568.0).view(1, 1, 1, 568)
    x = torch.clamp(0.5 + 0.25 * torch.sin(xx * 0.21) + 0.2 * torch.sin(yy * 0.13) + (torch.rand(4, 3, 320, 568) - 0.5) * 0.6, 0, 1).cuda()
    frames = torch.rand(4, 3, 1080, 1920).cuda()
    shift = torch.tensor([[3.5, -2.25]] * 4).cuda() * torch.arange(1, 5).view(4, 1).cuda()
    scale, angle = torch.ones(4).cuda(), torch.tensor([0.5, -0.75, 1.25, -0.3]).cuda()
    center = torch.tensor([[960.0, 540.0]] * 4).cuda()
    steps = [("pass 1 (4 x 320 x 568: net, keypoints, descriptors, 3 matchings)", 80,
              [("engine", lambda: engine_pass1(model, x)), ("torch", lambda: torch_pass1(sd_dev, x))]),
             ("pass 4 warp (4 x 3 x 1080 x 1920, border)", 2000,
              [("engine", lambda: E.apply_transform(frames, shift, scale, angle, center)),
               ("torch", lambda: torch_warp(frames, shift, scale, angle, center))])]
    with torch.inference_mode():
        counts = [len(r["keypoints"]) for r in model.infer(x)]
        lines = [f"device: {torch.cuda.get_device_name(0)}; keypoints per image: {counts}",
                 f"ms per call: median (min .. max) of {args.rounds} rounds, engine and torch alternating round by round, HIP events"]
        for name, inner, variants in steps:
            t = alternate(variants, inner, args.rounds)
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"{name}, {inner} calls per window")
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
