"""Times stlizer's pass 2 on the HIP engine against eager torch-ROCm on the same GPU and writes profiles/find_transform.txt,
and measures the kernel on the cases of tests/golden/find_transform.npz and writes profiles/find_transform_errloc.txt (the error
table of tests/find_transform_ref.py with the kernel's rows, ``e_gpu``):

  find_transform on B = 128, N = 1024 and on B = 32, N = 3500, iteration = 50, sigma = 2.0, disable_scale (pass 2's own call);
  pass 2 of a 1024-pair video end to end (batch_size 4: 128 pairs per call), host reads included.

The torch side restates the reference's algorithm as what stlizer runs without the engine: an eager autograd loop of 50 Adam steps
with CosineAnnealingWarmRestarts (nunif/utils/superpoint.py:233-327), and pass 2's two host reads per pair
(stlizer/multipass_pipeline.py:246-269).  Points are the synthetic pairs of tests/find_transform_ref.py.

    python tools/time_find_transform.py [--rounds 7 --out FILE --errloc FILE]

HIP events around windows of back-to-back calls (0.2 s or longer each), after warm-up, the two variants alternating round by round in one process; reports
the median and the spread (min, max) over the rounds."""
import argparse
import os
import statistics
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import find_transform_ref as R  # noqa: E402
from nunif_amd.stlizer import find_transform as engine_find_transform, pack_points, pass2 as engine_pass2  # noqa: E402
from nunif_amd.stlizer.find_transform import find_transform_traced  # noqa: E402


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner                            # ms per call


def alternate(variants, rounds):
    for _, fn, n in variants:
        window(fn, max(1, n // 4))
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, fn, n in variants:
            times[name].append(window(fn, n))
    return times


def torch_find_transform(xy1, xy2, center, mask, iteration=50, lr=0.1, sigma=2.0, disable_scale=True):
    """The reference's batch algorithm as an eager autograd loop."""
    B = xy1.shape[0]
    with torch.enable_grad():
        translation = torch.zeros((B, 1, 2), device=xy1.device, requires_grad=True)
        scale = torch.ones((B, 1, 1), device=xy1.device, requires_grad=not disable_scale)
        rotation = torch.zeros((B, 1, 1), device=xy1.device, requires_grad=True)
        opt = torch.optim.Adam([{"params": [translation], "lr": lr}, {"params": [scale, rotation], "lr": lr}], betas=(0.5, 0.9))
        sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=iteration, eta_min=lr * 1e-3)
        a, b = xy1 - center, xy2 - center
        norm_scale = torch.nan_to_num(a).abs().amax(dim=[1, 2]).view(B, 1, 1)
        a, b = a / norm_scale, b / norm_scale
        for i in range(iteration):
            opt.zero_grad()
            rc, rs = rotation.cos(), rotation.sin()
            xy = torch.cat([a[:, :, :1] * rc - a[:, :, 1:] * rs, a[:, :, :1] * rs + a[:, :, 1:] * rc], dim=2) * scale + translation
            if i > 0:
                loss = F.l1_loss(xy, b, reduction="none")
                tmp = loss.detach().clone()
                tmp[torch.logical_not(mask)] = torch.nan
                mean = tmp.nanmean(dim=[1, 2], keepdim=True)
                std = (tmp - mean).pow(2).nanmean(dim=[1, 2], keepdim=True).sqrt()
                loss = loss[torch.logical_and(mask, ((tmp - mean) / std) < sigma)].mean()
            else:
                loss = F.l1_loss(xy[mask], b[mask])
            loss.backward()
            opt.step()
            sched.step()
    angle = rotation.detach().reshape(B, 1)
    return ((translation.detach() * norm_scale).reshape(B, 2), scale.detach().reshape(B, 1),
            torch.atan2(angle.sin(), angle.cos()).rad2deg(), center.reshape(B, 2))


def torch_pass2(points1, points2, center, resize_scale, args):
    device = args.state["device"]
    out = []
    p1, p2, masks = pack_points(points1, points2)
    for kp1, kp2, mask in zip(p1.split(args.batch_size * 32), p2.split(args.batch_size * 32), masks.split(args.batch_size * 32)):
        kp1, kp2, mask = kp1.to(device), kp2.to(device), mask.to(device)
        cb = torch.tensor(center, dtype=torch.float32, device=device).view(1, 2).expand(kp1.shape[0], 1, 2)
        shift, scale, angle, _ = torch_find_transform(kp1, kp2, cb, mask, iteration=args.iteration)
        for i in range(kp1.shape[0]):
            out.append((shift[i].tolist(), scale[i].item(), angle[i].item(), center, resize_scale))
    return out


def kernel_error_table(dev):
    """The kernel on every fixture case -> the text of profiles/find_transform_errloc.txt."""
    rows = {}
    for name in R.CASES:
        xy1, xy2, mask, center, kwargs = R.fixture_input(name)
        out = find_transform_traced(xy1.to(dev), xy2.to(dev), center.to(dev), None if mask is None else mask.to(dev), trace=True, **kwargs)
        rows[name] = tuple(out[k].cpu() for k in (0, 1, 2, 4))
    return R.error_table(extra={"e_gpu": rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_transform.txt"))
    ap.add_argument("--errloc", default=os.path.join(ROOT, "profiles", "find_transform_errloc.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"ms per call: median (min .. max) of {args.rounds} rounds, engine and torch alternating round by round, HIP events",
             "find_transform: iteration 50, sigma 2.0, disable_scale (pass 2's call); torch = the reference's algorithm as an eager autograd loop"]
    steps = []
    for B, N in ((128, 1024), (32, 3500)):
        counts = [int(v) for v in rng.integers(N // 2, N + 1, B)]
        counts[0] = N
        xy1, xy2, mask, center = [t.to(dev) for t in R.synthetic_pairs(B, counts, N)]
        steps.append((f"find_transform B = {B}, N = {N}", [
            ("engine", lambda a=xy1, b=xy2, c=center, m=mask: engine_find_transform(a, b, c, m, **R.PASS2), 500),
            ("torch", lambda a=xy1, b=xy2, c=center.view(-1, 1, 2), m=mask: torch_find_transform(a, b, c, m), 6)]))
    counts = [int(v) for v in rng.integers(300, 1025, 1024)]
    xy1, xy2, mask, _ = R.synthetic_pairs(7, counts, max(counts))
    p1 = [xy1[i, :n] for i, n in enumerate(counts)]
    p2 = [xy2[i, :n] for i, n in enumerate(counts)]
    pargs = types.SimpleNamespace(state={"device": dev}, batch_size=4, iteration=50)
    steps.append(("pass 2 of a 1024-pair video (300 .. 1024 points per pair, batch_size 4: 8 calls of 128 pairs; packing, uploads and host reads included)", [
        ("engine", lambda: engine_pass2(p1, p2, list(R.CENTER), 0.5, pargs), 12),
        ("torch", lambda: torch_pass2(p1, p2, list(R.CENTER), 0.5, pargs), 1)]))
    for name, variants in steps:
        t = alternate(variants, args.rounds)
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append(name + ", calls per window: " + ", ".join(f"{k} {n}" for k, _, n in variants))
        for k, v in t.items():
            lines.append(f"  {k:<7} {med[k]:9.3f} ({min(v):.3f} .. {max(v):.3f})")
        lines.append(f"  torch / engine {med['torch'] / med['engine']:.1f} x")
    text = "\n".join(lines) + "\n"
    print(text)
    table = kernel_error_table(dev)
    print(table)
    for path, body in ((args.out, text), (args.errloc, table)):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(body)


if __name__ == "__main__":
    main()
