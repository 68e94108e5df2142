"""Times stlizer's pass 3 ``grad_opt`` on the HIP engine against eager torch-ROCm on the same GPU and writes
profiles/stlizer_pass3.txt, followed by the converged-parity ratios that tests/test_gpu_stlizer_pass3.py asserts, computed here
with the same function (tests/stlizer_pass3_ref.py ``converged_ratios``) from the same fixture.

  grad_opt with pass 3's arguments (iteration 100, penalty weight 2e-3 / 2 s, resolution 320) at N = 1 800, 18 000 and 216 000
  frames (one minute, ten minutes and two hours at 30 fps), synthetic jitter paths of tests/stlizer_pass3_ref.py.

The torch side restates the reference's algorithm as what stlizer runs without the engine: the autograd closure of
stlizer/multipass_pipeline.py:311-325 under ``torch.optim.LBFGS(history_size=10, max_iter=4)`` for 100 steps.

    python tools/time_pass3.py [--rounds 7 --out FILE]

Wall time around synchronised calls (the torch loop synchronises at every ``if`` of LBFGS anyway), the two variants alternating
round by round in one process; reports the median and the spread (min .. max) over the rounds, and the engine's launch count."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stlizer_pass3_ref as R  # noqa: E402
from nunif_amd.stlizer import pass3 as P  # noqa: E402


def torch_grad_opt(tx, ty, ta, scene_weight, resolution, iteration=100, penalty_weight=1e-3):
    """The reference's grad_opt as an eager autograd + LBFGS loop."""
    rw = resolution / 320
    pad = lambda v: torch.cat([v, v[-1:].expand(3)])                         # noqa: E731
    tx, ty, ta = pad(tx) * rw, pad(ty) * rw, pad(ta)
    sw = F.pad(scene_weight, (0, 3))
    with torch.inference_mode(False), torch.enable_grad():
        px, py, pa = (t.clone().requires_grad_(True) for t in (tx, ty, ta))
        opt = torch.optim.LBFGS([px, py, pa], history_size=10, max_iter=4)

        def f():
            opt.zero_grad()
            loss = 0.0
            for x, t in zip((px, py, pa), (tx, ty, ta)):
                fx1 = x[1:] - x[:-1]
                fx2 = fx1[1:] - fx1[:-1]
                fx3 = fx2[1:] - fx2[:-1]
                grad_loss = (fx1.pow(2).mul(sw[:fx1.shape[0]]).mean() + fx2.pow(2).mul(sw[:fx2.shape[0]]).mean() +
                             fx3.pow(2).mul(sw[:fx3.shape[0]]).mean())
                loss = loss + grad_loss * (1.0 / 9.0) + (x - t).pow(2).mean() * penalty_weight
            loss.backward()
            return loss

        for _ in range(iteration):
            opt.step(f)
    return (px[:-3].detach() - tx[:-3]) / rw, (py[:-3].detach() - ty[:-3]) / rw, pa[:-3].detach() - ta[:-3]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stlizer_pass3.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"ms per call: median (min .. max) of {args.rounds} rounds, engine and torch alternating round by round, wall time",
             "grad_opt: iteration 100, penalty weight 1e-3, resolution 320 (pass 3's call); torch = the reference's algorithm as an "
             "eager autograd + torch.optim.LBFGS loop",
             f"engine launches per call: 1 + 100 * 4 * 22 + 1 = {2 + 100 * 4 * 22}, no host read"]
    for n in (1800, 18000, 216000):
        sx, sy, an = R.jitter_path(n, n)
        w = R.calc_scene_weight(R.match_scores(n, n, (n // 2,)))
        paths = torch.from_numpy(R.prepare(sx, sy, an, w)).to(dev)
        wd = torch.from_numpy(w).to(dev)
        variants = [("engine", lambda: P.grad_opt(paths[0], paths[1], paths[2], wd, 320, 100, 1e-3)),
                    ("torch", lambda: torch_grad_opt(paths[0], paths[1], paths[2], wd, 320, 100, 1e-3))]
        for _, fn in variants:
            timed(fn)
        times = {k: [] for k, _ in variants}
        for _ in range(args.rounds):
            for k, fn in variants:
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"N = {n}")
        for k, v in times.items():
            lines.append(f"  {k:<7} {med[k]:10.3f} ({min(v):.3f} .. {max(v):.3f})")
        lines.append(f"  torch / engine {med['torch'] / med['engine']:.2f} x")
    lines += ["", "converged parity, iteration 100: distance to the exact minimiser d and objective gap g of the engine over the worst",
              "of the nine recorded reference runs (the unperturbed one and its eight perturbations by k 2^-52); the tests' bound is 2"]
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "stlizer_pass3.npz")))
    for name in R.CONVERGED_CASES:
        paths, wd = (torch.from_numpy(golden[f"ref/{name}/{k}"]).to(dev) for k in ("paths", "weight"))
        out = P.grad_opt_traced(paths, wd, R.CASES[name][2], 100, R.penalty_weight(name))[0].cpu().numpy()
        d_hip, d_ref, g_hip, g_ref = R.converged_ratios(golden, name, out)
        lines.append(f"  {name:<6} d {d_hip:.3e} / {d_ref:.3e} = {d_hip / d_ref:.3f}   g {g_hip:.3e} / {g_ref:.3e} = {g_hip / g_ref:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
