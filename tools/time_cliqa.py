"""Times cliqa's three nets and the patch selection on the HIP engine against eager torch-ROCm on the same GPU and writes
profiles/cliqa.txt:

  one forward of 8 and of 512 patches of 128 x 128, per net (8 = one image of ``python -m cliqa.filter_*``);
  patch selection (8 of the 8 x 15 patches) on a 1080p image.

The torch side is the restatement tests/cliqa_f64.py in fp32 under fp16 autocast, eager (what the reference runs without the
engine), and the torch expression of ``extract_patches`` (slice, stack, ``std``, ``topk``, gather).  Weights are seeded
(nunif_amd.synthetic.cliqa_state_dict).  An end-to-end CLI run is bound by the host's image decoding and is not measured.

    python tools/time_cliqa.py [--rounds 7 --out FILE]

HIP events around ``inner`` back-to-back calls after warm-up, the two variants alternating round by round in one process; reports
the median and the spread (min, max) over the rounds, and the engine's TFLOP/s against 5.7 GFLOP per patch (2 x 2.85 GMAC)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cliqa_f64 as R  # noqa: E402
import nunif_amd.cliqa.models as M  # noqa: E402
from nunif_amd.cliqa import utils as U  # noqa: E402
from nunif_amd.synthetic import cliqa_state_dict  # noqa: E402

GFLOP_PER_PATCH = 5.7


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner                            # ms per call


def compare(engine, torch_fn, inner, rounds):
    for fn in (engine, torch_fn):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    te, tt = [], []
    for _ in range(rounds):
        te.append(window(engine, inner))
        tt.append(window(torch_fn, inner))
    return te, tt


def line(name, t):
    return f"  {name:8s} {statistics.median(t):9.3f} ({min(t):.3f} .. {max(t):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cliqa.txt"))
    a = ap.parse_args()
    dev = "cuda:0"
    out = [f"device: {torch.cuda.get_device_name(0)}",
           f"ms per call: median (min .. max) of {a.rounds} rounds, engine and torch alternating round by round, HIP events",
           "torch = tests/cliqa_f64.py in fp32 under fp16 autocast, eager; TFLOP/s against 5.7 GFLOP per 128 x 128 patch"]
    classes = {"jpeg_quality": M.JPEGQuality, "grain_noise_level": M.GrainNoiseLevel, "scale_factor": M.ScaleFactor}
    with torch.inference_mode():
        for kind, cls in classes.items():
            sd = cliqa_state_dict(R.SEED[kind], kind)
            model = cls()
            model.load_state_dict(sd)
            model = model.to(dev)
            sdd = {k: v.to(dev) for k, v in sd.items()}
            for n, inner in ((8, 200), (512, 10)):
                x = torch.rand((n, 3, 128, 128), device=dev)

                def torch_fn():
                    with torch.autocast("cuda", dtype=torch.float16):
                        return R.forward(sdd, x, kind)
                te, tt = compare(lambda: model(x), torch_fn, inner, a.rounds)
                me, mt = statistics.median(te), statistics.median(tt)
                out += [f"cliqa.{kind}, {n} x 3 x 128 x 128, {inner} calls per window",
                        line("engine", te) + f"   {n * GFLOP_PER_PATCH / me:8.1f} TFLOP/s   {n / 8 / me * 1e3:9.0f} images / s",
                        line("torch", tt) + f"   {n * GFLOP_PER_PATCH / mt:8.1f} TFLOP/s",
                        f"  torch / engine {mt / me:.2f} x"]
        img = torch.rand((3, 1080, 1920), device=dev)

        def torch_select():
            p = torch.stack([img[:, y:y + 128, x:x + 128] for y in range(0, 1080 - 127, 128) for x in range(0, 1920 - 127, 128)])
            _, idx = torch.topk(U.std_score(p), 8)
            return p[idx]
        te, tt = compare(lambda: U.select_patches(img, 8), torch_select, 200, a.rounds)
        out += ["patch selection, 3 x 1080 x 1920, 8 of 120 patches, 200 calls per window", line("engine", te), line("torch", tt),
                f"  torch / engine {statistics.median(tt) / statistics.median(te):.2f} x"]
    out.append("an end-to-end `python -m cliqa.filter_*` run is bound by the host's image decoding and was not measured")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
