"""Times ``waifu2x.wgmlp_4x`` on the HIP engine and writes profiles/wgmlp.txt:

  the forward at 4 x 3 x 256 x 256 (the reference's own ``_bench`` shape, wgmlp.py:473-494) and at 16 x 3 x 256 x 256 against the
  eager torch restatement (tests/wgmlp_ref.py, fp32 weights under fp16 autocast) on the same GPU in the same process, and, for
  context only, the engine's ``swin_unet_v2_4x`` and ``swin_unet_4x`` at the same shapes;
  the engine's per-kernel-class times of one forward (the engine's profiler, HIP events around every launch of the forward: the
  launches are serialised by it, so the shares are of the SUM of the classes, not of the forward above);
  the fused window-gMLP launch at C = 128 and C = 256: microseconds, TFLOP/s against the dense fp16 MFMA peak of the part
  (2.5 PFLOP/s) and the bytes it must move, 2 * tokens * C * 2, as a rate.

    python tools/time_wgmlp.py [--rounds 7 --out FILE]

HIP events around ``inner`` back-to-back calls after warm-up, the variants alternating round by round in one process; median
(min .. max) over the rounds.  Weights are seeded (nunif_amd.synthetic.wgmlp_state_dict): no released checkpoint exists."""
import argparse
import os
import statistics
import sys

os.environ.setdefault("NUNIF_PROF_TAGS", "1")

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wgmlp_ref as R  # noqa: E402
from nunif_amd import _hip, synthetic  # noqa: E402
from nunif_amd.nunif.models import create_model  # noqa: E402
import nunif_amd.waifu2x.utils  # noqa: E402,F401

PEAK_TFLOPS = 2500.0


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner                            # ms per call


def compare(fns, inner, rounds):
    for fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(ts, fns):
            t.append(window(fn, inner))
    return ts


def line(name, t):
    return f"  {name:22s} {statistics.median(t):9.3f} ({min(t):.3f} .. {max(t):.3f})"


def klass(name):
    if "wgmlp_block" in name:
        return "gMLP (fused window-gMLP kernel)"
    if "wg_stem" in name:
        return "stem (IR / Overscan convs)"
    if "to_image" in name or "source_residual" in name:
        return "head (ToImage GEMM, source residual)"
    if "shortcut" in name:
        return "PatchDown / PatchUp GEMMs and shortcuts"
    if "down1" in name or "up1" in name:
        return "PatchDown / PatchUp GEMMs and shortcuts"
    return "conv-MLP (w1 GEMMs, GLU, 3x3 convs; the patch conv is in here)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgmlp.txt"))
    a = ap.parse_args()
    dev = "cuda:0"
    out = [f"device: {torch.cuda.get_device_name(0)}",
           f"ms per call: median (min .. max) of {a.rounds} rounds, the variants alternating round by round, HIP events",
           "torch = tests/wgmlp_ref.py with fp32 weights under fp16 autocast, eager; seeded weights"]
    with torch.inference_mode():
        sd = synthetic.wgmlp_state_dict(21)
        model = create_model("waifu2x.wgmlp_4x").eval()
        model.load_state_dict(sd)
        model = model.to(dev)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        v2 = create_model("waifu2x.swin_unet_v2_4x").eval()
        v2.load_state_dict(synthetic.swin_unet_v2_state_dict(5, 4))
        v2 = v2.to(dev)
        sw = create_model("waifu2x.swin_unet_4x").eval()
        sw.load_state_dict(synthetic.swin_unet_state_dict(5, 4))
        sw = sw.to(dev)
        for B, inner in ((4, 5), (16, 2)):
            x = torch.rand((B, 3, 256, 256), device=dev)

            def torch_fn():
                with torch.autocast("cuda", dtype=torch.float16):
                    return R.forward(sdd, x)
            te, tt, tv, ts = compare([lambda: model(x), torch_fn, lambda: v2(x), lambda: sw(x)], inner, a.rounds)
            sep = "ranges do not overlap" if max(te) < min(tt) else "RANGES OVERLAP"
            out += [f"forward, {B} x 3 x 256 x 256 -> {B} x 3 x 952 x 952, {inner} calls per window",
                    line("engine wgmlp_4x", te), line("torch wgmlp_4x", tt),
                    f"  torch / engine {statistics.median(tt) / statistics.median(te):.2f} x ({sep})",
                    line("engine swin_unet_v2_4x", tv) + "   (context)", line("engine swin_unet_4x", ts) + "   (context)"]
            _hip.profile_enable(True)
            model(x)
            torch.cuda.synchronize()
            recs = _hip.profile_read(True)
            _hip.profile_enable(False)
            total = sum(r["total_ms"] for r in recs)
            groups = {}
            for r in recs:
                groups[klass(r["name"])] = groups.get(klass(r["name"]), 0.0) + r["total_ms"]
            out.append(f"  per kernel class, one profiled forward (sum of the classes {total:.3f} ms, every launch of the forward):")
            out += [f"    {k:60s} {v:8.3f} ms  {100 * v / total:5.1f} %" for k, v in sorted(groups.items(), key=lambda kv: -kv[1])]
            for r in sorted(recs, key=lambda r: -r["total_ms"]):
                tf = r["flops"] / (r["total_ms"] * 1e9) if r["total_ms"] > 0 else 0.0
                out.append(f"      {r['name']:40s} {r['launches']:3d} launches {r['total_ms']:8.3f} ms {tf:8.1f} TFLOP/s")
                if "wgmlp_block" in r["name"]:
                    us = 1e3 * r["total_ms"] / r["launches"]
                    out.append(f"        per launch {us:8.1f} us, {100 * tf / PEAK_TFLOPS:4.1f} % of the fp16 MFMA peak, "
                               f"{r['bytes'] / r['launches'] / (us * 1e-6) / 1e12:5.2f} TB/s of the algorithmic 2 * tokens * C * 2 bytes")
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
