"""Times the Any_V3_Mono launch groups against the eager torch restatement of the reference's expressions on the same GPU in the
same run: the disparity stage (raw and not raw), ``extract_features`` and the ``DA3MonoDisparity`` forward, at B = 4, 392 x 700 and
B = 8, 518 x 920 (the reference's ``_bench`` shape).  Median (min .. max) of 7 alternating rounds, device events.

    python tools/time_da3.py [--out profiles/da3_disparity.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import da3_ref as R  # noqa: E402

ROUNDS, INNER = 7, 20


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / INNER           # us per call


def compare(name, ours, eager, lines):
    for fn in (ours, eager):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"engine": [], "eager": []}
    for _ in range(ROUNDS):                              # alternating: both see the same neighbours on the machine
        t["engine"].append(timed(ours))
        t["eager"].append(timed(eager))
    fmt = lambda v: f"{statistics.median(v):9.1f} us ({min(v):.1f} .. {max(v):.1f})"      # noqa: E731
    ratio = statistics.median(t["eager"]) / statistics.median(t["engine"])
    lines.append(f"{name:34s} engine {fmt(t['engine'])}   eager torch {fmt(t['eager'])}   eager / engine {ratio:6.2f}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "da3_disparity.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run measures nothing"
    import nunif_amd.iw3.models  # noqa: F401
    from nunif_amd.iw3.depth_anything_v3_model import disparity_stage
    from nunif_amd.iw3.models import DA3MonoDisparity
    dev = "cuda:0"
    sd = R.seeded_state_dict(20)
    net = DA3MonoDisparity()
    net.load_state_dict(sd)
    net = net.eval().to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    lines = [f"tools/time_da3.py on {torch.cuda.get_device_name(0)}: median (min .. max) of {ROUNDS} alternating rounds of {INNER} calls,",
             "device events; eager torch = tests/da3_ref.py (the reference's expressions) on the same GPU, same run.  The eager stage",
             "synchronises with the host once per image (the all-sky test), as the reference does."]
    with torch.inference_mode():
        for B, H, W in ((4, 392, 700), (8, 518, 920)):
            depth, sky = R.depth_map("noise", B, H, W, 1).to(dev), R.sky_map(B, H, W, 1).to(dev)
            tag = f"B={B} {H}x{W}"
            for raw in (False, True):
                compare(f"{tag} stage raw={int(raw)}", lambda: disparity_stage(depth, sky, raw_output=raw),
                        lambda: R.forward_stage(depth, sky, raw_output=raw), lines)
            compare(f"{tag} extract_features", lambda: DA3MonoDisparity.extract_features(depth), lambda: R.extract_features(depth), lines)
            compare(f"{tag} model forward", lambda: net(depth), lambda: R.model_forward(sd_dev, depth), lines)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
