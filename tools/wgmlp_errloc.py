"""Runs the cases of tests/test_gpu_wgmlp.py (the fused window-gMLP kernel alone and the whole ``waifu2x.wgmlp_4x`` net against float64,
with the fp16 emulation as yardstick) and writes the worst error ratios per class to profiles/wgmlp_errloc.txt.

    python tools/wgmlp_errloc.py [--out FILE]

A ratio is max |engine - float64| over max |emulation - float64|: over the whole map ("global", limit 2.5 for outputs and 3.5 for taps)
and per 8 x 8 window with the floor tau ("per region", limits 3.75 and 5.5)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_wgmlp as T  # noqa: E402
import wgmlp_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgmlp_errloc.txt"))
    a = ap.parse_args()
    worst = {}

    def note(key, stats, taps_as=None):
        for k, st in stats.items():
            name = f"{key}.{k if k == 'out' or taps_as is None else taps_as}"
            g, w = worst.get(name, (0.0, 0.0))
            worst[name] = (max(g, st["global"]), max(w, st["worst"]))

    benign, hot = T._model(), T._model("hot")
    for C in (128, 256):
        for B, H, W in T.GMLP_SHAPES[C]:
            for shift in (False, True):
                x = R.gmlp_input(100 + C + H, B, H, W, C)
                note(f"gmlp{C}", T.measure_gmlp(benign[0], benign[1], T.GMLP_BLOCK[C], x, shift, with_taps=H * W * B <= 4096))
        sd, m = T.gelu_tail_case(T.GMLP_BLOCK[C])
        note(f"gmlp{C}.tail", T.measure_gmlp(sd, m, T.GMLP_BLOCK[C], R.gmlp_input(7, 1, 16, 24, C), True, with_taps=True))
    for regime, (sd, m) in (("benign", benign), ("hot", hot)):
        for tile, batch in ((64, 1), (64, 3), (112, 1), (112, 3)):
            note(f"net.{regime}", T.measure_net(sd, m, tile, batch), taps_as="taps")
    lines = ["waifu2x.wgmlp_4x on the HIP engine: worst error ratios against the fp16 emulation (tools/wgmlp_errloc.py)",
             "key                          global   per region"]
    lines += [f"{k:28s} {g:6.2f}   {w:6.2f}" for k, (g, w) in sorted(worst.items())]
    text = "\n".join(lines) + "\n"
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
