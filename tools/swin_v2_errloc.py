"""Runs the cases of tests/test_gpu_swin_v2_errloc.py (every debug tap of the swin_unet_v2 nets against float64 with the fp16
emulation as yardstick, and the window attention kernel alone against its own expression in float64) and writes the worst error
ratios to profiles/swin_v2_errloc.txt.

    python tools/swin_v2_errloc.py [--out FILE]

Taps: ratio = max |engine - float64| over max |emulation - float64|, over the whole map ("global", limit 3.5; the output 2.5) and per
window of the block and head / 16 channels with the floor tau ("per region", limit 5.5; the output 3.75).  The attention alone:
e_hip over 2.2 e_ref + half an fp16 ulp, over the whole map and per (window, head) (limit 1), and e_hip / e_ref."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import swin_v2_cases as S  # noqa: E402
import test_gpu_swin_v2_errloc as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_v2_errloc.txt"))
    a = ap.parse_args()
    worst, where = {}, {}
    for case in S.NET_CASES:
        for k, st in T.measure_net(case).items():
            g, w = worst.get(k, (0.0, 0.0))
            if st["worst"] > w:
                where[k] = S.case_id(case)
            worst[k] = (max(g, st["global"]), max(w, st["worst"]))
    lines = ["waifu2x.swin_unet_v2_1x / 2x / 4x on the HIP engine: worst error ratios per debug tap against the fp16 emulation, over",
             "the cases " + ", ".join(S.case_id(c) for c in S.NET_CASES) + " (tools/swin_v2_errloc.py)",
             "tap                    global   per region   case of the worst region"]
    lines += [f"{k:22s} {g:6.2f}   {w:6.2f}       {where.get(k, '')}" for k, (g, w) in worst.items()]
    taps = [v for k, v in worst.items() if k != "out"]
    att = [v for k, v in worst.items() if k.endswith(".att")]
    lines += [f"{'all taps':22s} {max(g for g, _ in taps):6.2f}   {max(w for _, w in taps):6.2f}       (limits 3.50 / 5.50)",
              f"{'att taps':22s} {max(g for g, _ in att):6.2f}   {max(w for _, w in att):6.2f}",
              f"{'out':22s} {worst['out'][0]:6.2f}   {worst['out'][1]:6.2f}       (limits 2.50 / 3.75)", "",
              "v2_wattn_kernel alone (ws-shift-H-W-C-B; shifted windows of 6 and H != W are exercised here): fraction of the bound",
              "2.2 e_ref + half an fp16 ulp (limit 1)",
              "case                    whole map   per (window, head)   e_hip / e_ref"]
    for case in S.WATTN_CASES:
        st = T.measure_wattn(case)
        lines.append(f"{S.case_id(case):22s} {st['global']:9.3f}   {st['worst']:9.3f}            {st['k']:6.2f}")
    text = "\n".join(lines) + "\n"
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
