"""Time the HDR -> SDR tone mapping (hdr.hip) against the same map run eagerly in torch on the same device, and record its accuracy.

    python tools/time_hdr2sdr.py [--rounds 7 --inner 10 --out profiles/hdr2sdr.txt]

Per size (1920 x 1080, 3840 x 2160) and curve (PQ, HLG), medians over alternating rounds, after warm-up, in one process:
  * the kernel alone, device frame in, ``u16`` and ``chw`` forms: HIP events around `inner` back-to-back launches;
  * the whole ``hdr2sdr(av_frame)`` call, host array in to host array out (stand-ins for the two PyAV objects: the array is handed
    over and taken back without PyAV's own copies, for both routes alike), host clock, the call ends in a synchronise;
  * the eager route: tests/hdr_ref.py's fp32 restatement of the reference's passes on the same device, upload and download
    included — what the reference's function does on this GPU.
Bytes moved, the share of the achievable HBM rate (6.3 TB/s measured float4 copy on MI355X) and the kernel's instruction counts are
reported with the times; the accuracy section is the worst ``e_hip / (2.2 * e_ref + 2^-23)`` per curve over the cases of
tests/test_gpu_hdr.py."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdr_ref as R  # noqa: E402

ACHIEVABLE_HBM = 6.3e12
DEV = "cuda:0"


def accuracy(hdr, lines):
    lines.append("accuracy, debug form against float64; yardstick: the fp32 restatement of the reference (worst over the whole map and "
                 "over each of the 16 bands of the brightest input code)")
    cases = [(n,) + c for n, c in R.CASES.items()]
    cases += [(f"noise270x480_{t}", "noise270", t, "bt709", {}) for t in (R.PQ, R.HLG)]
    worst = {R.PQ: (0.0, ""), R.HLG: (0.0, "")}
    for name, inp, trc, cs, params in cases:
        x16 = R.make_input("noise", 270, 480) if inp == "noise270" else R.make_input(inp)
        v64, _ = R.hdr2sdr_ref(x16, trc, cs, torch.float64, **params)
        v32, u32 = R.hdr2sdr_ref(x16, trc, cs, torch.float32, **params)
        xd = torch.from_numpy(x16.view(np.int16)).to(DEV)
        got = hdr.hdr2sdr_tensor(xd, trc, cs, form="debug", **params).cpu()
        u16 = hdr.hdr2sdr_tensor(xd, trc, cs, form="u16", **params).cpu().numpy().view(np.uint16)
        e_hip = (got.double() - v64).abs().amax(dim=2).numpy()
        e_ref = (v32.double() - v64).abs().amax(dim=2).numpy()
        band = R.brightest_band(x16)
        ratio = e_hip.max() / (2.2 * e_ref.max() + 2.0 ** -23)
        for b in range(16):
            m = band == b
            if m.any():
                ratio = max(ratio, e_hip[m].max() / (2.2 * e_ref[m].max() + 2.0 ** -23))
        lines.append(f"  {name:30s} e_hip {e_hip.max():.3g}  e_ref {e_ref.max():.3g}  worst e_hip / bound {ratio:.3f}  "
                     f"integers equal to the reference's fp32: {100.0 * (u16 == u32).mean():.2f} %")
        if ratio > worst[trc][0]:
            worst[trc] = (ratio, name)
    for trc, label in ((R.PQ, "PQ"), (R.HLG, "HLG")):
        lines.append(f"  worst ratio, {label}: {worst[trc][0]:.3f} ({worst[trc][1]})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdr2sdr.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_hdr2sdr needs a ROCm device")
    from nunif_amd.nunif.utils import hdr
    from nunif_amd.nunif.utils.video import hdr2sdr
    for name, mod in R.fake_av_modules().items():
        sys.modules[name] = mod

    class VideoFrame:                                   # takes the array as it is: no copy on either route
        @classmethod
        def from_ndarray(cls, array, format=None):
            f = cls()
            f.array = array
            return f
    sys.modules["av.video.frame"].VideoFrame = VideoFrame

    class Frame(R.FakeFrame):
        def to_ndarray(self, **kwargs):
            return self.rgb48

    lines = [f"HDR -> SDR tone mapping (hdr.hip), {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"medians of {a.rounds} alternating rounds; kernel windows: HIP events around {a.inner} launches; calls: host clock, "
             "each call ends in a synchronise", ""]
    for h, w in ((1080, 1920), (2160, 3840)):
        x16 = np.random.default_rng(1).integers(0, 65536, size=(h, w, 3)).astype(np.uint16)
        xd = torch.from_numpy(x16.view(np.int16)).to(DEV)
        frame = Frame(x16)
        for trc, label in ((R.PQ, "PQ"), (R.HLG, "HLG")):
            o16 = torch.empty((h, w, 3), dtype=torch.int16, device=DEV)
            ochw = torch.empty((3, h, w), dtype=torch.float32, device=DEV)

            def events(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / a.inner * 1e3

            def clock(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e6

            runs = {
                "kernel u16": lambda: events(lambda: hdr.hdr2sdr_tensor(xd, trc, "bt709", form="u16", out=o16)),
                "kernel chw": lambda: events(lambda: hdr.hdr2sdr_tensor(xd, trc, "bt709", form="chw", out=ochw)),
                "hdr2sdr(av_frame)": lambda: clock(lambda: hdr2sdr(frame, trc, "bt709", device=DEV)),
                "eager torch route": lambda: clock(lambda: R.hdr2sdr_ref(x16, trc, "bt709", torch.float32, DEV)),
            }
            for fn in runs.values():
                for _ in range(2):
                    fn()
            t = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    t[k].append(fn())
            med = {k: statistics.median(v) for k, v in t.items()}
            lines.append(f"{w} x {h}, {label}")
            for k in runs:
                lines.append(f"  {k:18s}: median {med[k]:10.1f} us  (min {min(t[k]):.1f}, max {max(t[k]):.1f})")
            for k, nb, what in (("kernel u16", h * w * 12, "6 B read + 6 B store"), ("kernel chw", h * w * 18, "6 B read + 12 B store")):
                lines.append(f"  {k}: {nb / 1e6:.1f} MB ({what} per pixel) -> {nb / med[k] / 1e6:.2f} TB/s = "
                             f"{nb / (med[k] * 1e-6) / ACHIEVABLE_HBM * 100:.0f} % of the achievable {ACHIEVABLE_HBM / 1e12:.1f} TB/s "
                             f"(floor {nb / ACHIEVABLE_HBM * 1e6:.0f} us)")
            e = med["eager torch route"]
            lines.append(f"  eager route over: kernel u16 {e / med['kernel u16']:.1f} x, kernel chw {e / med['kernel chw']:.1f} x, "
                         f"hdr2sdr(av_frame) {e / med['hdr2sdr(av_frame)']:.2f} x")
            lines.append("")
    accuracy(hdr, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
