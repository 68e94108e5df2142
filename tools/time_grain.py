"""Time the fused film-grain video step (grain.hip grain_video_step) on one output frame against the same step written with the
same step in eager torch on the same tensors: launch for launch what the reference's frame callback issues for --grain
(nunif/utils/rgb_noise.py rgb_noise_like + apply_rgb_noise, the noise-buffer blend of waifu2x/ui_utils.py:167-175,
nunif/utils/video.py from_tensor without its host copy) — 24 ATen launches, written here from the formulas.

    python tools/time_grain.py [--height 2160 --width 3840 --bits 8 --rounds 20 --inner 10]

HIP events around `inner` back-to-back launches, after warm-up, the two variants alternating round by round in one process;
reports the median and the spread per call, the bytes the fused step has to move and the share of achievable HBM bandwidth
(6.3 TB/s measured float4 copy on MI355X)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACHIEVABLE_HBM = 6.3e12


def baseline_noise(frame):
    """The distribution of level-2 rgb_noise_like in eager torch: 5 launches (two normal draws, a nearest resize, a scale and a
    scaled add), the number the reference's function issues."""
    c, h, w = frame.shape
    fine = torch.randn_like(frame)
    coarse = torch.randn(c, h // 2, w // 2, dtype=frame.dtype, device=frame.device)
    coarse_up = F.interpolate(coarse[None], size=(h, w), mode="nearest")[0]
    return fine.mul_(0.5).add_(coarse_up, alpha=0.5)


def baseline_apply(frame, grain, strength, gamma=2.2, decay=0.8):
    """apply_rgb_noise with light decay in eager torch: 11 pointwise launches (three pow, rsub, clamp, six mul / add), the number
    the reference's function issues; the formula is the one tests/grain_ref.py apply64 states."""
    lin = torch.pow(frame, gamma)
    shot = lin * grain
    fade = torch.rsub(lin, 1.0)
    fade.mul_(decay)
    fade.add_(1.0 - decay)
    fade.pow_(gamma)
    fade.mul_(strength)
    shot.mul_(fade)
    lin.add_(shot)
    lin.clamp_(0, 1)
    return lin.pow_(1.0 / gamma)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--bits", type=int, default=8, choices=[8, 16])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    from nunif_amd.nunif.utils import rgb_noise as R
    dev = "cuda:0"
    h, w, speed, strength = a.height, a.width, 0.8, 0.2
    maxv = 255.0 if a.bits == 8 else 65535.0
    x = torch.rand(3, h, w, device=dev)
    buf_f, buf_t = torch.randn(3, h, w, device=dev), torch.randn(3, h, w, device=dev)
    out = torch.empty((h, w, 3), dtype=torch.uint8 if a.bits == 8 else torch.int16, device=dev)
    counter = [0]

    def fused():
        R.grain_video_step(x, buf_f, out, bits=a.bits, seed=1, counter=counter[0], speed=speed, first=False, strength=strength)
        counter[0] += 1

    def chain():
        # the blend in 3 launches, then permute + contiguous, scale, round, cast: 4 more (24 in all with the two above)
        fresh = baseline_noise(x).mul_(speed)
        buf_t.mul_(1.0 - speed).add_(fresh)
        y = baseline_apply(x, buf_t, strength)
        hwc = y.permute(1, 2, 0).contiguous()
        return hwc.mul_(maxv).round_().to(torch.uint8 if a.bits == 8 else torch.uint16)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner * 1e3            # us per call

    for _ in range(3):
        timed(fused)
        timed(chain)
    t_f, t_c = [], []
    for _ in range(a.rounds):
        t_f.append(timed(fused))
        t_c.append(timed(chain))
    nbytes = h * w * (12 + 12 + 12 + 3 * a.bits // 8)
    mf, mc = statistics.median(t_f), statistics.median(t_c)
    print(f"film grain video step, output frame {h} x {w}, {a.bits} bit, {a.rounds} rounds x {a.inner} calls, alternating")
    print(f"  fused grain_video_step : median {mf:9.1f} us  (min {min(t_f):.1f}, max {max(t_f):.1f})")
    print(f"  eager torch, 24 launches: median {mc:9.1f} us  (min {min(t_c):.1f}, max {max(t_c):.1f})")
    print(f"  speed-up               : {mc / mf:.2f} x")
    print(f"  bytes the fused step moves: {nbytes / 1e6:.1f} MB (12 B frame read + 12 B + 12 B noise buffer + {3 * a.bits // 8} B store "
          f"per pixel) -> {nbytes / (mf * 1e-6) / 1e12:.2f} TB/s = {nbytes / (mf * 1e-6) / ACHIEVABLE_HBM * 100:.0f} % of the "
          f"achievable {ACHIEVABLE_HBM / 1e12:.1f} TB/s (floor {nbytes / ACHIEVABLE_HBM * 1e6:.0f} us)")


if __name__ == "__main__":
    main()
