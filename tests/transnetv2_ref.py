"""TransNetV2 restated in plain torch for the tests: a function of (state dict, frames) that runs in any floating dtype, so that
float64 can serve as the yardstick (the reference class asserts fp32 / fp16 inputs).  Eval mode; the geometry of
``TransNetV2()``.  Also the synthetic clips the TransNetV2 tests share, and the detector windowing driven by any predictor.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

DILATIONS = (1, 2, 4, 8)
LOOKUP = 101


def _band(x):
    """[B,T,D] unit rows -> [B,T,101]: <x[t], x[t + j - 50]>, zero where t + j - 50 leaves the window."""
    B, T, _ = x.shape
    gram = torch.bmm(x, x.transpose(1, 2))
    half = (LOOKUP - 1) // 2
    gram = F.pad(gram, (half, half))
    rows = torch.arange(T, device=x.device).view(T, 1)
    return gram[:, rows, rows + torch.arange(LOOKUP, device=x.device).view(1, LOOKUP)]


def color_histograms(frames):
    """[B,T,3,27,48] of any float dtype -> L2-normalised 512-bin histograms [B,T,512] (float64): int(v) >> 5 per channel."""
    B, T = frames.shape[:2]
    v = frames.to(torch.int32) >> 5
    bins = ((v[:, :, 0] << 6) + (v[:, :, 1] << 3) + v[:, :, 2]).reshape(B * T, -1).long()
    hist = torch.zeros(B * T, 512, dtype=torch.float64, device=frames.device)
    hist.scatter_add_(1, bins, torch.ones(bins.shape, dtype=torch.float64, device=frames.device))
    return F.normalize(hist, p=2, dim=1).view(B, T, 512)


def ddcnn(sd, prefix, x, relu):
    outs = []
    for d in DILATIONS:
        y = F.conv3d(x, sd[f"{prefix}Conv3D_{d}.layers.0.weight"], padding=(0, 1, 1))
        outs.append(F.conv3d(y, sd[f"{prefix}Conv3D_{d}.layers.1.weight"], padding=(d, 0, 0), dilation=(d, 1, 1)))
    x = torch.cat(outs, dim=1)
    x = F.batch_norm(x, sd[prefix + "bn.running_mean"], sd[prefix + "bn.running_var"], sd[prefix + "bn.weight"],
                     sd[prefix + "bn.bias"], training=False, eps=1e-3)
    return F.relu(x) if relu else x


def prepare(sd, dtype, device="cpu"):
    return {k: v.to(device=device, dtype=dtype) for k, v in sd.items() if torch.is_floating_point(v)}


def forward(sd, frames, dtype=torch.float64):
    """sd: reference-layout state dict; frames [T,3,27,48] or [B,T,3,27,48].  Returns (one_hot [B,T], many_hot [B,T]) in dtype.
    dtype=None: sd is already the output of prepare() (frames' device and the dtype to run in)."""
    if frames.ndim == 4:
        frames = frames.unsqueeze(0)
    if dtype is None:
        dtype = sd["fc1.weight"].dtype
    else:
        sd = prepare(sd, dtype, frames.device)
    x = frames.to(dtype).permute(0, 2, 1, 3, 4)                     # [B,3,T,H,W]
    means = []
    for b in range(3):
        first = ddcnn(sd, f"SDDCNN.{b}.DDCNN.0.", x, True)
        x = F.relu(ddcnn(sd, f"SDDCNN.{b}.DDCNN.1.", first, False)) + first
        x = F.avg_pool3d(x, (1, 2, 2))
        means.append(x.mean(dim=(3, 4)))
    B, _, T = x.shape[:3]
    feat = x.permute(0, 2, 3, 4, 1).reshape(B, T, -1)
    sim = torch.cat(means, dim=1).transpose(1, 2)
    sim = F.normalize(F.linear(sim, sd["frame_sim_layer.projection.weight"], sd["frame_sim_layer.projection.bias"]), p=2, dim=2)
    sim = F.relu(F.linear(_band(sim), sd["frame_sim_layer.fc.weight"], sd["frame_sim_layer.fc.bias"]))
    col = _band(color_histograms(frames).to(dtype))
    col = F.relu(F.linear(col, sd["color_hist_layer.fc.weight"], sd["color_hist_layer.fc.bias"]))
    h = F.relu(F.linear(torch.cat([col, sim, feat], dim=2), sd["fc1.weight"], sd["fc1.bias"]))
    one = F.linear(h, sd["cls_layer1.weight"], sd["cls_layer1.bias"])[..., 0]
    many = F.linear(h, sd["cls_layer2.weight"], sd["cls_layer2.bias"])[..., 0]
    return one, many


# ---- synthetic clips ----------------------------------------------------------------------------------------------------------

def _scene(rng, n):
    """n frames [n,3,27,48] in [0,1] of one shot: a coloured low-frequency pattern that drifts slowly."""
    yy, xx = np.meshgrid(np.linspace(0, 1, 27), np.linspace(0, 1, 48), indexing="ij")
    base = rng.uniform(0.15, 0.85, size=3)
    amp = rng.uniform(0.05, 0.3, size=3)
    fx, fy = rng.uniform(0.5, 4.0, size=3), rng.uniform(0.5, 4.0, size=3)
    ph, speed = rng.uniform(0, 2 * math.pi, size=3), rng.uniform(-0.08, 0.08, size=3)
    out = np.empty((n, 3, 27, 48), np.float32)
    for t in range(n):
        for c in range(3):
            out[t, c] = base[c] + amp[c] * np.sin(2 * math.pi * (fx[c] * xx + fy[c] * yy) + ph[c] + speed[c] * t)
    return np.clip(out, 0.0, 1.0)


def make_clip(n, seed, kind="cuts"):
    """A clip of n frames, float32 in [0,1].  kind: "cuts" hard cuts every 17-40 frames; "dissolve" a 12-frame cross fade in the
    middle; "static" one frame repeated over the second half; "flash" a single white frame inside a shot."""
    rng = np.random.RandomState(seed)
    if kind == "cuts":
        parts, left = [], n
        while left > 0:
            m = min(left, int(rng.randint(17, 41)))
            parts.append(_scene(rng, m))
            left -= m
        x = np.concatenate(parts)
    elif kind == "dissolve":
        a, b = _scene(rng, n), _scene(rng, n)
        w = np.clip((np.arange(n) - (n // 2 - 6)) / 12.0, 0, 1).astype(np.float32).reshape(n, 1, 1, 1)
        x = a * (1 - w) + b * w
    elif kind == "static":
        x = _scene(rng, n)
        x[n // 2:] = x[n // 2]
    elif kind == "flash":
        x = _scene(rng, n)
        x[n // 2] = 1.0
    else:
        raise ValueError(kind)
    return torch.from_numpy(np.ascontiguousarray(x))


# fixture (a): name -> (frames per window, windows in the batch, value scale, clip kind, seed)
FIXTURE_CASES = {
    "t100_cuts": (100, 1, 1.0, "cuts", 11),
    "t100_dissolve": (100, 1, 1.0, "dissolve", 12),
    "t100_static": (100, 1, 1.0, "static", 13),
    "t100_flash": (100, 1, 1.0, "flash", 14),
    "t100_b2": (100, 2, 1.0, "cuts", 15),
    "t37": (37, 1, 1.0, "cuts", 16),
    "t1": (1, 1, 1.0, "cuts", 17),
    "t100_u8": (100, 1, 255.0, "cuts", 18),
}
WEIGHT_SEED = 7
# fixture (b): frame counts that hit every edge of the windowing
DETECT_LENGTHS = (1, 24, 25, 26, 49, 50, 51, 75, 99, 100, 101, 237)
DETECT_SEED = 21


def case_frames(name):
    T, B, scale, kind, seed = FIXTURE_CASES[name]
    x = make_clip(T * B, seed, kind).view(B, T, 3, 27, 48)
    return (x * scale).round() if scale != 1.0 else x


def detect_clip(n):
    return make_clip(n, DETECT_SEED, "cuts")


class RefPredictor:
    """The restatement as a detector model: ``predict(x)`` -> sigmoid(one_hot) [B,T] (float32, as the reference thresholds it)."""

    def __init__(self, sd, dtype=torch.float64):
        self.sd, self.dtype = sd, dtype

    def predict(self, x):
        one, _ = forward(self.sd, x.cpu(), self.dtype)
        return torch.sigmoid(one.float())
