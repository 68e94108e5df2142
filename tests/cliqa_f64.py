"""The three cliqa nets (cliqa/models/jpeg_quality.py, grain_noise_level.py, scale_factor.py of the reference) restated with conv,
batch_norm, ReLU and the pools written out unfolded, in the dtype of the state dict and the input (helper module, not a conftest).
It runs in float64 (the exact answer, pinned to the reference classes by tests/golden/cliqa.npz), in fp32, and in fp32 under
``oracle.fp16_autocast_emulation`` (the reference's own fp16-autocast arithmetic, cliqa/utils.py:65,78,91: the GPU tests' yardstick).

``mutate`` switches one detail to a plausible wrong one, for the tests that show the bounds can tell:
``zero_pad_first`` (zero instead of replicate padding in the first conv), ``replicate_later`` (replicate instead of zero padding
in the second conv), ``ceil_pool`` (ceil instead of floor pooling), ``max_subsampling`` (max instead of mean in the subsampling head).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle.fp16_emulation import fp16_autocast_emulation

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cliqa.npz")
# whole taps of the shapes small enough to store (float32, one file per net); the larger shapes keep digests only
GOLDEN_TAPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cliqa_taps_%s.npz")
WHOLE_TAP_SHAPES = ((1, 8, 8), (3, 16, 24), (2, 21, 30))
K_OUT = 2.1
KINDS = ("jpeg_quality", "grain_noise_level", "scale_factor")
HEADS = {"jpeg_quality": ("quality_output", "subsampling_output"), "grain_noise_level": ("noise_level_output",),
         "scale_factor": ("scale_factor_output",)}
SHAPES = ((1, 8, 8), (3, 16, 24), (2, 21, 30), (9, 40, 56), (2, 128, 128))
SEED = {"jpeg_quality": 11, "grain_noise_level": 12, "scale_factor": 13}
TAPS = ("pool1", "pool2", "pool3", "head_maps")
# (H, W, num_patches) of the patch selection cases
SELECT = ((128, 128, 8), (300, 390, 8), (256, 1024, 8), (640, 512, 3))
PATCH = 128
BN_EPS = 1e-5


def net_input(kind, shape):
    """Seeded [B,3,H,W] fp32 in [0, 1): a smooth field plus noise, so that neighbouring pixels correlate as in a photo."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * SEED[kind] + 7 * B + 3 * H + W)
    low = torch.rand((B, 3, max(2, H // 8), max(2, W // 8)), generator=g)
    low = low.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :H, :W]
    if low.shape[2] < H or low.shape[3] < W:
        low = F.pad(low, (0, W - low.shape[3], 0, H - low.shape[2]), mode="replicate")
    return (0.7 * low + 0.3 * torch.rand((B, 3, H, W), generator=g)).contiguous()


def select_image(case):
    """Seeded [3,H,W] fp32 image whose 128 x 128 blocks carry noise of distinct amplitudes (distinct std scores)."""
    H, W, _ = case
    g = torch.Generator().manual_seed(5000 + 3 * H + W)
    rows, cols = -(-H // PATCH), -(-W // PATCH)
    amp = (0.15 + 0.8 * torch.rand((rows * cols,), generator=g)[torch.randperm(rows * cols, generator=g)]).reshape(rows, cols)
    amp = amp.repeat_interleave(PATCH, 0).repeat_interleave(PATCH, 1)[:H, :W]
    return (0.5 + amp * (torch.rand((3, H, W), generator=g) - 0.5)).contiguous()


def std_scores64(image, patch=PATCH):
    """float64 ``std_score`` (cliqa/utils.py:26-27) of the row-major non-overlapping patches of ``image`` [3,H,W]."""
    _, H, W = image.shape
    p = [image[:, y:y + patch, x:x + patch] for y in range(0, H - patch + 1, patch) for x in range(0, W - patch + 1, patch)]
    p = torch.stack(p)
    return torch.std(p.double(), dim=[2, 3]).mean(dim=1), p


def preprocess(kind, x):
    if kind == "jpeg_quality":
        r, g, b = x[:, 0:1], x[:, 1:2], x[:, 2:3]
        y = r * 0.299 + g * 0.587 + b * 0.114
        cb = (b - y) * 0.564 + 0.5
        cr = (r - y) * 0.713 + 0.5
        x = torch.cat([y, cb, cr, r, g, b], dim=1)
    return x * 2. - 1.


def _conv_bn(sd, conv, bn, x, pad_mode):
    x = F.pad(x, (1, 1, 1, 1), mode=pad_mode) if pad_mode == "replicate" else F.pad(x, (1, 1, 1, 1))
    x = F.conv2d(x, sd[conv + ".weight"], sd.get(conv + ".bias"))
    return F.batch_norm(x, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, BN_EPS)


def forward(sd, x, kind, taps=None, mutate=None, clamp=True):
    """-> tuple of [B,1] outputs.  ``taps``: a dict that receives pool1 / pool2 / pool3 / head_maps."""
    ceil = mutate == "ceil_pool"
    pool = lambda t: F.max_pool2d(t, 2, ceil_mode=ceil)     # noqa: E731
    x = preprocess(kind, x)
    x = torch.relu(_conv_bn(sd, "features.0", "features.1", x, "constant" if mutate == "zero_pad_first" else "replicate"))
    x = torch.relu(_conv_bn(sd, "features.3", "features.4", x, "replicate" if mutate == "replicate_later" else "constant"))
    x = pool(x)
    if taps is not None:
        taps["pool1"] = x
    for i, blk in enumerate(("features.7", "features.9")):
        y = torch.relu(_conv_bn(sd, blk + ".conv.0", blk + ".conv.1", x, "constant"))
        y = _conv_bn(sd, blk + ".conv.3", blk + ".conv.4", y, "constant")
        x = pool(torch.relu(y + x))
        if taps is not None:
            taps[f"pool{i + 2}"] = x
    outs, maps = [], []
    for h in HEADS[kind]:
        m = torch.relu(_conv_bn(sd, h + ".0", h + ".1", x, "constant"))
        maps.append(m)
        if h == "subsampling_output" and mutate != "max_subsampling":
            v = m.mean(dim=(2, 3), keepdim=True)
        else:
            v = m.amax(dim=(2, 3), keepdim=True)
        y = F.conv2d(v, sd[h + ".4.weight"], sd[h + ".4.bias"]).reshape(x.shape[0], -1)
        outs.append(torch.clamp(y, 1.0, 2.0) if (kind == "scale_factor" and clamp) else y)
    if taps is not None:
        taps["head_maps"] = torch.cat(maps, dim=1)
    return tuple(outs)


def forward64(sd, x, kind, **kw):
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return forward(sd64, x.double(), kind, **kw)


def half_conv_weights(sd):
    """autocast casts conv weights and conv biases to fp16; BatchNorm's tensors stay fp32 (``oracle.half_weights`` would round them
    too: their keys carry no "norm")."""
    def is_conv(k):
        return sd[k].dim() == 4 or (k.endswith(".bias") and k[:-5] + ".weight" in sd and sd[k[:-5] + ".weight"].dim() == 4)
    return {k: (v.half().float() if v.is_floating_point() and is_conv(k) else v) for k, v in sd.items()}


def emulated(sd, x, kind, **kw):
    with fp16_autocast_emulation():
        return forward(half_conv_weights(sd), x.float(), kind, **kw)


def digest(t):
    """What the fixture keeps of a map too large to store: mean, mean |.|, max |.| and 64 strided samples, float64."""
    f = t.double().flatten()
    step = max(1, f.numel() // 64)
    return np.concatenate([[float(f.mean()), float(f.abs().mean()), float(f.abs().max())], f[::step][:64].numpy()])


def golden():
    return np.load(GOLDEN)


def fp16_ulp(v):
    """One fp16 ulp at magnitude v (normal range)."""
    return 2.0 ** (np.floor(np.log2(max(float(v), 2.0 ** -14))) - 10)


def out_bound(y64, yemu):
    """The GPU tests' output bound of one head: 2.1 x the emulation's error + one fp16 ulp at max |y64|."""
    return K_OUT * float((yemu.double() - y64).abs().max()) + fp16_ulp(float(y64.abs().max()))


_cache = {}


def references(kind, shape):
    """(sd, x, y64, yemu, taps64, tapsemu) of a case, computed once per process and shared; treat as read-only."""
    key = (kind, tuple(shape))
    if key not in _cache:
        from nunif_amd.synthetic import cliqa_state_dict
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
        sd, x = cliqa_state_dict(SEED[kind], kind), net_input(kind, shape)
        t64, temu = {}, {}
        with torch.inference_mode():
            y64 = forward64(sd, x, kind, taps=t64, clamp=False)
            yemu = emulated(sd, x, kind, taps=temu, clamp=False)
        _cache[key] = (sd, x, y64, yemu, t64, temu)
    return _cache[key]
