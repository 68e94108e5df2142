"""Restatement of what iw3 wraps around the Depth-Anything-3 mono backbone, in torch on the CPU, in float64 and in fp32:
``_forward`` :33-56 of ``iw3/depth_anything_v3_model.py`` and ``extract_features`` :53-73 / ``forward`` :29-50 of
``iw3/models/da3mono_disparity.py`` (reference).  The fp32 form is the yardstick of the GPU tests (its error against the float64
form is ``e_ref``) and is compared with the recorded reference outputs in tests/test_da3_cpu.py; ``mut`` switches on one
kernel-shaped mistake at a time, which that comparison must catch.

Also the seeded inputs the fixture (tests/golden/make_golden_da3.py) and the GPU tests share.
"""
import math
from collections import OrderedDict

import torch

FEAT_DIM = 64
SKY_THRESH = 0.3
SHIFT = 0.2
SHAPES = ((1, 1, 3), (1, 1, 64), (1, 8, 8), (1, 37, 53), (2, 56, 98))      # (B, H, W) of the fixture
LARGE = (1, 518, 920)                                                      # GPU only: several histogram workgroups per image
KINDS = ("noise", "constant", "two_valued", "ramp_ties", "low_bits")
MUTATIONS = ("mask_ge", "no_clamp", "count9", "count11", "q_times_n", "lower_only", "no_max_clamp", "ranks_off", "shift_outside")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def depth_map(kind, B, H, W, seed=0):
    """[B,1,H,W] fp32, positive.  noise: uniform; constant; two_valued; ramp_ties: a ramp whose top quarter is one exact maximum;
    low_bits: values that differ only in the low 8 bits of their pattern (the last radix level alone separates them)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + KINDS.index(kind))
    n = H * W
    if kind == "noise":
        x = torch.rand(B, n, generator=g) * 4.0 + 0.05
    elif kind == "constant":
        x = torch.full((B, n), 1.25)
    elif kind == "two_valued":
        x = torch.where(torch.rand(B, n, generator=g) < 0.37, torch.tensor(0.5), torch.tensor(3.0))
    elif kind == "ramp_ties":
        ramp = torch.linspace(0.1, 2.0, n).clamp(max=float(torch.linspace(0.1, 2.0, n)[max(0, (3 * n) // 4 - 1)]))
        x = torch.stack([ramp[torch.randperm(n, generator=g)] for _ in range(B)])
    else:
        bits = torch.randint(0, 256, (B, n), generator=g, dtype=torch.int32) + 0x3FC00000      # 1.5 + k * 2^-23
        x = bits.view(torch.float32)
    return x.reshape(B, 1, H, W).contiguous()


def sky_map(B, H, W, seed=0, n_clear=None, on_threshold=0):
    """[B,1,H,W] fp32 in [0, 1].  Default: smooth noise on both sides of the threshold with a block exactly on it.  ``n_clear``:
    exactly that many pixels below the threshold, ``on_threshold`` more exactly on it (not sky: the mask is ``>``), the rest above."""
    g = torch.Generator().manual_seed(2000 * seed + 11 * H + W)
    n = H * W
    t = torch.tensor(SKY_THRESH, dtype=torch.float32)
    if n_clear is None:
        s = torch.rand(B, n, generator=g)
        s[:, : max(1, n // 7)] = t
        s = torch.stack([row[torch.randperm(n, generator=g)] for row in s])
    else:
        s = 0.35 + 0.6 * torch.rand(B, n, generator=g)
        s[:, :n_clear] = 0.25 * torch.rand(B, n_clear, generator=g)
        s[:, n_clear:n_clear + on_threshold] = t
        s = torch.stack([row[torch.randperm(n, generator=g)] for row in s])
    return s.reshape(B, 1, H, W).contiguous()


def host_ranks(n):
    """extract_features :65, the reference's expression itself."""
    return torch.linspace(1, n - 2, FEAT_DIM - 2, device="cpu").long()


def seeded_state_dict(seed):
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for key, cout, cin in (("mlp.0", 128, FEAT_DIM), ("mlp.2", 128, 128), ("mlp.4", 2, 128)):
        sd[key + ".weight"] = torch.randn(cout, cin, generator=g) * math.sqrt(1.0 / cin)
        sd[key + ".bias"] = torch.rand(cout, generator=g) * 0.2
    sd["mlp.4.weight"] *= 0.1               # both outputs clear of the ReLU: shift and sky_shift are at work
    sd["mlp.4.bias"] += 0.5
    return sd


# ---- _forward :33-56 ---------------------------------------------------------------------------------------------------------------------
def _quantile(v, dtype, mut):
    """torch.quantile(v, 0.99), linear: position 0.99 * (n - 1) between two order statistics.  fp32: torch's own function (it forms
    the position in fp32); float64 and the mutations: the definition, position in double."""
    if mut is None and dtype == torch.float32:
        return torch.quantile(v, 0.99)
    s = torch.sort(v.double())[0]
    n = s.numel()
    p = min(0.99 * n, n - 1.0) if mut == "q_times_n" else 0.99 * (n - 1)
    lo, hi = int(math.floor(p)), int(math.ceil(p))
    q = s[lo] if mut == "lower_only" else s[lo] + (s[hi] - s[lo]) * (p - lo)
    return q.to(dtype)


def forward_stage(depth, sky, raw_output=False, dtype=torch.float32, sky_thresh=SKY_THRESH, shift=SHIFT, mut=None, all_sky_zeros=False):
    """depth, sky [B,1,H,W] fp32 -> [B,1,H,W] of ``dtype``.  The sky mask is decided on the fp32 values in both precisions (it is a
    decision, not arithmetic).  ``all_sky_zeros``: the engine's answer where the reference raises (raw, no non-sky pixel)."""
    sky32 = sky.float()
    mask = sky32 >= sky_thresh if mut == "mask_ge" else sky32 > sky_thresh
    d, s = depth.to(dtype), sky.to(dtype)
    w = ((s if mut == "no_clamp" else s.clamp(sky_thresh, 1.0)) - sky_thresh) / (1.0 - sky_thresh)
    least = {"count9": 9, "count11": 11}.get(mut, 10)
    out = []
    for di, mi, wi in zip(d, mask, w):
        if not raw_output:
            if mi.numel() - mi.sum() < least:
                di = torch.zeros_like(di)
            else:
                di = 1.0 / (di + shift)
                di = di * (1 - wi)
        elif all_sky_zeros and bool(mi.all()):
            di = torch.zeros_like(di)
        else:
            q = _quantile(di[~mi], dtype, mut)
            di = di * (1 - wi) + wi * q
            if mut != "no_max_clamp":
                di = di.clamp(max=q)
        out.append(di)
    return torch.stack(out)


# ---- DA3MonoDisparity :29-73 -----------------------------------------------------------------------------------------------------------------
def extract_features(x, mut=None):
    """x [B,1,H,W] -> [B,64] of x's dtype: indexing a full sort."""
    flat = x.reshape(x.shape[0], -1)
    s = torch.sort(flat, dim=-1)[0]
    idx = host_ranks(flat.shape[-1])
    if mut == "ranks_off":
        idx = (idx + 1).clamp(max=flat.shape[-1] - 1)
    return torch.cat([s[:, :1], s[:, idx], s[:, -1:]], dim=-1)


def mlp(sd, feat, dtype):
    f = torch.nn.functional
    w = {k: v.to(dtype) for k, v in sd.items()}
    h = f.silu(f.linear(feat.to(dtype), w["mlp.0.weight"], w["mlp.0.bias"]))
    h = f.silu(f.linear(h, w["mlp.2.weight"], w["mlp.2.bias"]))
    return f.relu(f.linear(h, w["mlp.4.weight"], w["mlp.4.bias"]))


def model_forward(sd, depth, dtype=torch.float32, mut=None):
    """depth [B,1,H,W] fp32 -> disparity [B,1,H,W] of ``dtype`` (:29-50).  The sky mask (depth == max) is exact in any precision."""
    feat = extract_features(depth.float())
    x = mlp(sd, feat, dtype)
    d = depth.to(dtype)
    shift, sky_shift = x[:, 0].reshape(-1, 1, 1, 1), x[:, 1].reshape(-1, 1, 1, 1)
    mask = depth == depth.amax(dim=(1, 2, 3), keepdim=True)
    moved = d + sky_shift if mut == "shift_outside" else torch.where(mask, d + sky_shift, d)
    return 1.0 / (moved + shift)


# ---- the GPU tests' rule -------------------------------------------------------------------------------------------------------------------
def within_rule(got, ref32, ref64, factor=2.2):
    """e_hip <= factor * e_ref + 2^-23 * max|out| against float64; -> (ok, e_hip, bound)."""
    e_hip = float((got.double() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    bound = factor * e_ref + 2.0 ** -23 * float(ref64.abs().max())
    return e_hip <= bound, e_hip, bound
