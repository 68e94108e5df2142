"""SuperPoint, descriptor matching and the stabilising warp restated from the architecture (not from the engine and not from the
reference's module graph), parametrised by dtype: float64 is the oracle of tests/test_gpu_superpoint.py, float32 is tied to the
reference class by tests/test_superpoint_cpu.py on the fixture tests/golden/superpoint.npz.

The net: 4 blocks of two VGG units (3x3 conv, pad 1 -> ReLU -> BatchNorm eps 1e-3), a 2x2/2 max-pool (floor) after each of the
first three; channels 1 -> 64 -> 64 -> 128 -> 128.  Two heads on the stride-8 features, each a 3x3 VGG unit to 256 and a 1x1 conv
+ BatchNorm without ReLU: the detector to 65 logits (softmax, drop the last, 8x8 depth-to-space), the descriptor to 256 (L2 norm).
Cases, seeds and the test inputs are defined here and nowhere else."""
import math

import torch
import torch.nn.functional as F

WEIGHT_SEED = 20260
THRESHOLD = 0.01            # stlizer's SUPERPOINT_CONF detection_threshold
NMS_RADIUS = 4
REMOVE_BORDERS = 4
BN_EPS = 1e-3

# name -> (B, C, H, W, seed)
CASES = {
    "s40x48": (1, 3, 40, 48, 11),        # 5 x 6 cells: the whole map lies inside NMS and border halos
    "s44x61": (1, 1, 44, 61, 12),        # floors at every pool (61 -> 30 -> 15 -> 7), score map 40 x 56; gray input taken as it is
    "s64x88": (2, 3, 64, 88, 13),
    "s72x104": (2, 3, 72, 104, 14),
    "s120x160": (3, 3, 120, 160, 15),    # more workgroups than one wave of tiles, batch stride
}
DENSE_DESCRIPTOR_CASES = ("s40x48", "s44x61", "s64x88")                       # recorded in the fixture
TAP_CASES = {"s40x48": ("backbone.0", "backbone.1", "backbone.2", "backbone.3"), "s64x88": ("backbone.2", "backbone.3"),
             "s72x104": ("backbone.3",)}
TAPS = ("backbone.0", "backbone.1", "backbone.2", "backbone.3", "heads")

MATCH_CASES = {"m1x1": (1, 1, 31), "m7x300": (7, 300, 32), "m300x7": (300, 7, 33), "m257x513": (257, 513, 34)}

# warp: name -> (B, C, H, W, seed); parameter sets: (angle degrees, shift x, shift y, scale)
WARP_SHAPES = {"w21x33": (1, 1, 21, 33, 41), "w97x131": (3, 3, 97, 131, 42), "w40x64": (3, 1, 40, 64, 43)}
WARP_PARAMS = {"shift_int": (0.0, 3.0, -2.0, 1.0), "rot_p": (7.5, 2.25, -1.5, 1.0), "rot_n": (-7.5, -3.75, 0.5, 1.0),
               "scale": (0.0, 0.0, 0.0, 0.9), "rot90": (90.0, 0.0, 0.0, 1.0)}


def case_image(name):
    """Uniform noise over a sinusoidal ramp, clamped to [0, 1]."""
    B, C, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    phase = torch.rand(B, C, 1, 1, generator=g) * 6.28
    ramp = 0.5 + 0.25 * torch.sin(xx * 0.21 + phase) + 0.2 * torch.sin(yy * 0.13 + 2 * phase)
    return torch.clamp(ramp + (torch.rand(B, C, H, W, generator=g) - 0.5) * 0.6, 0, 1)


def unit(sd, p, x, relu, dtype):
    x = F.conv2d(x, sd[p + ".conv.weight"].to(dtype), sd[p + ".conv.bias"].to(dtype), padding=sd[p + ".conv.weight"].shape[-1] // 2)
    if relu:
        x = torch.relu(x)
    w, b, mean, var = (sd[f"{p}.bn.{k}"].to(dtype).view(1, -1, 1, 1) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - mean) / torch.sqrt(var + BN_EPS) * w + b


def dense(sd, image, dtype):
    """image [B, 1 or 3, H, W] -> {"backbone.0" .. "backbone.3", "heads" [B,512,h,w], "scores" [B,8h,8w], "descriptors" [B,256,h,w]}."""
    x = image.to(dtype)
    if x.shape[1] == 3:
        x = (x * torch.tensor([0.299, 0.587, 0.114], dtype=dtype, device=x.device).view(1, 3, 1, 1)).sum(1, keepdim=True)
    out = {}
    for b in range(4):
        x = unit(sd, f"backbone.{b}.0", x, True, dtype)
        x = unit(sd, f"backbone.{b}.1", x, True, dtype)
        if b < 3:
            x = F.max_pool2d(x, 2, 2)
        out[f"backbone.{b}"] = x
    hd, hs = unit(sd, "detector.0", x, True, dtype), unit(sd, "descriptor.0", x, True, dtype)
    out["heads"] = torch.cat([hd, hs], dim=1)
    logits = unit(sd, "detector.1", hd, False, dtype)
    prob = torch.softmax(logits, dim=1)[:, :64]
    B, _, h, w = prob.shape
    out["scores"] = prob.view(B, 8, 8, h, w).permute(0, 3, 1, 4, 2).reshape(B, h * 8, w * 8)
    d = unit(sd, "descriptor.1", hs, False, dtype)
    out["descriptors"] = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return out


def pool(x, r):
    return F.max_pool2d(x, 2 * r + 1, 1, r)


def nms(scores, r=NMS_RADIUS):
    """Greedy-free NMS: local maxima, then two rounds that admit maxima of what is left outside the suppressed discs."""
    zeros = torch.zeros_like(scores)
    keep = scores == pool(scores, r)
    for _ in range(2):
        supp = pool(keep.to(scores.dtype), r) > 0
        rest = torch.where(supp, zeros, scores)
        keep = keep | ((rest == pool(rest, r)) & ~supp)
    return torch.where(keep, scores, zeros)


def keypoints(scores, threshold=THRESHOLD, r=NMS_RADIUS, border=REMOVE_BORDERS):
    """scores [B,H,W] -> per image (xy [n,2] in row-major order, score [n]), and the suppressed map with its -1 band."""
    s = nms(scores, r).clone()
    if border:
        s[:, :border] = -1
        s[:, :, :border] = -1
        s[:, -border:] = -1
        s[:, :, -border:] = -1
    out = []
    for b in range(s.shape[0]):
        ys, xs = torch.where(s[b] > threshold)
        out.append((torch.stack([xs, ys], dim=-1).to(scores.dtype), s[b][ys, xs]))
    return out, s


def bilinear(x, ix, iy, border=False):
    """Four-tap bilinear at pixel coordinates (ix, iy) [B,N] of x [B,C,H,W] -> [B,C,N]; taps outside contribute nothing, taps
    inside are always multiplied and added (NaN * 0 = NaN)."""
    B, C, H, W = x.shape
    if border:
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    flat = x.reshape(B, C, H * W)
    out = torch.zeros(B, C, ix.shape[1], dtype=x.dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            wgt = ((x0 + 1 - ix) if dx == 0 else (ix - x0)) * ((y0 + 1 - iy) if dy == 0 else (iy - y0))
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
            val = torch.gather(flat, 2, idx[:, None, :].expand(B, C, -1))
            out = out + torch.where(ok[:, None, :], val * wgt[:, None, :], torch.zeros((), dtype=x.dtype))
    return out


def sample(kp, dense_desc, s=8):
    """kp [n,2] (x, y), dense_desc [256,h,w] -> [n,256]: bilinear at ((kp + 0.5) / s) - 0.5 cell units, L2 normalised."""
    dtype = dense_desc.dtype
    c, h, w = dense_desc.shape
    g = (kp.to(dtype) + 0.5) / (torch.tensor([w, h], dtype=dtype) * s) * 2 - 1
    ix, iy = ((g[:, 0] + 1) * w - 1) / 2, ((g[:, 1] + 1) * h - 1) / 2
    d = bilinear(dense_desc[None], ix[None], iy[None])[0].t()
    return d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)


def match_inputs(name):
    """Seeded unit descriptors; a few rows of d1 are noisy copies of rows of d2 so that matches above 0.5 exist."""
    n1, n2, seed = MATCH_CASES[name]
    g = torch.Generator().manual_seed(seed)
    d2 = F.normalize(torch.randn(n2, 256, generator=g), dim=1)
    d1 = torch.randn(n1, 256, generator=g)
    pick = torch.randint(0, n2, (n1,), generator=g)
    near = torch.rand(n1, generator=g) < 0.6
    d1 = torch.where(near[:, None], d2[pick] + 0.04 * d1, d1)
    return F.normalize(d1, dim=1), d2


def match(d1, d2, dtype):
    """-> (argmax, max, gap between the best and the second best similarity of every row)."""
    sim = d1.to(dtype) @ d2.to(dtype).t()
    top = torch.topk(sim, min(2, sim.shape[1]), dim=1)
    gap = top.values[:, 0] - top.values[:, 1] if sim.shape[1] > 1 else torch.full((sim.shape[0],), math.inf, dtype=dtype)
    return torch.argmax(sim, dim=1), sim.max(dim=1).values, gap


def warp_image(name):
    B, C, H, W, seed = WARP_SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, C, H // 6 + 2, W // 6 + 2, generator=g)
    up = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    return torch.clamp(0.8 * up + 0.2 * torch.rand(B, C, H, W, generator=g), 0, 1)


def warp_params(name, pname, dtype=torch.float32):
    """-> shift [B,2], scale [B], angle [B], center [B,2]; image b of a batch gets the set's values times (1 + b / 8)."""
    B, _, H, W, _ = WARP_SHAPES[name]
    ang, sx, sy, sc = WARP_PARAMS[pname]
    k = 1 + torch.arange(B, dtype=dtype) / 8
    shift = torch.stack([sx * k, sy * k], dim=1)
    if pname in ("shift_int", "rot90"):
        k = torch.ones(B, dtype=dtype)
        shift = torch.tensor([[sx, sy]], dtype=dtype).repeat(B, 1)
    scale = torch.full((B,), sc, dtype=dtype)
    angle = ang * k
    center = torch.tensor([[W // 2, H // 2]], dtype=dtype).repeat(B, 1)
    return shift, scale, angle, center


def warp_coords(shape, shift, scale, angle, center, dtype):
    """Sampling position (ix, iy) [B, H*W] in input pixels of every output pixel: rotate by -angle about the center, divide by
    scale, subtract the shift, through the normalisation to [-1, 1] over (size - 1) and back over size (align_corners=False)."""
    B, _, H, W = shape
    shift, scale, angle, center = (t.to(dtype) for t in (shift, scale, angle, center))
    py, px = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    px, py = px.reshape(1, -1) - center[:, 0:1], py.reshape(1, -1) - center[:, 1:2]
    a = -(angle * (math.pi / 180)).view(B, 1)
    gx, gy = px * torch.cos(a) - py * torch.sin(a), px * torch.sin(a) + py * torch.cos(a)
    inv = (1 / scale).view(B, 1)
    gx, gy = gx * inv + (center[:, 0:1] - shift[:, 0:1]), gy * inv + (center[:, 1:2] - shift[:, 1:2])
    gx, gy = gx / ((W - 1) * 0.5) - 1, gy / ((H - 1) * 0.5) - 1
    return ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2


def warp(x, shift, scale, angle, center, padding_mode, dtype):
    ix, iy = warp_coords(x.shape, shift, scale, angle, center, dtype)
    return bilinear(x.to(dtype), ix, iy, border=padding_mode == "border").reshape(x.shape)


def unsure_band(scores64, e_ref, threshold=THRESHOLD, r=NMS_RADIUS):
    """Pixels whose float64 score is within 8 e_ref of the threshold, or of the runner-up in their (2r+1)^2 window."""
    B, H, W = scores64.shape
    k = 2 * r + 1
    win = F.unfold(F.pad(scores64[:, None], (r, r, r, r), value=-math.inf), k).view(B, k * k, H, W).clone()
    win[:, (k * k) // 2] = -math.inf
    runner = win.max(dim=1).values
    return ((scores64 - threshold).abs() <= 8 * e_ref) | ((scores64 - runner).abs() <= 8 * e_ref)
