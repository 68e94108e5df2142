"""The SOD v1 saliency net and the convergence estimator restated as plain functions of (state dict, tensors) that run in any
floating dtype (the tests use float64 as the truth): ``iw3/models/sod_v1.py`` :30-56 over ``nunif/utils/u2netp.py`` :11-430 and
``iw3/convergence_estimator.py`` :33-84 of the reference.  BatchNorm is applied as BatchNorm (eval), not folded.  Also the inputs
the SOD tests share.  Test infrastructure only."""
import math

import torch
import torch.nn.functional as F

WEIGHT_SEED = 20260125
NET = 192
CONVERGENCE = 0.5
EMA_DECAY = 0.9
EMA_FRAMES = 8
EMA_RESETS = (2, 5)
EMPTY_OUT_BIAS = -60.0
# (name, rgb size, depth size, scene seed).  "flat": constant depth 0.4 (quantile range < 1e-6).
CASES = (("scene_a", (192, 192), (192, 192), 1), ("scene_b", (192, 192), (192, 192), 2), ("flat", (192, 192), (192, 192), 3))


def scene(seed, rgb_size, depth_size, flat=False, dtype=torch.float32):
    """A synthetic frame: smooth colour blobs over a gradient, and a depth with a near object; values in [0, 1]."""
    g = torch.Generator().manual_seed(1000 + seed)

    def field(size):
        h, w = size
        ys = torch.linspace(0, 1, h)[:, None]
        xs = torch.linspace(0, 1, w)[None, :]
        return ys, xs

    ys, xs = field(rgb_size)
    rgb = torch.zeros(3, *rgb_size)
    for c in range(3):
        a = torch.rand(6, generator=g)
        rgb[c] = 0.5 + 0.25 * torch.sin(6.0 * a[0] * xs + 5.0 * a[1] * ys + 6.28 * a[2]) + 0.2 * torch.cos(9.0 * a[3] * xs * ys + a[4])
        cx, cy, r = 0.2 + 0.6 * torch.rand(3, generator=g)
        rgb[c] += 0.4 * torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (0.02 + 0.05 * r))
    ys, xs = field(depth_size)
    a = torch.rand(5, generator=g)
    depth = 0.15 + 0.35 * ys + 0.1 * xs + 0.45 * torch.exp(-((xs - 0.3 - 0.4 * a[0]) ** 2 + (ys - 0.3 - 0.4 * a[1]) ** 2) / 0.03)
    if flat:
        depth = torch.full(depth_size, 0.4)
    return rgb.clamp(0, 1).to(dtype)[None], depth.clamp(0, 1).to(dtype)[None, None]


def case_inputs(name, dtype=torch.float32):
    for n, rs, ds, seed in CASES:
        if n == name:
            return scene(seed, rs, ds, flat=(n == "flat"), dtype=dtype)
    raise KeyError(name)


def ema_inputs(dtype=torch.float32):
    """8 frames (the three cases and variations of them), rgb [8,3,192,192], depth [8,1,192,192]."""
    rgbs, depths = [], []
    for i in range(EMA_FRAMES):
        r, d = scene(1 + i % 2 + 10 * (i // 2), (NET, NET), (NET, NET), dtype=dtype)
        rgbs.append(r)
        depths.append(d)
    return torch.cat(rgbs), torch.cat(depths)


def _cast(sd, dtype):
    return {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in sd.items()}


def rebnconv(sd, p, x, dirate):
    y = F.conv2d(x, sd[p + ".conv_s1.weight"], sd[p + ".conv_s1.bias"], padding=dirate, dilation=dirate)
    y = F.batch_norm(y, sd[p + ".bn_s1.running_mean"], sd[p + ".bn_s1.running_var"], sd[p + ".bn_s1.weight"], sd[p + ".bn_s1.bias"],
                     training=False, eps=1e-5)
    return F.relu(y)


def up_like(src, tar):
    return F.interpolate(src, size=tar.shape[2:], mode="bilinear", align_corners=False)


def pool(x):
    return F.max_pool2d(x, 2, stride=2, ceil_mode=True)


def rsu(sd, p, L, x):
    """RSU7..RSU4 (L = 7..4) :44-284."""
    hxin = rebnconv(sd, p + ".rebnconvin", x, 1)
    h = [None, rebnconv(sd, p + ".rebnconv1", hxin, 1)]
    for i in range(2, L):
        h.append(rebnconv(sd, f"{p}.rebnconv{i}", pool(h[i - 1]), 1))
    h.append(rebnconv(sd, f"{p}.rebnconv{L}", h[L - 1], 2))
    d = rebnconv(sd, f"{p}.rebnconv{L - 1}d", torch.cat((h[L], h[L - 1]), 1), 1)
    for i in range(L - 2, 0, -1):
        d = rebnconv(sd, f"{p}.rebnconv{i}d", torch.cat((up_like(d, h[i]), h[i]), 1), 1)
    return d + hxin


def rsu4f(sd, p, x):
    hxin = rebnconv(sd, p + ".rebnconvin", x, 1)
    h1 = rebnconv(sd, p + ".rebnconv1", hxin, 1)
    h2 = rebnconv(sd, p + ".rebnconv2", h1, 2)
    h3 = rebnconv(sd, p + ".rebnconv3", h2, 4)
    h4 = rebnconv(sd, p + ".rebnconv4", h3, 8)
    h3d = rebnconv(sd, p + ".rebnconv3d", torch.cat((h4, h3), 1), 4)
    h2d = rebnconv(sd, p + ".rebnconv2d", torch.cat((h3d, h2), 1), 2)
    h1d = rebnconv(sd, p + ".rebnconv1d", torch.cat((h2d, h1), 1), 1)
    return h1d + hxin


def u2netp(sd, x, taps=None):
    """U2NETP.forward :364-430, eval: sigmoid(d0).  ``taps``: dict that receives hx1 .. hx6 and hx1d."""
    q = "u2netp."
    hx1 = rsu(sd, q + "stage1", 7, x)
    hx2 = rsu(sd, q + "stage2", 6, pool(hx1))
    hx3 = rsu(sd, q + "stage3", 5, pool(hx2))
    hx4 = rsu(sd, q + "stage4", 4, pool(hx3))
    hx5 = rsu4f(sd, q + "stage5", pool(hx4))
    hx6 = rsu4f(sd, q + "stage6", pool(hx5))
    hx5d = rsu4f(sd, q + "stage5d", torch.cat((up_like(hx6, hx5), hx5), 1))
    hx4d = rsu(sd, q + "stage4d", 4, torch.cat((up_like(hx5d, hx4), hx4), 1))
    hx3d = rsu(sd, q + "stage3d", 5, torch.cat((up_like(hx4d, hx3), hx3), 1))
    hx2d = rsu(sd, q + "stage2d", 6, torch.cat((up_like(hx3d, hx2), hx2), 1))
    hx1d = rsu(sd, q + "stage1d", 7, torch.cat((up_like(hx2d, hx1), hx1), 1))
    if taps is not None:
        taps.update(hx1=hx1, hx2=hx2, hx3=hx3, hx4=hx4, hx5=hx5, hx6=hx6, hx1d=hx1d)
    ds = []
    for i, m in enumerate((hx1d, hx2d, hx3d, hx4d, hx5d, hx6), start=1):
        d = F.conv2d(m, sd[f"{q}side{i}.weight"], sd[f"{q}side{i}.bias"], padding=1)
        ds.append(d if i == 1 else up_like(d, ds[0]))
    d0 = F.conv2d(torch.cat(ds, 1), sd[q + "outconv.weight"], sd[q + "outconv.bias"])
    return torch.sigmoid(d0)


def entry(rgb, depth, size=NET):
    """SODV1.infer :50-54 + forward :40-41: (x6 [B,6,s,s], depth resized)."""
    s = (size, size)
    rgb = F.interpolate(rgb, s, mode="bilinear", antialias=False, align_corners=False)
    depth = F.interpolate(depth, s, mode="bilinear", antialias=False, align_corners=False)
    return torch.cat((rgb, depth, depth ** 0.5, depth ** 2), dim=1), depth


def infer(sd, rgb, depth, dtype=torch.float64, taps=None):
    sd = _cast(sd, dtype)
    x6, d = entry(rgb.to(dtype), depth.to(dtype))
    return u2netp(sd, x6, taps=taps), d


def depth_position(saliency, depth, pos):
    """depth_position_from_ratio :33-59 in the dtype of ``depth``; [B]."""
    out = []
    for i in range(depth.shape[0]):
        d = depth[i].flatten()[saliency[i].flatten() > 0.5]
        if d.numel() == 0:
            out.append(torch.tensor(0.5, dtype=depth.dtype))
            continue
        q01, q09 = d.quantile(0.1), d.quantile(0.9)
        r = q09 - q01
        out.append(q01 if r < 1e-6 else (q01 + q09) / 2 + (pos - 0.5) * (r * 3.0))
    return torch.stack(out).clamp(0, 1)


def ema(z, decay, reset_pts, state=None):
    """__call__ :69-82 over the values z [N]; returns (results [N], state after)."""
    out = []
    for i in range(z.shape[0]):
        state = z[i].clone() if state is None else decay * state + (1.0 - decay) * z[i]
        out.append(state.clone())
        if reset_pts[i]:
            state = None
    return torch.stack(out), state


def max_err_per_image(a, b):
    return (a.double() - b.double()).abs().flatten(1).max(dim=1).values
