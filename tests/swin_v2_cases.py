"""Cases and references of the swin_unet_v2 tap-by-tap checks (helper module: ``test_gpu_swin_v2_errloc.py`` on the GPU,
``test_errloc_swin_v2.py`` on the CPU, ``tools/swin_v2_errloc.py`` for the record).

The net: the three registered nets at the smallest valid tile (T = 64: level 1 is 48 x 48 = 6 x 6 windows of 8 and 8 x 8 of 6, level 2
is 24 x 24, the IR blocks run at 32 x 32), the 2x net at batch 3 (heads = 3: 108 B, 192 B ... (window, head) units, so the last
workgroup of four waves is partly idle) and at T = 112, and a "loud-bias" 2x net whose ``qkv_proj.bias`` is redrawn at N(0, 0.5):
a token in the zero padding of a shifted window is a key / value equal to that bias, and at the synthetic N(0, 0.02) a kernel that
took it for zero could not be told from a correct one.

The attention alone (``nunif_hip_swin_unet_v2_debug_wattn``): the kernel's own base-2 expression

    s[i][j] = btab[i][j] + sum_d q[i][d] k[j][d],   att[i] = sum_j 2^(s[i][j] - max_j s[i][j]) v[j] / sum_j 2^(s[i][j] - max_j s[i][j])

on the same fp16 values, q / k / v of a padded token = bqkv, evaluated in float64 (the reference) and in fp32 torch rounded to fp16
(``e_ref``).  ``forward`` restates ``oracle.swin_unet_v2.model_forward`` with hooks for the mutations of the CPU file."""
import functools
import math

import torch
import torch.nn.functional as F

import errloc as E
from conftest import synth_image
from oracle import row_flow_v3 as RF
from oracle import swin_unet_v2 as OV

NAMES = {1: "waifu2x.swin_unet_v2_1x", 2: "waifu2x.swin_unet_v2_2x", 4: "waifu2x.swin_unet_v2_4x"}
SEED = {1: 41, 2: 42, 4: 44}
LOUD_SEED, LOUD_STD = 7, 0.5
# (scale, tile, batch, weights)
NET_CASES = [(1, 64, 1, "synthetic"), (2, 64, 1, "synthetic"), (4, 64, 1, "synthetic"), (2, 64, 3, "synthetic"),
             (2, 112, 1, "synthetic"), (2, 64, 1, "loud-bias")]
# the kernel alone: (ws, shift, H, W, C, B)
WATTN_CASES = [(8, False, 8, 8, 64, 1),        # one window, 2 units: two idle waves
               (8, True, 8, 8, 96, 1),         # four windows, each three quarters padding
               (8, True, 16, 24, 96, 3),       # H != W, 3 heads
               (8, True, 24, 24, 256, 1),      # 8 heads
               (6, False, 6, 6, 64, 1),        # one window of 6
               (6, True, 12, 18, 128, 2)]      # shifted windows of 6, H != W
K_FP32 = 2.2                                   # the project's constant for fp32 kernels (errloc.K_WARP)
LOG2E = 1.4426950408889634
QSCALE = LOG2E / math.sqrt(32.0)


def case_id(c):
    return "-".join(str(v) for v in c)


def state_dict(scale, weights="synthetic"):
    from nunif_amd import synthetic
    sd = synthetic.swin_unet_v2_state_dict(SEED[scale], scale)
    if weights == "loud-bias":
        g = torch.Generator().manual_seed(LOUD_SEED)
        for k in sorted(sd):
            if k.endswith("qkv_proj.bias"):
                sd[k] = torch.randn(sd[k].shape, generator=g) * LOUD_STD
    return sd


def make_input(tile, batch, seed=500):
    return torch.stack([synth_image(seed + i, 3, tile, tile) for i in range(batch)])


@functools.lru_cache(maxsize=None)
def references(case):
    """(x, y64, ye, taps64, taps_emulated) of one net case, computed once per process and left unchanged."""
    scale, tile, batch, weights = case
    E.set_threads()
    with torch.inference_mode():
        sd, x = state_dict(scale, weights), make_input(tile, batch)
        t64, te = {}, {}
        y64, ye = E.oracle64(sd, x, NAMES[scale], taps=t64), E.emulated(sd, x, NAMES[scale], taps=te)
    return x, y64, ye, t64, te


def tap_view(name, t):
    """The [B, C, H, W] view ``errloc`` takes: the taps are channels-last but ``residual``."""
    return t if name == "residual" else E.nhwc(t)


def tap_stats(name, tap, got, ref64, emu):
    """``localised_stats`` of one tap with the tap constants: its own cells and channel group, tau = TAP_TAU_REL x its rms."""
    cells, group = E.v2_tap_cells(name, tap)
    tau = E.TAP_TAU_REL * float(ref64.pow(2).mean().sqrt())
    return E.localised_stats(tap_view(tap, got.reshape(ref64.shape)), tap_view(tap, ref64), tap_view(tap, emu), cells, E.B_TAP, tau,
                             group=group)


# ---- the attention alone ------------------------------------------------------------------------------------------------------------
def wattn_inputs(case, seed=None):
    """(qkv fp16 [B,H,W,3C] with q pre-scaled, btab fp32 [N,N] log2e-scaled, bqkv fp32 [3C] with its q part pre-scaled): q, k, v
    ~ N(0, 1) so that the base-2 logits have a std of log2 e, the table and bqkv at O(1)."""
    ws, shift, H, W, C, B = case
    g = torch.Generator().manual_seed(1000 + ws * 100 + H * 7 + W + C if seed is None else seed)
    qkv = torch.randn((B, H, W, 3 * C), generator=g)
    qkv[..., :C] *= QSCALE
    btab = torch.randn((ws * ws, ws * ws), generator=g) * LOG2E
    bqkv = torch.randn((3 * C,), generator=g)
    bqkv[2 * C:] *= 2.0                                            # a padded value that is far from zero in every channel group
    bqkv[:C] *= QSCALE
    return qkv.half(), btab, bqkv


def _windows(t, ws):
    """[B, Hp, Wp, ...] -> [B, nwy, nwx, ws * ws, ...]"""
    B, Hp, Wp = t.shape[:3]
    rest = t.shape[3:]
    t = t.reshape(B, Hp // ws, ws, Wp // ws, ws, *rest)
    return t.permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).reshape(B, Hp // ws, Wp // ws, ws * ws, *rest)


def inside_mask(case):
    """[nwy, nwx, N] bool: the tokens of each window that lie inside the map."""
    ws, shift, H, W, C, B = case
    pad = ws // 2 if shift else 0
    m = F.pad(torch.ones(1, H, W, dtype=torch.bool), (pad, pad, pad, pad))
    return _windows(m, ws)[0]


def wattn_ref(case, qkv, btab, bqkv, dtype, mut=()):
    """The kernel's expression in ``dtype`` on the given values -> (att [B, nwy, nwx, heads, N, 32], softmax weights
    [B, nwy, nwx, heads, N, N]).  ``mut`` (the CPU file): "pad_zero" (padded q / k / v = 0), "pad_masked" (padded keys masked out),
    "transposed" (table [key][query]), "head_v" (head 0 reads head 1's values)."""
    ws, shift, H, W, C, B = case
    pad, heads, N = (ws // 2 if shift else 0), C // 32, ws * ws
    full = bqkv.to(dtype).expand(B, H + 2 * pad, W + 2 * pad, 3 * C).clone()
    if "pad_zero" in mut:
        full.zero_()
    full[:, pad:pad + H, pad:pad + W] = qkv.to(dtype)
    w = _windows(full, ws).reshape(B, (H + 2 * pad) // ws, (W + 2 * pad) // ws, N, 3, heads, 32)
    q, k, v = (w[..., i, :, :].permute(0, 1, 2, 4, 3, 5) for i in range(3))           # [B, nwy, nwx, heads, N, 32]
    if "head_v" in mut:
        v = torch.cat([v[:, :, :, 1:2], v[:, :, :, 1:]], dim=3)
    tab = btab.to(dtype)
    s = q @ k.transpose(-1, -2) + (tab.t() if "transposed" in mut else tab)
    if "pad_masked" in mut:
        s = s.masked_fill(~inside_mask(case)[None, :, :, None, None, :], float("-inf"))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    return (p @ v) / l, p / l


def wattn_to_windows(case, att):
    """The kernel's att map [B,H,W,C] in the layout of ``wattn_ref`` (padded tokens 0)."""
    ws, shift, H, W, C, B = case
    pad = ws // 2 if shift else 0
    full = F.pad(att, (0, 0, pad, pad, pad, pad))
    w = _windows(full, ws)
    return w.reshape(*w.shape[:4], C // 32, 32).permute(0, 1, 2, 4, 3, 5)


def half_ulp_fp16(m):
    """Half an fp16 ulp at magnitude ``m`` (a tensor): the one rounding of the kernel's output."""
    e = torch.floor(torch.log2(m.clamp_min(2.0 ** -14)))
    return torch.exp2(e - 11)


def wattn_stats(case, got, ref64, ref32h):
    """``got`` / ``ref32h`` (fp16 results in the window layout) against ``ref64``, over the tokens inside the map: the whole map and
    per (image, window, head).  Returns {"global": e_hip / bound, "worst": the worst region's e_hip / bound, "k": e_hip / e_ref
    over the map}; the bound is K_FP32 e_ref + half an fp16 ulp of the region's largest reference magnitude."""
    inside = inside_mask(case)[None, :, :, None, :, None]
    e_hip = ((got.double() - ref64).abs() * inside).amax((-1, -2))
    e_ref = ((ref32h.double() - ref64).abs() * inside).amax((-1, -2))
    mag = (ref64.abs() * inside).amax((-1, -2))
    region = e_hip / (K_FP32 * e_ref + half_ulp_fp16(mag))
    glob = e_hip.max() / (K_FP32 * e_ref.max() + half_ulp_fp16(mag.max()))
    return {"global": float(glob), "worst": float(region.max()), "k": float(e_hip.max() / e_ref.max().clamp_min(1e-30)),
            "finite": bool(torch.isfinite(got).all())}


@functools.lru_cache(maxsize=None)
def wattn_references(case):
    """(qkv, btab, bqkv, ref64, e_ref's fp16 result, softmax weights in float64)"""
    with torch.inference_mode():
        qkv, btab, bqkv = wattn_inputs(case)
        ref64, w64 = wattn_ref(case, qkv, btab, bqkv, torch.float64)
        ref32, _ = wattn_ref(case, qkv, btab, bqkv, torch.float32)
    return qkv, btab, bqkv, ref64, ref32.half(), w64


# ---- the forward restated, with the mutations of test_errloc_swin_v2.py ---------------------------------------------------------------
def _window_mha(sd, p, x, ws, bias, num_heads, shift, norm_weight, taps, name, mut):
    pad = ws // 2 if shift else 0
    if pad and "pad_short" in mut:                                 # windows start at -(ws / 2 - 1)
        lo, hi = pad - 1, pad + 1
    else:
        lo, hi = pad, pad
    if pad:
        x = F.pad(x, (lo, hi, lo, hi), mode="constant", value=0)
    B, C, H, W = x.shape
    oh, ow = H // ws, W // ws
    t = x.reshape(B, C, oh, ws, ow, ws).permute(0, 2, 4, 3, 5, 1).reshape(B * oh * ow, ws * ws, C)
    t = F.layer_norm(t, (C,), norm_weight, None, 1e-5)
    qkv = F.linear(t, sd[p + "mha.qkv_proj.weight"], sd[p + "mha.qkv_proj.bias"])
    hd, n = C // num_heads, ws * ws
    if pad:
        valid = F.pad(torch.ones(1, 1, H - lo - hi, W - lo - hi, dtype=torch.bool), (lo, hi, lo, hi))
        valid = valid.reshape(1, 1, oh, ws, ow, ws).permute(0, 2, 4, 3, 5, 1).reshape(oh * ow, n).repeat(B, 1)
        if "pad_zero" in mut:
            qkv = qkv * valid[..., None].to(qkv.dtype)
    q, k, v = qkv.split(C, dim=-1)

    def heads(z):
        return z.view(-1, n, num_heads, hd).permute(0, 2, 1, 3)
    if "transposed" in mut:
        bias = bias.transpose(-1, -2)
    s = (heads(q) @ heads(k).transpose(-1, -2)) * (1.0 / math.sqrt(hd)) + bias
    if pad and "pad_masked" in mut:
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    vh = heads(v)
    if "head_v" in mut:
        vh = torch.cat([vh[:, 1:2], vh[:, 1:]], dim=1)
    o = (torch.softmax(s, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(-1, n, C)
    if taps is not None:
        a = o.reshape(B, oh, ow, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
        taps[name + ".att"] = (a[:, lo:H - hi, lo:W - hi] if pad else a).contiguous()
    o = F.linear(o, sd[p + "mha.head_proj.weight"], sd[p + "mha.head_proj.bias"])
    o = o.reshape(B, oh, ow, ws, ws, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)
    return o[:, :, lo:H - hi, lo:W - hi] if pad else o


def _wac_block(sd, p, x, num_heads, ws, shift, conv_mlp, taps, muts):
    name = p[len("unet."):-1]
    mut = muts.get(name, ())
    bias = RF.window_score_bias(sd, p + "relative_bias.", (ws, ws))
    x = x + _window_mha(sd, p + "mha.", x, ws, bias, num_heads, shift, sd[p + "norm.weight"], taps, name, mut)
    z = F.conv2d(x, sd[p + "conv_mlp.w1.weight"], sd[p + "conv_mlp.w1.bias"])
    if conv_mlp:
        if "glu_swapped" in mut:
            z = torch.cat(tuple(reversed(z.chunk(2, dim=1))), dim=1)
        z = F.glu(z, dim=1)
        z = F.conv2d(F.pad(z, (1, 1, 1, 1), mode="replicate"), sd[p + "conv_mlp.w2.weight"], sd[p + "conv_mlp.w2.bias"])
        x = x + F.leaky_relu(z, 0.2)
    else:
        x = x + F.conv2d(F.leaky_relu(z, 0.1), sd[p + "conv_mlp.w2.weight"], sd[p + "conv_mlp.w2.bias"])
    if taps is not None:
        taps[name] = x.permute(0, 2, 3, 1).contiguous()
    return x


def forward(sd, x, scale, taps=None, muts=None):
    """``oracle.swin_unet_v2.model_forward`` (clamped) restated; bit-equal to it without a mutation.  ``muts``: {block name: (mutation,
    ...)} for the block mutations ("pad_zero", "pad_masked", "transposed", "head_v", "pad_short", "glu_swapped"), and under the key
    "net": "down1_stride" (the shortcut's mean over channels C2 apart instead of adjacent ones), "up1_order" (proj's channel taken as
    q C + c instead of 4 c + q), "crop_off" (the residual image cropped one pixel further up / left)."""
    muts = muts or {}
    net = muts.get("net", ())

    def tap(name, t, nchw=True):
        if taps is not None:
            taps[name] = (t.permute(0, 2, 3, 1) if nchw else t).contiguous()
    u = "unet."
    src = x
    x1 = F.leaky_relu(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), sd[u + "ir.path1.0.weight"], sd[u + "ir.path1.0.bias"]), 0.2)
    x2 = F.conv2d(F.pixel_unshuffle(x, 2), sd[u + "ir.path2.1.weight"], sd[u + "ir.path2.1.bias"])
    x2 = _wac_block(sd, u + "ir.path2.2.", x2, 2, 8, True, True, taps, muts)
    x2 = _wac_block(sd, u + "ir.path2.3.", x2, 2, 8, False, True, taps, muts)
    x = torch.cat([x1, F.pixel_shuffle(x2, 2)], dim=1)
    tap("ir", x)
    x = F.conv2d(x, sd[u + "patch.weight"], sd[u + "patch.bias"])
    x = F.leaky_relu(x[:, :, 7:-7, 7:-7], 0.2)
    tap("patch", x)
    C = x.shape[1]
    C2 = sd[u + "down1.conv.weight"].shape[0]
    heads, heads2 = max(C // 32, 2), max(C2 // 32, 2)
    n1, n3 = OV.n_blocks(sd, u + "wac1."), OV.n_blocks(sd, u + "wac3.")
    windows1 = [8, 6][:n1]
    for i, sh in enumerate(OV.shift_config(n1)):
        x = _wac_block(sd, f"{u}wac1.blocks.{i}.", x, heads, windows1[i], sh, True, taps, muts)
    skip = x
    sc = F.pixel_unshuffle(x, 2)
    B, C4, H, W = sc.shape
    if "down1_stride" in net:
        sc = sc.view(B, C4 // C2, C2, H, W).mean(dim=1)
    else:
        sc = sc.view(B, C2, C4 // C2, H, W).mean(dim=2)
    x = sc + F.leaky_relu(F.conv2d(x, sd[u + "down1.conv.weight"], sd[u + "down1.conv.bias"], stride=2), 0.2)
    tap("down1", x)
    for i, sh in enumerate(OV.shift_config(4)):
        x = _wac_block(sd, f"{u}wac2.blocks.{i}.", x, heads2, 8, sh, True, taps, muts)
    sc = F.pixel_shuffle(x.repeat_interleave(C * 4 // C2, dim=1), 2)
    pr = F.leaky_relu(F.conv2d(x, sd[u + "up1.proj.weight"], sd[u + "up1.proj.bias"]), 0.2)
    if "up1_order" in net:
        b_, _, h_, w_ = pr.shape
        pr = pr.view(b_, 4, C, h_, w_).transpose(1, 2).reshape(b_, 4 * C, h_, w_)
    x = sc + F.pixel_shuffle(pr, 2)
    x = x + skip
    tap("up1", x)
    for i, sh in enumerate(OV.shift_config(n3)):
        x = _wac_block(sd, f"{u}wac3.blocks.{i}.", x, heads, 8, sh, i < n3 - 1, taps, muts)
    x = F.conv2d(x, sd[u + "to_residual_image.proj.weight"], sd[u + "to_residual_image.proj.bias"])
    if scale > 1:
        x = F.pixel_shuffle(x, scale)
    d = 1 if "crop_off" in net else 0
    x = x[:, :, scale - d:x.shape[2] - scale - d, scale - d:x.shape[3] - scale - d]
    tap("residual", x, nchw=False)
    s = F.conv2d(F.pad(src, (1, 1, 1, 1), mode="replicate"), sd[u + "to_image.resampling.weight"])
    if scale > 1:
        s = F.pixel_shuffle(s, scale)
    unpad = (s.shape[2] - x.shape[2]) // 2
    if unpad:
        s = s[:, :, unpad:-unpad, unpad:-unpad]
    return torch.clamp(s + x * sd[u + "to_image.scale_bias"], 0.0, 1.0)


def forward64(sd, x, scale, taps=None, muts=None):
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return forward(sd64, x.double(), scale, taps, muts)
