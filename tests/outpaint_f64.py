"""LightOutpaintV1, its ``infer`` wrapper and the EMA frame buffer of stlizer's pass 4 restated from the architecture (not from the
engine and not from the reference's module graph), parametrised by dtype: float64 is the oracle of tests/test_gpu_outpaint.py,
float32 is tied to the reference class by tests/test_outpaint_cpu.py on the fixture tests/golden/outpaint.npz.

The net (stlizer/models/light_outpaint_v1.py): cat(x, mask) -> three 3x3 stride-2 convs over a replicate pad (4 -> 8 -> 16 -> 64,
LeakyReLU 0.2) -> enc = MHABlock(64, 2 heads) + PoolBlock(64) -> x + proj_out(mid(proj_mid(x))), mid = (MHABlock(32, 1 head) +
PoolBlock(32)) twice -> dec = MHABlock(64) + PoolBlock(64) -> 1x1 conv to 3 -> bilinear x8.  MHABlock: 8 x 8 windows, softmax(q k^T
/ sqrt(32) + one 64 x 64 bias table) v, head projection, residual, then a GLU MLP with a residual.  PoolBlock: (5 x 5 average over
the in-image taps) - x, 1x1 conv to 2C, LeakyReLU, replicate pad, depthwise 3x3, GLU, 1x1 conv, residual.
``mut`` names one deliberate mistake (tests/test_outpaint_cpu.py shows that the checks catch each).
Cases, seeds and the test inputs are defined here and nowhere else."""
import math

import torch
import torch.nn.functional as F

WEIGHT_SEED = 20261
UNIT = 64

# name -> (B, H, W, max_size, masks per image, seed)
CASES = {
    "a": (1, 64, 64, 640, ("three",), 21),          # one window, no pad: x is non-zero under the mask and goes in unmasked
    "b": (1, 40, 24, 640, ("all",), 22),            # both sides pad up to one window
    "c": (2, 72, 100, 640, ("top", "right"), 23),   # pad to 128 x 128 (4 windows), crop after the upsample
    "d": (1, 136, 200, 640, ("left_half",), 24),    # non-square map 24 x 32: 3 x 4 windows
    "e": (1, 150, 84, 96, ("three",), 25),          # tall resize branch, mask dilation, resize back
    "f": (1, 90, 170, 128, ("three",), 26),         # wide resize branch
    "g": (1, 700, 396, 640, ("three",), 27),        # the real limit
}
FIXTURE_CASES = ("a", "b", "c", "e", "f")           # raw outputs recorded from the reference class
FIXTURE_TAP_CASES = ("a", "b", "e")                 # and the five taps
TAPS = ("dct", "enc", "mid", "dec", "proj")
MUTATIONS = ("bias_transposed", "pool_div25", "dw_zero_pad", "mask_unpadded", "merged_resize", "skip_last_window_row")


def band_mask(kind, H, W):
    m = torch.zeros(1, H, W, dtype=torch.bool)
    if kind in ("top", "three"):
        m[:, :max(2, H // 8)] = True
    if kind in ("right", "three"):
        m[:, :, W - max(2, W // 10):] = True
    if kind in ("left_half", "three"):
        m[:, H // 2:, :W // 12 + 1] = True
    if kind == "all":
        m[:] = True
    return m


def case_input(name):
    """-> x [B,3,H,W] in [0,1] (a smooth picture plus noise, NOT zeroed under the mask), mask [B,1,H,W] bool."""
    B, H, W, _, kinds, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, H // 12 + 2, W // 12 + 2, generator=g)
    x = torch.clamp(0.8 * F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
                    + 0.2 * torch.rand(B, 3, H, W, generator=g), 0, 1)
    return x, torch.stack([band_mask(k, H, W) for k in kinds])


def net_size(H, W, max_size):
    """The size the net sees before its pad (:179-186); Python's round on a double."""
    if max(H, W) <= max_size:
        return H, W
    if H > W:
        return max_size, round(W * (max_size / H))
    return round(H * (max_size / W)), max_size


def resized_pooled_mask(mask, max_size, dtype=torch.float32):
    """The values the ``> 0.5`` threshold of :191 sees (None when infer does not resize)."""
    H, W = mask.shape[-2:]
    nh, nw = net_size(H, W, max_size)
    if (nh, nw) == (H, W):
        return None
    return F.max_pool2d(F.interpolate(mask.to(dtype), (nh, nw), mode="bilinear", align_corners=False), 3, 1, 1)


def score_bias_table(sd, p, dtype):
    """to_bias(delta)[index] as [64, 64]: Linear(2, 16) -> GELU -> Linear(16, 1) over the 225 unique offsets."""
    g = lambda k: sd[f"{p}.bias.{k}"].to(dtype)     # noqa: E731
    hid = F.gelu(g("delta") @ g("to_bias.0.weight").t() + g("to_bias.0.bias"))
    return (hid @ g("to_bias.2.weight").t() + g("to_bias.2.bias"))[sd[f"{p}.bias.index"].long()].reshape(64, 64)


def conv1(sd, p, x, dtype):
    return F.conv2d(x, sd[p + ".weight"].to(dtype), sd[p + ".bias"].to(dtype))


def mha_block(sd, p, x, dtype, mut=()):
    B, C, H, W = x.shape
    heads = C // 32
    t = x.reshape(B, C, H // 8, 8, W // 8, 8).permute(0, 2, 4, 3, 5, 1).reshape(-1, 64, C)      # [windows, tokens, C]
    qkv = t @ sd[p + ".mha.mha.qkv_proj.weight"].to(dtype).t() + sd[p + ".mha.mha.qkv_proj.bias"].to(dtype)
    q, k, v = (u.reshape(-1, 64, heads, 32).transpose(1, 2) for u in qkv.split(C, dim=-1))
    table = score_bias_table(sd, p, dtype)
    if "bias_transposed" in mut:
        table = table.t()
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32) + table, dim=-1) @ v
    a = a.transpose(1, 2).reshape(-1, 64, C) @ sd[p + ".mha.mha.head_proj.weight"].to(dtype).t() + sd[p + ".mha.mha.head_proj.bias"].to(dtype)
    a = a.reshape(B, H // 8, W // 8, 8, 8, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)
    if "skip_last_window_row" in mut:
        a = a.clone()
        a[:, :, H - 8:] = 0
    x = x + a
    return x + conv1(sd, p + ".mlp.2", F.glu(conv1(sd, p + ".mlp.0", x, dtype), dim=1), dtype)


def pool_block(sd, p, x, dtype, mut=()):
    x1 = F.avg_pool2d(x, 5, 1, 2, count_include_pad="pool_div25" in mut) - x
    h = F.leaky_relu(conv1(sd, p + ".mlp.0", x1, dtype), 0.2)
    h = F.pad(h, (1, 1, 1, 1), mode="constant" if "dw_zero_pad" in mut else "replicate")
    h = F.conv2d(h, sd[p + ".mlp.3.weight"].to(dtype), sd[p + ".mlp.3.bias"].to(dtype), groups=h.shape[1])
    return x + conv1(sd, p + ".mlp.5", F.glu(h, dim=1), dtype)


def net(sd, x, mask_f, dtype, mut=()):
    """x [B,3,Hp,Wp], mask_f [B,1,Hp,Wp] (sides multiples of 64) -> z [B,3,Hp,Wp] and the five taps."""
    taps = {}
    h = torch.cat([x, mask_f], dim=1)
    for i in (1, 4, 7):
        h = F.leaky_relu(F.conv2d(F.pad(h, (1, 1, 1, 1), mode="replicate"), sd[f"net.dct.blocks.{i}.weight"].to(dtype),
                                  sd[f"net.dct.blocks.{i}.bias"].to(dtype), stride=2), 0.2)
    taps["dct"] = h
    h = pool_block(sd, "net.enc_block.1", mha_block(sd, "net.enc_block.0", h, dtype, mut), dtype, mut)
    taps["enc"] = h
    m = conv1(sd, "net.proj_mid", h, dtype)
    for i in (0, 2):
        m = pool_block(sd, f"net.mid_block.{i + 1}", mha_block(sd, f"net.mid_block.{i}", m, dtype, mut), dtype, mut)
    h = h + conv1(sd, "net.proj_out", m, dtype)
    taps["mid"] = h
    h = pool_block(sd, "net.dec_block.1", mha_block(sd, "net.dec_block.0", h, dtype, mut), dtype, mut)
    taps["dec"] = h
    taps["proj"] = conv1(sd, "net.to_image_biliner.proj", h, dtype)
    return F.interpolate(taps["proj"], scale_factor=8, mode="bilinear", align_corners=False), taps


def padded_net(sd, x, mask, dtype, mut=()):
    """OutpaintBase.forward: pad right / bottom to a multiple of 64 (x replicated, mask ones), mask x only when padded, crop."""
    H, W = x.shape[-2:]
    ph, pw = (-H) % UNIT, (-W) % UNIT
    mask_f = mask.to(dtype)
    if ph or pw:
        x = F.pad(x, (0, pw, 0, ph), mode="replicate")
        mask_f = F.pad(mask_f, (0, pw, 0, ph), value=1.0)
    if ph or pw or "mask_unpadded" in mut:
        x = x * (1 - mask_f)
    z, taps = net(sd, x, mask_f, dtype, mut)
    return z[:, :, :H, :W], taps


def infer(sd, x, mask, max_size=640, mode="raw", dtype=torch.float64, mut=()):
    """-> (output [B,3,H,W] of LightOutpaintV1.infer (``composite`` / ``raw``) or of its eval forward (``forward``), taps)."""
    src, src_mask = x.to(dtype), mask.bool()
    H, W = x.shape[-2:]
    x = src
    nh, nw = net_size(H, W, max_size) if mode != "forward" else (H, W)
    if (nh, nw) != (H, W):
        x = F.interpolate(x, (nh, nw), mode="bilinear", align_corners=False)
        m = F.max_pool2d(F.interpolate(src_mask.to(dtype), (nh, nw), mode="bilinear", align_corners=False), 3, 1, 1) > 0.5
        x = torch.where(m, torch.zeros((), dtype=dtype), x)
    else:
        m = src_mask
    if "merged_resize" in mut and (nh, nw) != (H, W):
        # one gather from the map straight to (H, W) instead of x8 -> crop -> resize
        _, taps = padded_net(sd, x, m, dtype, mut)
        Hp, Wp = nh + (-nh) % UNIT, nw + (-nw) % UNIT
        z = F.interpolate(taps["proj"], (round(Hp * H / nh), round(Wp * W / nw)), mode="bilinear", align_corners=False)[:, :, :H, :W]
    else:
        z, taps = padded_net(sd, x, m, dtype, mut)
        if z.shape[-2:] != (H, W):
            z = F.interpolate(z, (H, W), mode="bilinear", align_corners=False)
    return finish(src, src_mask, z, mode), taps


def finish(src, src_mask, z, mode):
    """The tail of infer / forward on the net's output z at the frame's size (:164-173, :201-206)."""
    m3 = src_mask.expand_as(src)
    if mode == "raw":
        return z
    if mode == "composite":
        return torch.where(m3, z.clamp(0, 1), src.to(z.dtype))
    mf = m3.to(z.dtype)
    return (src.to(z.dtype) * (1 - mf) + z * mf).clamp(0, 1)


# ---- the EMA frame buffer (stlizer/multipass_pipeline.py:447-474) ----------------------------------------------------------------

def blend_weight(buffer_decay, fps):
    d = min(max(0.5, (1.0 - buffer_decay) * (29.97 / float(fps))), 1.0)
    return 1.0 - d


def buffer_step(frames, coarse, buffer, reset, d, dtype):
    """frames [B,3,H,W] with NaN outside, coarse [B,3,H,W], buffer [3,H,W] or None, reset [B] -> (frames out, buffer).  The blend
    weights are the fp32 roundings of d and 1 - d in every dtype: they are inputs of the step, not part of its arithmetic."""
    frames, coarse = frames.to(dtype), coarse.to(dtype)
    d_old, d_new = float(torch.tensor(d, dtype=torch.float32)), float(torch.tensor(1.0 - d, dtype=torch.float32))
    buf = None if buffer is None else buffer.to(dtype).clone()
    out = []
    for j in range(frames.shape[0]):
        if buf is None or reset[j]:
            buf = coarse[j].clone()
        buf = buf * d_old + coarse[j] * d_new
        out.append(torch.where(torch.isnan(frames[j]), buf, frames[j]).clamp(0, 1))
    return torch.stack(out), buf


def buffer_case(B, H=37, W=53, seed=31, clean_frame=None):
    """Frames with a NaN border of varying width (per channel the same, as the warp leaves it, plus a few single-element NaN so
    that the per-element mask shows), coarse views a little outside [0, 1]."""
    g = torch.Generator().manual_seed(seed + B)
    frames = torch.rand(B, 3, H, W, generator=g) * 1.1 - 0.05
    coarse = torch.rand(B, 3, H, W, generator=g) * 1.2 - 0.1
    for j in range(B):
        if j == clean_frame:
            continue
        frames[j, :, :2 + j] = math.nan
        frames[j, :, :, W - 3 - j:] = math.nan
        frames[j, 1, H // 2, 5 + j] = math.nan
    return frames, coarse


def border(sd, batches, scene_weights, buffer_decay, fps, dtype, max_size=640):
    """stabilizer_callback :447-474 after the warp, over a stream of batches z (NaN outside): the list of output batches."""
    out, buf = [], None
    d = blend_weight(buffer_decay, fps) if buffer_decay > 0 else 0.0
    for z, sw in zip(batches, scene_weights):
        z = z.to(dtype)
        masks = torch.isnan(z)
        zeroed = torch.where(masks, torch.zeros((), dtype=dtype), z)
        if buffer_decay > 0:
            coarse, _ = infer(sd, zeroed, masks[:, 0:1], max_size, "raw", dtype)
            frames, buf = buffer_step(z, coarse, buf, [w < 0.01 for w in sw], d, dtype)
        else:
            frames, _ = infer(sd, zeroed, masks[:, 0:1], max_size, "composite", dtype)
        out.append(frames)
    return out
