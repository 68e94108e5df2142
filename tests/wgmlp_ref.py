"""``waifu2x.wgmlp_4x`` restated in torch on a state dict (helper module, not a conftest): the float64 / fp32 reference of the HIP
engine's tests, with a hook for every tap, and — under ``oracle.fp16_emulation.fp16_autocast_emulation`` with ``half_weights`` — the
fp16 yardstick.  Follows waifu2x/models/wgmlp.py (reference): GLUConvMLP :15-35, MLP :38-52, WGMLPBlock :75-101, Overscan :126-153,
IR :156-173, PatchDown :176-200, PatchUp :203-226, ToImage :229-242, SourceResidual :245-286, get_shift_config :289-295, _forward
:339-353, and nunif/modules/attention.py GMLP :621-651, WindowGMLP2d :654-693.  Pinned to the reference's own class by
tests/golden/wgmlp.npz (tests/test_wgmlp_cpu.py).

``mut``: a set of names of deliberate mistakes, the ones a kernel is likely to make (tests/test_wgmlp_cpu.py shows that the seeded
weights and inputs see each of them): ``mix_transposed``, ``pad_zero``, ``ln2_on_u``, ``shift_order``, ``down_strided``,
``up_repeat``, ``dilation_swapped``, ``patch_crop``, ``gelu_tanh``.
"""
import torch
import torch.nn.functional as F

WINDOW = 8
GROUPS = (("wgmlp1", 2), ("wgmlp2", 4), ("wgmlp3", 3))
GMLP_TAPS = ("ln1", "gelu", "ln2", "mix", "gate")
MUTATIONS = ("mix_transposed", "pad_zero", "ln2_on_u", "shift_order", "down_strided", "up_repeat", "dilation_swapped", "patch_crop",
             "gelu_tanh")


def shift_config(n, mut=()):
    """get_shift_config :289-295 (last=False): REVERSED, block i is shifted iff n - 1 - i is odd."""
    s = [i % 2 == 1 for i in range(n)]
    return tuple(s) if "shift_order" in mut else tuple(reversed(s))


def block_prefixes():
    return [f"unet.{g}.blocks.{i}." for g, n in GROUPS for i in range(n)]


def _windows(x):
    """[B,H,W,C] -> [B nwy nwx, 64, C], token t = 8 row + column (permute.py bchw_to_bnc)."""
    B, H, W, C = x.shape
    return x.reshape(B, H // WINDOW, WINDOW, W // WINDOW, WINDOW, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, WINDOW * WINDOW, C)


def _unwindows(t, shape):
    B, H, W, C = shape
    return t.reshape(B, H // WINDOW, W // WINDOW, WINDOW, WINDOW, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


def window_gmlp(sd, p, x, shift, taps=None, mut=()):
    """WindowGMLP2d.forward(x, norm1, norm2) of block ``p`` on an NHWC map [B,H,W,C]; ``taps``: a dict that receives the five inner
    maps (``GMLP_TAPS``) as NHWC maps of the un-padded extent."""
    B, H, W, C = x.shape
    pad = WINDOW // 2 if shift else 0
    xp = F.pad(x, (0, 0, pad, pad, pad, pad)) if shift else x
    shape = xp.shape
    inside = None
    if "pad_zero" in mut and shift:
        inside = F.pad(torch.ones(B, H, W, 1, dtype=x.dtype), (0, 0, pad, pad, pad, pad))
    t = _windows(xp)
    g = p + "gmlp.gmlp."
    ln1 = F.layer_norm(t, (C,), sd[p + "norm1.weight"], None, 1e-5)
    h = F.linear(ln1, sd[g + "proj_in.weight"], sd[g + "proj_in.bias"])
    h = F.gelu(h, approximate="tanh") if "gelu_tanh" in mut else F.gelu(h)
    u, v = h.chunk(2, dim=-1)
    if "ln2_on_u" in mut:
        u = F.layer_norm(u, (C,), sd[p + "norm2.weight"], None, 1e-5)
        ln2 = v
    else:
        ln2 = F.layer_norm(v, (C,), sd[p + "norm2.weight"], None, 1e-5)
    if inside is not None:
        ln2 = ln2 * _windows(inside)
    ws = sd[g + "proj_spatial.weight"]
    if "mix_transposed" in mut:
        ws = ws.transpose(0, 1).contiguous()
    mix = F.conv1d(ln2, ws, sd[g + "proj_spatial.bias"])
    gate = u * mix
    out = F.linear(gate, sd[g + "proj_out.weight"], sd[g + "proj_out.bias"]) + t

    def back(m):
        m = _unwindows(m, shape[:3] + (m.shape[-1],))
        return m[:, pad:pad + H, pad:pad + W] if shift else m

    if taps is not None:
        taps.update(ln1=back(ln1), gelu=back(h), ln2=back(ln2), mix=back(mix), gate=back(gate))
    return back(out)


def _conv(sd, key, x, **kw):
    return F.conv2d(x, sd[key + ".weight"], sd.get(key + ".bias"), **kw)


def _rpad(x, n):
    return F.pad(x, (n,) * 4, mode="replicate")


def block(sd, p, x, shift, glu, mut=()):
    """WGMLPBlock.forward :92-101 on NCHW."""
    x = window_gmlp(sd, p, x.permute(0, 2, 3, 1), shift, None, mut).permute(0, 3, 1, 2)
    h = _conv(sd, p + "conv_mlp.w1", x)
    if glu:
        h = F.leaky_relu(_conv(sd, p + "conv_mlp.w2", _rpad(F.glu(h, dim=1), 1)), 0.2)
    else:
        h = _conv(sd, p + "conv_mlp.w2", F.leaky_relu(h, 0.1))
    return x + h


def ir_stem(sd, x, mut=()):
    """IR.forward :165-173 with Overscan.forward :141-153."""
    P = "unet.ir."
    d2, d3 = (3, 2) if "dilation_swapped" in mut else (2, 3)
    s0 = F.leaky_relu(_conv(sd, P + "patch", _rpad(x, 1)), 0.2)
    x1 = F.leaky_relu(_conv(sd, P + "overscan.conv1", _rpad(s0, 7)), 0.2)
    x2 = F.leaky_relu(_conv(sd, P + "overscan.conv2", x1, dilation=d2), 0.2)
    x3 = F.leaky_relu(_conv(sd, P + "overscan.conv3", x2, dilation=d3), 0.2)
    c1 = (x1.shape[-1] - x3.shape[-1]) // 2
    c2 = (x2.shape[-1] - x3.shape[-1]) // 2
    x4 = torch.cat([x1[:, :, c1:-c1, c1:-c1], x2[:, :, c2:-c2, c2:-c2], x3], dim=1)
    ov = _conv(sd, P + "overscan.fuse.2", F.leaky_relu(_conv(sd, P + "overscan.fuse.0", x4), 0.2))
    return _conv(sd, P + "fusion", _rpad(torch.cat([s0, ov], dim=1), 1))


def forward(sd, x, taps=None, raw=False, mut=()):
    """WGMLP4x.forward in eval mode: x [B,3,T,T] -> [B,3,4T-72,4T-72], clamped unless ``raw``.  ``taps``: a dict that receives
    ``ir`` (NCHW) and every block's output under its prefix as an NHWC map."""
    P = "unet."
    f = ir_stem(sd, x, mut)
    if taps is not None:
        taps["ir"] = f
    f = _conv(sd, P + "patch", f)
    f = f[:, :, 8:-6, 8:-6] if "patch_crop" in mut else f[:, :, 7:-7, 7:-7]
    f = F.leaky_relu(f, 0.2)
    maps = {}
    for group, n in GROUPS:
        if group == "wgmlp2":
            skip = f
            sc = F.pixel_unshuffle(f, 2)
            B, C4, H, W = sc.shape
            if "down_strided" in mut:
                sc = sc.view(B, 2, C4 // 2, H, W).mean(dim=1)
            else:
                sc = sc.view(B, C4 // 2, 2, H, W).mean(dim=2)
            f = sc + F.leaky_relu(_conv(sd, P + "down1.conv", f, stride=2), 0.2)
        if group == "wgmlp3":
            sc = f.repeat(1, 2, 1, 1) if "up_repeat" in mut else f.repeat_interleave(2, dim=1)
            f = F.pixel_shuffle(sc, 2) + F.pixel_shuffle(F.leaky_relu(_conv(sd, P + "up1.proj", f), 0.2), 2)
            f = f + skip
        shifts = shift_config(n, mut)
        for i in range(n):
            p = f"{P}{group}.blocks.{i}."
            f = block(sd, p, f, shifts[i], not (group == "wgmlp3" and i == n - 1), mut)
            maps[p] = f.permute(0, 2, 3, 1)
    if taps is not None:
        taps.update(maps)
    r = F.pixel_shuffle(_conv(sd, P + "to_residual_image.proj", f), 4)[:, :, 4:-4, 4:-4]
    src = F.pixel_shuffle(F.conv2d(_rpad(x, 1), sd[P + "to_image.resampling.weight"]), 4)
    unpad = (r.shape[2] - src.shape[2]) // 2
    if unpad != 0:
        src = F.pad(src, (unpad,) * 4)
    z = src + r * sd[P + "to_image.scale_bias"]
    return z if raw else torch.clamp(z, 0.0, 1.0)


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def forward64(sd, x, **kw):
    return forward(cast(sd, torch.float64), x.double(), **kw)


def emulated(sd, x, **kw):
    """The reference's fp16 autocast arithmetic (oracle/fp16_emulation.py): the yardstick of the localised bounds."""
    from oracle.fp16_emulation import fp16_autocast_emulation, half_weights
    with fp16_autocast_emulation():
        return forward(half_weights(sd), x.float(), **kw)


def gelu_tail_weights(sd, p):
    """``sd`` with block ``p``'s proj_in scaled by 0.05 and its bias lowered by 3.7: every pre-activation of the GELU lies in about
    [-3.9, -3.5].  That is where the erf form and its tanh approximation can be told apart by an fp16 yardstick: they differ by
    2e-4 there, a quarter of the value, while the reference's own fp16 error (half an ulp of z, 1e-3, times gelu'(z) < 3e-3, plus the
    rounding of a value below 1e-3) is under 5e-6.  Around z = +-2, where a net's activations usually are, the two forms differ by
    5e-4 at most and one fp16 rounding of the value is as large.  Used by the ``gelu_tanh`` case of tests/test_wgmlp_cpu.py and by
    the GPU case that holds the kernel's GELU there (tests/test_gpu_wgmlp.py)."""
    out = dict(sd)
    k = p + "gmlp.gmlp.proj_in."
    out[k + "weight"] = sd[k + "weight"] * 0.05
    out[k + "bias"] = sd[k + "bias"] - 3.7
    return out


def gmlp_input(seed, B, H, W, C):
    """An NHWC map for the kernel-alone tests: fp16-exact values, every channel at a scale of its own."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, C, generator=g) * (1.0 + torch.rand(1, 1, 1, C, generator=g))).half().float()


def gmlp64(sd, p, x, shift, taps=None):
    return window_gmlp(cast(sd, torch.float64), p, x.double(), shift, taps)


def gmlp_emulated(sd, p, x, shift, taps=None):
    from oracle.fp16_emulation import fp16_autocast_emulation, half_weights
    with fp16_autocast_emulation():
        return window_gmlp(half_weights(sd), p, x.float(), shift, taps)


def test_input(seed, B, T):
    """A smooth picture plus texture in [0, 1]: every channel and position differs, nothing saturates."""
    g = torch.Generator().manual_seed(seed)
    low = F.interpolate(torch.rand(B, 3, T // 8 + 2, T // 8 + 2, generator=g), size=(T, T), mode="bicubic", align_corners=False)
    return (0.15 + 0.7 * low.clamp(0, 1) + 0.1 * (torch.rand(B, 3, T, T, generator=g) - 0.5)).clamp(0, 1).contiguous()


test_input.__test__ = False
