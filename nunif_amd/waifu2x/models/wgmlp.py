"""waifu2x wgmlp_4x (window gMLP + GLU conv-MLP, two-level U-Net) on the HIP engine.

Mirrors ``WGMLP4x`` of ``waifu2x/models/wgmlp.py`` (reference :441-470; ``WGMLPBase`` :298-353, ``tile_size_validator`` :406-409): the
same registry name, constructor kwargs, ``i2i_*`` geometry (scale 4, offset 36, blend 16) and ``state_dict`` keys, so a reference
``.pth`` of this family loads unchanged.  The forward pass is ``nunif_hip_wgmlp_forward`` (nunif_amd/csrc/wgmlp.hip); Python holds the
fp32 master weights only.

Only the registered geometry is carried (``base_dim`` 128, both mlp ratios 2, 3 -> 3 channels): the fused window-gMLP kernel is
instantiated for 128 / 256 channels.  Not carried: the training-time ``tile_mode`` 2 x 2 split (:355-403) and the 19-channel
``IRMixIn`` input form (:412-438, :458-460), whose ``has_callback()`` returns False in the reference so that nothing calls it.
"""
import ctypes
from collections import OrderedDict

import torch
import torch.nn.functional as F

from ...nunif.models import register_model
from ... import _hip
from ...engine import HipEngine
from .swin_unet import _FlatWeightsModel

GEOMETRY = "base_dim 128, lv1_mlp_ratio 2, lv2_mlp_ratio 2, in_channels = out_channels = 3"
FIRST_LAYERS, SECOND_LAYERS, LAST_LAYERS = 2, 4, 3          # WGMLPBase defaults :301, :319-321
WINDOW = 8


def tile_size_validator(size):
    return (size > 16 and
            (size - 16) % 12 == 0 and
            (size - 16) % 16 == 0)


def block_names():
    """The nine ``WGMLPBlock`` prefixes in forward order with their widths and shifts (get_shift_config :289-295: reversed, the last
    block of an even group is the shifted one)."""
    out = []
    for group, n, wide in (("wgmlp1", FIRST_LAYERS, False), ("wgmlp2", SECOND_LAYERS, True), ("wgmlp3", LAST_LAYERS, False)):
        shift = tuple(reversed([i % 2 == 1 for i in range(n)]))
        for i in range(n):
            out.append((f"unet.{group}.blocks.{i}.", 256 if wide else 128, shift[i], not (group == "wgmlp3" and i == n - 1)))
    return out


def _icnr(cout, cin, scale_factor):
    w = torch.zeros(cout // scale_factor ** 2, cin, 1, 1)
    torch.nn.init.kaiming_normal_(w)
    w = F.interpolate(w.permute(1, 0, 2, 3), scale_factor=scale_factor, mode="nearest")
    return F.pixel_unshuffle(w, scale_factor).permute(1, 0, 2, 3).contiguous()


def _init_weights(base_dim=128, mlp_ratio=2):
    """Fresh weights in the reference's key order and with its initialisers (WGMLPBase.__init__ :298-331): kaiming convs and
    truncated-normal Linears with zero biases (basic_module_init), the token mixing near zero with bias 1 (GMLP :631-632), unit norm
    weights, ICNR projections, nearest-neighbour resampling and a zero ``scale_bias`` — a freshly constructed model is the
    nearest-neighbour upscaler, like the reference's."""
    sd = OrderedDict()
    C, C2 = base_dim, base_dim * 2

    def conv(key, cin, cout, k):
        w = torch.empty(cout, cin, k, k)
        torch.nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
        sd[key + ".weight"], sd[key + ".bias"] = w, torch.zeros(cout)

    def linear(key, cin, cout):
        w = torch.empty(cout, cin)
        torch.nn.init.trunc_normal_(w, std=0.02)
        sd[key + ".weight"], sd[key + ".bias"] = w, torch.zeros(cout)

    def block(p, dim, conv_mlp):
        linear(p + "gmlp.gmlp.proj_in", dim, dim * 2)
        n = WINDOW * WINDOW
        sd[p + "gmlp.gmlp.proj_spatial.weight"] = (torch.rand(n, n, 1) * 2 - 1) * (1e-3 / dim)
        sd[p + "gmlp.gmlp.proj_spatial.bias"] = torch.ones(n)
        linear(p + "gmlp.gmlp.proj_out", dim, dim)
        sd[p + "norm1.weight"], sd[p + "norm2.weight"] = torch.ones(dim), torch.ones(dim)
        mid = int(dim * mlp_ratio)
        conv(p + "conv_mlp.w1", dim, mid, 1)
        if conv_mlp:
            conv(p + "conv_mlp.w2", mid // 2, dim, 3)
        else:
            conv(p + "conv_mlp.w2", mid, dim, 1)

    P = "unet."
    conv(P + "ir.patch", 3, 16, 3)
    conv(P + "ir.overscan.conv1", 16, 16, 3)
    conv(P + "ir.overscan.conv2", 16, 8, 3)
    conv(P + "ir.overscan.conv3", 8, 8, 3)
    conv(P + "ir.overscan.fuse.0", 32, 16, 3)
    conv(P + "ir.overscan.fuse.2", 16, 16, 1)
    conv(P + "ir.fusion", 32, 16, 3)
    conv(P + "patch", 16, C, 3)
    names = block_names()
    for p, dim, _, conv_mlp in names[:FIRST_LAYERS]:
        block(p, dim, conv_mlp)
    conv(P + "down1.conv", C, C2, 2)
    for p, dim, _, conv_mlp in names[FIRST_LAYERS:FIRST_LAYERS + SECOND_LAYERS]:
        block(p, dim, conv_mlp)
    sd[P + "up1.proj.weight"], sd[P + "up1.proj.bias"] = _icnr(C * 4, C2, 2), torch.zeros(C * 4)
    for p, dim, _, conv_mlp in names[FIRST_LAYERS + SECOND_LAYERS:]:
        block(p, dim, conv_mlp)
    sd[P + "to_residual_image.proj.weight"], sd[P + "to_residual_image.proj.bias"] = _icnr(48, C, 4), torch.zeros(48)
    sd[P + "to_image.scale_bias"] = torch.zeros(1)
    w = torch.zeros(48, 3, 3, 3)
    for c in range(3):
        w[c * 16:(c + 1) * 16, c, 1, 1] = 1.0          # nearest_neighbor_init :256-271
    sd[P + "to_image.resampling.weight"] = w
    return sd


class HipWGMLPEngine(HipEngine):
    """Owns one ``nunif_wgmlp*`` handle (device weights + workspace) for one device."""

    def __init__(self, state_dict, device):
        super().__init__(device, state_dict, "nunif_hip_wgmlp_create", "nunif_hip_wgmlp_destroy", label="wgmlp")

    @staticmethod
    def _check(x):
        B, C, T, T2 = x.shape
        assert C == 3 and T == T2
        if not tile_size_validator(T):
            raise ValueError(f"tile_size {T} is not valid for waifu2x.wgmlp_4x ((T - 16) a positive multiple of 48)")
        return B, T

    def forward(self, x, clamp=True):
        B, T = self._check(x)
        z = torch.empty((B, 3, 4 * T - 72, 4 * T - 72), dtype=torch.float32, device=self.device)
        self.call(_hip.lib().nunif_hip_wgmlp_forward, self.handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(z.data_ptr()), B, T,
                  1 if clamp else 0)
        return z

    def debug_taps(self, x, clamp=True):
        """``forward`` that also returns every block's output (tests only; ``nunif_hip_wgmlp_debug_taps``): (z, {block prefix:
        [B,S,S,C] fp32 NHWC})."""
        B, T = self._check(x)
        S = T - 16
        z = torch.empty((B, 3, 4 * T - 72, 4 * T - 72), dtype=torch.float32, device=self.device)
        shapes = [(p, (B, S, S, 128) if dim == 128 else (B, S // 2, S // 2, 256)) for p, dim, _, _ in block_names()]
        sizes = [s[0] * s[1] * s[2] * s[3] for _, s in shapes]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        self.call(_hip.lib().nunif_hip_wgmlp_debug_taps, self.handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(z.data_ptr()),
                  ctypes.c_void_p(flat.data_ptr()), B, T, 1 if clamp else 0)
        return z, {p: t.reshape(s) for (p, s), t in zip(shapes, flat.split(sizes))}

    def debug_gmlp(self, block, x, shift, taps=True):
        """The WindowGMLP2d of block ``block`` (0 .. 8) alone on x [B,H,W,C] fp32 NHWC (tests only; ``nunif_hip_wgmlp_debug_gmlp``):
        (out, {"ln1", "gelu", "ln2", "mix", "gate"} fp32 NHWC maps)."""
        B, H, W, C = x.shape
        assert x.dtype == torch.float32 and x.is_contiguous() and C == block_names()[block][1]
        out = torch.empty_like(x)
        maps = {k: torch.empty((B, H, W, C * (2 if k == "gelu" else 1)), dtype=torch.float32, device=self.device)
                for k in ("ln1", "gelu", "ln2", "mix", "gate")} if taps else {}
        ptrs = [ctypes.c_void_p(maps[k].data_ptr()) if taps else None for k in ("ln1", "gelu", "ln2", "mix", "gate")]
        self.call(_hip.lib().nunif_hip_wgmlp_debug_gmlp, self.handle, block, ctypes.c_void_p(x.data_ptr()),
                  ctypes.c_void_p(out.data_ptr()), B, H, W, 1 if shift else 0, *ptrs)
        return out, maps


@register_model
class WGMLP4x(_FlatWeightsModel):
    name = "waifu2x.wgmlp_4x"
    unet_scale_factor = 4

    def __init__(self, in_channels=3, out_channels=3, base_dim=128, lv1_mlp_ratio=2, lv2_mlp_ratio=2, **kwargs):
        super().__init__(dict(in_channels=in_channels, out_channels=out_channels, base_dim=base_dim, lv1_mlp_ratio=lv1_mlp_ratio,
                              lv2_mlp_ratio=lv2_mlp_ratio, **kwargs),
                         scale=4, offset=36, in_channels=in_channels, blend_size=16)
        if in_channels != 3 or out_channels != 3 or base_dim != 128 or lv1_mlp_ratio != 2 or lv2_mlp_ratio != 2:
            raise ValueError(f"the HIP wgmlp engine carries the registered geometry only ({GEOMETRY})")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self._setup_weights(_init_weights(base_dim, lv1_mlp_ratio))
        self.register_tile_size_validator(tile_size_validator)

    def _make_engine(self, device):
        return HipWGMLPEngine(self._weights, device)

    def forward(self, x):
        if x.shape[1] == 16 + 3:
            raise NotImplementedError("the 19-channel IRMixIn input form (wgmlp.py:412-438, :458-460) is not on the HIP engine: "
                                      "has_callback() returns False in the reference and nothing calls it")
        return super().forward(x)

    def has_callback(self):
        return False

    def set_tile_mode(self):
        raise NotImplementedError("tile_mode is a training-time 2 x 2 split (wgmlp.py:355-403); the HIP engine is inference-only")
