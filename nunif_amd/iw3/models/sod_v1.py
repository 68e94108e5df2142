"""iw3 ``iw3.sod_v1`` (salient-object net of ``--convergence-mode sod_v1``) on the HIP engine.

Mirrors ``iw3/models/sod_v1.py`` (reference) ``SODV1`` :9-56 — registry name and alias, ``i2i_*`` attributes (scale 1, offset 0,
in_channels 4, blend_size 0, in_size 192), ``fuse()`` / ``compile()`` (no-ops here: BatchNorm is always folded and there is nothing
to compile), ``infer(rgb, depth)`` :49-56 and the ``state_dict`` key layout of ``U2NETP(in_ch=6)`` (``nunif/utils/u2netp.py``
:321-356) under ``u2netp.``, so ``iw3_sod_v1_20260125.pth`` loads unchanged.  The net is ``nunif_hip_sod_v1_forward``
(nunif_amd/csrc/sod_v1.hip): fp32 operands and accumulation.
"""
import ctypes
import math
from collections import OrderedDict

import torch

from ...nunif.models import I2IBaseModel, register_model
from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine

NET_SIZE = 192
BN_EPS = 1e-5
# (stage, RSU height L — 0 is RSU4F —, in_ch): U2NETP.__init__ :325-347 in registration order
STAGES = (("stage1", 7, 6), ("stage2", 6, 64), ("stage3", 5, 64), ("stage4", 4, 64), ("stage5", 0, 64), ("stage6", 0, 64),
          ("stage5d", 0, 128), ("stage4d", 4, 128), ("stage3d", 5, 128), ("stage2d", 6, 128), ("stage1d", 7, 128))
MID_CH, OUT_CH = 16, 64


def rebnconvs():
    """[(prefix under u2netp., in_ch, out_ch, dilation)] of every REBNCONV in registration order (RSU7 :48-74 and its kin)."""
    out = []
    for stage, L, in_ch in STAGES:
        n = L or 4
        flat = L == 0                                          # RSU4F: no pooling, dilations 1, 2, 4, 8
        out.append((f"{stage}.rebnconvin", in_ch, OUT_CH, 1))
        out.append((f"{stage}.rebnconv1", OUT_CH, MID_CH, 1))
        for i in range(2, n + 1):
            out.append((f"{stage}.rebnconv{i}", MID_CH, MID_CH, (2 ** (i - 1)) if flat else (2 if i == n else 1)))
        for i in range(n - 1, 0, -1):
            out.append((f"{stage}.rebnconv{i}d", 2 * MID_CH, MID_CH if i > 1 else OUT_CH, (2 ** (i - 1)) if flat else 1))
    return out


def state_dict_shapes():
    """Ordered ``{key: shape}`` of ``SODV1().state_dict()`` in the reference."""
    sd = OrderedDict()
    for p, cin, cout, _ in rebnconvs():
        k = f"u2netp.{p}."
        sd[k + "conv_s1.weight"] = (cout, cin, 3, 3)
        sd[k + "conv_s1.bias"] = (cout,)
        for name in ("weight", "bias", "running_mean", "running_var"):
            sd[k + "bn_s1." + name] = (cout,)
        sd[k + "bn_s1.num_batches_tracked"] = ()
    for i in range(1, 7):
        sd[f"u2netp.side{i}.weight"] = (1, 64, 3, 3)
        sd[f"u2netp.side{i}.bias"] = (1,)
    sd["u2netp.outconv.weight"] = (1, 6, 1, 1)
    sd["u2netp.outconv.bias"] = (1,)
    return sd


def _init_weights():
    sd = OrderedDict()
    for k, shape in state_dict_shapes().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.long)
        elif k.endswith(("running_var", "bn_s1.weight")):
            sd[k] = torch.ones(shape)
        elif len(shape) == 4:
            sd[k] = torch.randn(shape) * math.sqrt(1.0 / (shape[1] * shape[2] * shape[3]))
        else:
            sd[k] = torch.zeros(shape)
    return sd


def fold_bn(sd, prefix):
    """``fuse_conv_bn_eval`` (u2netp.py:20-26) of one REBNCONV: float64 arithmetic, fp32 result."""
    g = lambda n: sd[prefix + n].double()     # noqa: E731
    scale = g("bn_s1.weight") / torch.sqrt(g("bn_s1.running_var") + BN_EPS)
    w = g("conv_s1.weight") * scale[:, None, None, None]
    b = (g("conv_s1.bias") - g("bn_s1.running_mean")) * scale + g("bn_s1.bias")
    return w.float(), b.float()


def pack_weights(sd):
    """Reference state dict -> the packed fp32 tensors ``nunif_hip_sod_v1_create`` takes (layout: include/nunif_hip.h)."""
    packed = OrderedDict()
    for p, cin, cout, _ in rebnconvs():
        w, b = fold_bn(sd, f"u2netp.{p}.")
        # [co][ci][kh][kw] -> [co / 8][ci][tap][co % 8]
        packed[p + ".w"] = w.reshape(cout // 8, 8, cin, 9).permute(0, 2, 3, 1).contiguous()
        packed[p + ".b"] = b.contiguous()
    packed["side.w"] = torch.stack([sd[f"u2netp.side{i}.weight"].float().reshape(64, 9) for i in range(1, 7)]).contiguous()
    packed["side.b"] = torch.cat([sd[f"u2netp.side{i}.bias"].float().reshape(1) for i in range(1, 7)]).contiguous()
    packed["outconv.w"] = sd["u2netp.outconv.weight"].float().reshape(6).contiguous()
    packed["outconv.b"] = sd["u2netp.outconv.bias"].float().reshape(1).contiguous()
    return packed


TAP_NAMES = ("hx1", "hx2", "hx3", "hx4", "hx5", "hx6", "hx1d")


@register_model
class SODV1(FlatWeightsMixin, I2IBaseModel):
    name = "iw3.sod_v1"
    name_alias = ("iw3.dsod_v1",)

    def __init__(self):
        super().__init__({}, scale=1, offset=0, in_channels=4, blend_size=0, in_size=NET_SIZE)
        self._setup_weights(_init_weights())
        self.eval()

    def _param_filter(self, name, tensor):
        return tensor.is_floating_point() and "running_" not in name

    def _make_engine(self, device):
        return HipEngine(device, pack_weights(self._weights), "nunif_hip_sod_v1_create", "nunif_hip_sod_v1_destroy",
                         self.i2i_in_size, label="sod_v1")

    def fuse(self, mode=True):          # BatchNorm is folded when the weights are packed
        return self

    def compile(self, mode=True):
        return self

    @staticmethod
    def to_feature(depth):
        return torch.cat([depth, depth ** 0.5, depth ** 2], dim=1)

    def _infer(self, rgb, depth):
        """-> (saliency, depth resized, workspace of this run)."""
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        eng = self.engine()
        dev = eng.device
        rgb = rgb.to(device=dev, dtype=torch.float32).contiguous()
        depth = depth.to(device=dev, dtype=torch.float32).contiguous()
        assert rgb.ndim == 4 and rgb.shape[1] == 3 and depth.ndim == 4 and depth.shape[1] == 1 and depth.shape[0] == rgb.shape[0]
        B, s = rgb.shape[0], self.i2i_in_size
        sal = torch.empty((B, 1, s, s), dtype=torch.float32, device=dev)
        depth_scaled = torch.empty((B, 1, s, s), dtype=torch.float32, device=dev)
        ws = torch.empty((_hip.lib().nunif_hip_sod_v1_workspace_floats(B),), dtype=torch.float32, device=dev)
        eng.call(_hip.lib().nunif_hip_sod_v1_forward, eng.handle, ctypes.c_void_p(rgb.data_ptr()), rgb.shape[2], rgb.shape[3],
                 ctypes.c_void_p(depth.data_ptr()), depth.shape[2], depth.shape[3], B, ctypes.c_void_p(ws.data_ptr()),
                 ctypes.c_void_p(sal.data_ptr()), ctypes.c_void_p(depth_scaled.data_ptr()))
        return sal, depth_scaled, ws

    @torch.inference_mode()
    def infer(self, rgb, depth):
        """rgb [B,3,H,W], depth [B,1,h,w] -> (saliency [B,1,192,192], depth resized to 192 x 192), both fp32."""
        return self._infer(rgb, depth)[:2]

    def forward(self, x):
        """x [B,4,192,192] (rgb | depth) -> saliency (:38-46; at the net's own size the entry's resize is the identity)."""
        assert x.ndim == 4 and x.shape[1] == 4 and tuple(x.shape[2:]) == (self.i2i_in_size,) * 2
        return self.infer(x[:, 0:3], x[:, 3:4])[0]

    def debug_taps(self, rgb, depth):
        """Tests only: ``infer`` plus the seven maps hx1 .. hx6, hx1d (u2netp.py:368-404) of that run, ``{name: [B,64,S,S]}``."""
        with torch.inference_mode():
            sal, depth_scaled, ws = self._infer(rgb, depth)
        B = sal.shape[0]
        eng = self.engine()
        taps = {}
        for i, name in enumerate(TAP_NAMES):
            S = NET_SIZE >> (0 if name == "hx1d" else i)
            out = torch.empty((B, 64, S, S), dtype=torch.float32, device=eng.device)
            shape = (ctypes.c_int64 * 4)()
            eng.call(_hip.lib().nunif_hip_sod_v1_debug_taps, eng.handle, ctypes.c_void_p(ws.data_ptr()), B, name.encode(),
                     ctypes.c_void_p(out.data_ptr()), out.numel(), shape)
            assert tuple(shape) == tuple(out.shape)
            taps[name] = out
        return sal, depth_scaled, taps

    def load(self):
        raise RuntimeError("no network access: load the released state dict with nunif.models.load_model / load_state_dict")
