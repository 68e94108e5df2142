"""``inpaint.light_inpaint_v1`` on the HIP engine.

Mirrors ``iw3/models/light_inpaint_v1.py`` ``LightInpaintV1`` :53-161: registry name, i2i geometry (scale 1, offset 16,
blend 8), the ``state_dict`` key layout and ``infer(x, mask, closing, inner_dilation, outer_dilation, base_width)`` :106-110
(= ``preprocess`` :93-104 + ``forward(..., skip_i2i_offset=True)``), which is what ``MLBWInpaintImage`` calls.  The whole
of it is one C call, ``nunif_hip_light_inpaint_infer`` (nunif_amd/csrc/light_inpaint.hip).  The training-style
``forward(x, soft_mask)`` entry is not provided.
"""
import ctypes
import math
from collections import OrderedDict

import torch

from ...nunif.models import I2IBaseModel, register_model
from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine

OFFSET = 16


def _init_weights():
    """Fresh weights in the reference's key layout (basic_module_init-style scales; proj_spatial ~ 0 with bias 1)."""
    sd = OrderedDict()

    def lin(key, *shape):
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        sd[key + ".weight"] = torch.randn(shape) * math.sqrt(1.0 / fan_in)
        sd[key + ".bias"] = torch.zeros(shape[0])

    def block(p, C, ws):
        N = ws * ws
        lin(p + "gmlp.gmlp.proj_in", 4 * C, C)
        sd[p + "gmlp.gmlp.proj_spatial.weight"] = (torch.rand(N, N, 1) * 2 - 1) * (1e-3 / C)
        sd[p + "gmlp.gmlp.proj_spatial.bias"] = torch.ones(N)
        lin(p + "gmlp.gmlp.proj_out", C, 2 * C)
        sd[p + "norm1.weight"] = torch.ones(C)
        sd[p + "norm2.weight"] = torch.ones(2 * C)
        lin(p + "glu_conv.w1", C, C, 1, 1)
        lin(p + "glu_conv.w2", C, C // 2, 3, 3)

    sd["mask_bias"] = torch.randn(1, 96, 1, 1) * 0.01
    lin("patch.0", 96, 48, 1, 1)
    block("enc1.", 96, 16)
    lin("down", 192, 96, 2, 2)
    for i in range(4):
        block(f"enc2.{i}.", 192, 8)
    lin("up", 384, 192, 1, 1)
    block("dec1.", 96, 16)
    lin("to_image.1", 48, 96, 3, 3)
    return sd


class HipLightInpaintEngine(HipEngine):
    def __init__(self, state_dict, device):
        super().__init__(device, state_dict, "nunif_hip_light_inpaint_create", "nunif_hip_light_inpaint_destroy",
                         label="light_inpaint")
        self.dim, self.video = int(state_dict["mask_bias"].numel()), "patch.weight" in state_dict

    def infer(self, x, mask, closing, inner_iter, outer_iter, mirror_x=False):
        B, C, H, W = x.shape
        assert C == 3 and tuple(mask.shape) == (B, 1, H, W)
        out = torch.empty_like(x)
        self.call(_hip.lib().nunif_hip_light_inpaint_infer_ex, self.handle, ctypes.c_void_p(x.data_ptr()),
                  ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, H, W, 1 if closing else 0, int(inner_iter),
                  int(outer_iter), 1 if mirror_x else 0)
        return out

    TAPS = ("hard", "soft", "mtok", "patch", "enc1.gmlp", "enc1", "down") + tuple(
        f"enc2.{i}{s}" for i in range(5) for s in (".gmlp", "")) + ("up", "dec1.gmlp", "dec1", "to_image")

    def debug_taps(self, x, mask, closing, inner_iter, outer_iter, mirror_x=False, names=None):
        """``infer`` that also returns the maps of the forward (tests only; ``nunif_hip_light_inpaint_debug_taps``): (out, {name: map}),
        every map NCHW at its own resolution — ``hard`` / ``soft`` fp32 [B,1,H,W], ``mtok`` bool [B,1,h1,w1], the rest fp16."""
        B, C, H, W = x.shape
        assert C == 3 and tuple(mask.shape) == (B, 1, H, W)
        dim, n2 = self.dim, 5 if self.video else 4
        h1, w1 = (H + 64 - H % 64) // 4, (W + 64 - W % 64) // 4
        names = [n for n in self.TAPS if not n.startswith(f"enc2.{n2}")] if names is None else list(names)
        assert set(names) <= set(self.TAPS), sorted(set(names) - set(self.TAPS))
        bufs = {}
        for n in names:
            if n in ("hard", "soft"):
                bufs[n] = torch.empty(B, 1, H, W, dtype=torch.float32, device=x.device)
            elif n == "mtok":
                bufs[n] = torch.empty(B, 1, h1, w1, dtype=torch.uint8, device=x.device)
            elif n == "to_image":
                bufs[n] = torch.empty(B, h1, w1, 64 if n2 == 5 else 48, dtype=torch.float16, device=x.device)
            elif n == "down" or n.startswith("enc2."):
                bufs[n] = torch.empty(B, h1 // 2, w1 // 2, 2 * dim, dtype=torch.float16, device=x.device)
            else:
                bufs[n] = torch.empty(B, h1, w1, dim, dtype=torch.float16, device=x.device)
        ptrs = (ctypes.c_void_p * len(self.TAPS))(*[bufs[n].data_ptr() if n in bufs else None for n in self.TAPS])
        out = torch.empty_like(x)
        self.call(_hip.lib().nunif_hip_light_inpaint_debug_taps, self.handle, ctypes.c_void_p(x.data_ptr()),
                  ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, H, W, 1 if closing else 0, int(inner_iter),
                  int(outer_iter), 1 if mirror_x else 0, ptrs, len(self.TAPS))
        taps = {}
        for n, t in bufs.items():
            taps[n] = t if t.dim() == 4 and t.dtype != torch.float16 else t.permute(0, 3, 1, 2)[:, :48 if n == "to_image" else None]
        taps["mtok"] = taps["mtok"].bool() if "mtok" in taps else None
        return out, {k: v for k, v in taps.items() if v is not None}


@register_model
class LightInpaintV1(FlatWeightsMixin, I2IBaseModel):
    name = "inpaint.light_inpaint_v1"

    def __init__(self):
        super().__init__({}, scale=1, offset=OFFSET, in_channels=3, blend_size=8)
        self.downscaling_factor, self.mod = 4, 16
        self._setup_weights(_init_weights())

    def _make_engine(self, device):
        return HipLightInpaintEngine(self._weights, device)

    supports_mirror_x = True

    def infer(self, x, mask, closing=False, inner_dilation=0, outer_dilation=0, base_width=None, mirror_x=False):
        """x [B,3,H,W] float in [0,1], mask [B,1,H,W] bool (True = hole) -> inpainted [B,3,H,W].
        ``mirror_x`` (not in the reference): ``flip(infer(flip(x), mask))`` with ``mask`` given in the flipped frame, no flip passes."""
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        dev = self.get_device()
        W = x.shape[-1]

        def n_iter(n):          # dilate_inner / dilate_outer (iw3/dilation.py:74-103)
            if n <= 0:
                return 0
            return max(round(W / base_width * n), 1) if base_width is not None else n
        m = mask.to(device=dev)
        # the engine takes a byte per pixel, hole = non-zero: a bool mask IS that (zero-copy view), a uint8 mask passes as it is
        if m.dtype == torch.bool:
            m = m.contiguous().view(torch.uint8)
        elif m.dtype != torch.uint8:
            m = (m > 0).to(torch.uint8)
        m = m.contiguous()
        dtype = x.dtype
        out = self.engine().infer(x.to(device=dev, dtype=torch.float32).contiguous(), m, closing,
                                  n_iter(inner_dilation), n_iter(outer_dilation), mirror_x=mirror_x)
        return out.to(dtype)

    def forward(self, x, mask, skip_i2i_offset=False):
        raise NotImplementedError("the HIP engine implements LightInpaintV1.infer (hard hole mask in, inpainted frame out); "
                                  "the training-style forward(x, soft_mask) is not provided")
