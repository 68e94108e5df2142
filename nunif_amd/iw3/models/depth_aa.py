"""iw3 ``iw3.depth_aa`` (depth anti-aliasing) on the HIP engine.

Mirrors ``iw3/models/depth_aa.py`` (reference) ``DepthAA`` :29-95 — registry name, ``i2i_*`` attributes (scale 1,
offset 0, in_channels 1, blend_size 0), ``infer(x)`` :46-56, ``forward(x, clamp=None)`` :59-85 and the ``state_dict``
key layout (``proj_in``, ``blocks.N.*``, ``proj_out``), so ``iw3_depth_aa_20250530.pth`` loads unchanged.  The net is
``nunif_hip_depth_aa_forward`` (nunif_amd/csrc/depth_aa.hip).
"""
import ctypes
import math
from collections import OrderedDict

import torch

from ...nunif.models import I2IBaseModel, register_model
from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine
from .row_flow_v3 import _score_bias_input


def _init_weights():
    sd = OrderedDict()

    def lin(key, *shape, zero=False):
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        sd[key + ".weight"] = torch.zeros(shape) if zero else torch.randn(shape) * math.sqrt(1.0 / fan_in)
        sd[key + ".bias"] = torch.zeros(shape[0])

    lin("proj_in", 32, 4, 1, 1)
    for i in range(3):
        p = f"blocks.{i}."
        lin(p + "mha.mha.qkv_proj", 96, 32)
        lin(p + "mha.mha.head_proj", 32, 32)
        lin(p + "conv_mlp.0", 32, 32, 1, 1)
        lin(p + "conv_mlp.3", 32, 32, 3, 3)
        sd[p + "bias.index"], sd[p + "bias.delta"] = _score_bias_input((8, 8))
        lin(p + "bias.to_bias.0", 16, 2)
        lin(p + "bias.to_bias.2", 1, 16)
    lin("proj_out", 4, 32, 1, 1, zero=True)           # nn.init.constant_(proj_out.weight, 0)  (depth_aa.py:43)
    return sd


@register_model
class DepthAA(FlatWeightsMixin, I2IBaseModel):
    name = "iw3.depth_aa"

    def __init__(self):
        super().__init__({}, scale=1, offset=0, in_channels=1, blend_size=0)
        self._setup_weights(_init_weights())

    def _make_engine(self, device):
        return HipEngine(device, self._weights, "nunif_hip_depth_aa_create", "nunif_hip_depth_aa_destroy", label="depth_aa")

    def _run(self, x, mode):
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        squeeze = x.ndim == 3
        if squeeze:
            x = x.unsqueeze(0)
        eng = self.engine()
        xin = x.to(device=eng.device, dtype=torch.float32).contiguous()
        B, C, h, w = xin.shape
        assert C == 1
        y = torch.empty_like(xin)
        eng.call(_hip.lib().nunif_hip_depth_aa_forward, eng.handle, ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                 B, h, w, mode)
        y = y.to(x.dtype)
        return y.squeeze(0) if squeeze else y

    @torch.inference_mode()
    def infer(self, x):
        return self._run(x, 2)

    def forward(self, x, clamp=None):
        if clamp is None:
            clamp = True                                  # eval (the only mode the engine has)
        return self._run(x, 1 if clamp else 0)

    def load(self):
        raise RuntimeError("no network access: load the released state dict with nunif.models.load_model / load_state_dict")
