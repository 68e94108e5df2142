"""iw3 ``sbs.row_flow_v2`` (``--method row_flow_v2``, the previous default) on the HIP engine.

Mirrors ``iw3/models/row_flow_v2.py`` (reference) ``RowFlowV2`` :9-92 — registry name, ``i2i_*`` attributes (scale 1,
offset 28, in_channels 8, blend_size 4), the ``delta_output`` switch, the ``delta_scale`` buffer and the ``state_dict`` key
layout (``feature.0.*``, ``non_overlap.*``, ``overlap_residual.{0,2,4,6}.*``), so the released
``iw3_row_flow_v2_20240130.pth`` loads unchanged.  Only the inference path the CLI uses is on the engine:
``delta_output = True`` (``_forward_delta_only`` :80-86), called by ``apply_divergence_nn_delta``
(iw3/backward_warp.py:191-236).  The seven convolutions are ONE launch, ``nunif_hip_row_flow_v2_delta``
(nunif_amd/csrc/rowflow_v2.hip).
"""
import ctypes
import math
from collections import OrderedDict

import torch

from ...nunif.models import I2IBaseModel, register_model
from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine

OFFSET = 28
TAPS = (("feature", 16), ("relu1", 16), ("relu2", 32), ("relu3", 32), ("non_overlap", 1), ("residual", 1))


def _init_weights():
    """kaiming_normal_(fan_out, relu) weights and zero biases, as RowFlowV2.__init__ :38-42."""
    sd = OrderedDict()
    sd["delta_scale"] = torch.tensor(1.0 / 127.0)

    def conv(key, cout, cin, kh, kw):
        sd[key + ".weight"] = torch.randn(cout, cin, kh, kw) * math.sqrt(2.0 / (cout * kh * kw))
        sd[key + ".bias"] = torch.zeros(cout)

    conv("feature.0", 16, 3, 1, 3)
    conv("non_overlap", 1, 16, 1, 1)
    conv("overlap_residual.0", 16, 16, 1, 9)
    conv("overlap_residual.2", 32, 16, 1, 9)
    conv("overlap_residual.4", 32, 32, 1, 9)
    conv("overlap_residual.6", 1, 32, 3, 3)
    return sd


class HipRowFlowV2Engine(HipEngine):
    def __init__(self, state_dict, device):
        super().__init__(device, state_dict, "nunif_hip_row_flow_v2_create", "nunif_hip_row_flow_v2_destroy", label="row_flow_v2")

    def delta(self, x, flip=False):
        B, C, h, w = x.shape
        assert C == 3
        out = torch.empty((B, 1, h, w), dtype=torch.float32, device=self.device)
        self.call(_hip.lib().nunif_hip_row_flow_v2_delta, self.handle, ctypes.c_void_p(x.data_ptr()),
                  ctypes.c_void_p(out.data_ptr()), B, h, w, 1 if flip else 0)
        return out

    def debug_taps(self, x, flip=False):
        """delta and the six intermediate maps (``TAPS``) as fp32 [B,C,h,w], for the tests."""
        B, C, h, w = x.shape
        assert C == 3
        out = torch.empty((B, 1, h, w), dtype=torch.float32, device=self.device)
        taps = OrderedDict((name, torch.empty((B, c, h, w), dtype=torch.float32, device=self.device)) for name, c in TAPS)
        self.call(_hip.lib().nunif_hip_row_flow_v2_debug_taps, self.handle, ctypes.c_void_p(x.data_ptr()),
                  ctypes.c_void_p(out.data_ptr()), *(ctypes.c_void_p(t.data_ptr()) for t in taps.values()),
                  B, h, w, 1 if flip else 0)
        return out, taps


@register_model
class RowFlowV2(FlatWeightsMixin, I2IBaseModel):
    name = "sbs.row_flow_v2"

    def __init__(self):
        super().__init__({}, scale=1, offset=OFFSET, in_channels=8, blend_size=4)
        self._setup_weights(_init_weights())
        self.delta_output = False

    @property
    def delta_scale(self):
        return self._weights["delta_scale"]

    def _make_engine(self, device):
        return HipRowFlowV2Engine(self._weights, device)

    def _planes(self, x):
        return x.to(device=self.get_device(), dtype=torch.float32).contiguous()

    def infer_delta(self, x, flip=False):
        """[B,3,h,w] feature planes -> horizontal flow [B,1,h,w]; ``flip`` mirrors the planes inside the kernel's load."""
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        return self.engine().delta(self._planes(x), flip=flip)

    def debug_taps(self, x, flip=False):
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        return self.engine().debug_taps(self._planes(x), flip=flip)

    def forward(self, x):
        if not self.delta_output:
            raise NotImplementedError("the HIP engine implements the delta_output path (what iw3 inference uses); "
                                      "set model.delta_output = True")
        if x.ndim != 4 or x.shape[1] not in (3, 8):
            raise ValueError(f"sbs.row_flow_v2 takes [B,3,h,w] feature planes or the packed [B,8,h,w] input, got {tuple(x.shape)}")
        if x.shape[1] == 8:                     # training-style packed input: rgb | depth feat | grid
            x = x[:, 3:6]
        delta = self.infer_delta(x)
        return torch.cat([delta, torch.zeros_like(delta)], dim=1)            # _forward_delta_only :80-86
