"""iw3 ``iw3.da3mono_disparity`` (depth -> disparity of the Depth-Anything-3 mono model) on the HIP engine.

Mirrors ``iw3/models/da3mono_disparity.py`` (reference) ``DA3MonoDisparity`` :11-76 — registry name, ``i2i_*`` attributes (scale 1,
offset 0, in_channels 1, blend_size 0), the ``state_dict`` key layout (``mlp.0`` / ``mlp.2`` / ``mlp.4`` ``.weight`` / ``.bias``),
the static ``extract_features`` :53-73 and ``forward`` :29-50 for a 3-D and a batched map.  The features are one multi-rank radix
selection per image instead of a full ``torch.sort`` (``nunif_hip_da3mono_features``), the MLP and the per-pixel step follow it in
``nunif_hip_da3mono_forward`` (nunif_amd/csrc/da3_disparity.hip).
"""
import ctypes
import math
from collections import OrderedDict
from functools import lru_cache

import torch

from ...nunif.models import I2IBaseModel, register_model
from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine

FEAT_DIM = 64
HIDDEN = 128


@lru_cache(maxsize=64)
def host_ranks(n):
    """The 62 sorted positions ``extract_features`` :65 reads, by the reference's own expression on the CPU (fp32 ``linspace``
    truncated by ``.long()``): the engine takes them as they are and never re-derives them."""
    return torch.linspace(1, n - 2, FEAT_DIM - 2, device="cpu").long()


_device_ranks = {}


def device_ranks(n, device):
    key = (n, str(device))
    if key not in _device_ranks:
        _device_ranks[key] = host_ranks(n).to(device)
    return _device_ranks[key]


def _init_weights():
    sd = OrderedDict()
    for key, cout, cin in (("mlp.0", HIDDEN, FEAT_DIM), ("mlp.2", HIDDEN, HIDDEN), ("mlp.4", 2, HIDDEN)):
        sd[key + ".weight"] = torch.randn(cout, cin) * math.sqrt(1.0 / cin)
        sd[key + ".bias"] = torch.zeros(cout)
    return sd


def pack_weights(sd):
    """Reference state dict -> the tensors ``nunif_hip_da3mono_create`` takes (layout: include/nunif_hip.h)."""
    f = lambda k: sd[k].detach().float().contiguous()      # noqa: E731
    return OrderedDict([("mlp.0.wt", f("mlp.0.weight").t().contiguous()), ("mlp.0.bias", f("mlp.0.bias")),
                        ("mlp.2.wt", f("mlp.2.weight").t().contiguous()), ("mlp.2.bias", f("mlp.2.bias")),
                        ("mlp.4.weight", f("mlp.4.weight")), ("mlp.4.bias", f("mlp.4.bias"))])


def _maps(x, name):
    """-> (contiguous fp32 [B,1,H,W] on its ROCm device, was batched)."""
    if x.device.type != "cuda":
        raise RuntimeError(f"{name}: tensor must live on a ROCm device (got {x.device}); there is no CPU fallback")
    batch = x.ndim == 4
    assert x.ndim in (3, 4)
    x = x if batch else x.unsqueeze(0)
    assert x.shape[1] == 1, "C must be 1"
    return x.to(torch.float32).contiguous(), batch


@register_model
class DA3MonoDisparity(FlatWeightsMixin, I2IBaseModel):
    name = "iw3.da3mono_disparity"

    def __init__(self):
        super().__init__({}, scale=1, offset=0, in_channels=1, blend_size=0)
        self._setup_weights(_init_weights())
        self.eval()

    def _make_engine(self, device):
        return HipEngine(device, pack_weights(self._weights), "nunif_hip_da3mono_create", "nunif_hip_da3mono_destroy",
                         label="da3mono_disparity")

    def forward(self, depth):
        """depth [1,H,W] or [B,1,H,W] -> disparity of the same shape (:29-50)."""
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        x, batch = _maps(depth, "da3mono_disparity")
        eng = self.engine()
        if x.device != eng.device:
            raise RuntimeError(f"da3mono_disparity: input on {x.device}, model on {eng.device}")
        B, _, H, W = x.shape
        lib = _hip.lib()
        out = torch.empty_like(x)
        ws = torch.empty(lib.nunif_hip_da3mono_workspace_bytes(B, H, W), dtype=torch.uint8, device=x.device)
        ranks = device_ranks(H * W, x.device)
        eng.call(lib.nunif_hip_da3mono_forward, eng.handle, ctypes.c_void_p(x.data_ptr()), B, H, W, ctypes.c_void_p(ranks.data_ptr()),
                 ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel())
        out = out.to(depth.dtype)
        return out if batch else out.squeeze(0)

    @staticmethod
    def extract_features(x, workspace=None):
        """x [1,H,W] or [B,1,H,W] -> [64] or [B,64]: minimum, 62 order statistics, maximum (:53-73), bit-equal to the sort.
        ``workspace`` (tests): a uint8 device tensor of at least ``nunif_hip_da3mono_features_workspace_bytes`` bytes."""
        x, batch = _maps(x, "da3mono_disparity.extract_features")
        B, _, H, W = x.shape
        lib = _hip.lib()
        out = torch.empty((B, FEAT_DIM), dtype=torch.float32, device=x.device)
        if workspace is None:
            workspace = torch.empty(lib.nunif_hip_da3mono_features_workspace_bytes(B, H, W), dtype=torch.uint8, device=x.device)
        ranks = device_ranks(H * W, x.device)
        with torch.cuda.device(x.device):
            _hip.check(lib.nunif_hip_da3mono_features(ctypes.c_void_p(x.data_ptr()), B, H, W, ctypes.c_void_p(ranks.data_ptr()),
                                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(workspace.data_ptr()),
                                                      workspace.numel(), _hip.current_stream_ptr(x.device)))
        return out if batch else out.squeeze(0)

    def load(self):
        pass
