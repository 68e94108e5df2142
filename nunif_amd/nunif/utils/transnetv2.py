"""TransNetV2 (shot boundary detection) on the HIP engine.

Mirrors ``nunif/utils/transnetv2.py`` (reference) ``TransNetV2`` :7-93: the constructor signature, the ``state_dict`` keys and
shapes (so ``transnetv2-pytorch-weights.pth`` loads unchanged), ``eval()`` / ``to(device)``, and ``forward(inputs)`` returning
``(one_hot, {"many_hot": ...})``.  The network is ``nunif_hip_transnetv2_forward`` (nunif_amd/csrc/transnetv2.hip): fp32
operands and accumulation, as the reference runs it (``shot_boundary_detection.py:42``).  Only the geometry that ``TransNetV2()``
builds (F=16, L=3, S=2, D=1024, both similarity branches, many-hot head, no mean pooling) exists as kernels.

``load()`` reads the released file from ``<model_dir>/checkpoints`` (the reference lets ``torch.hub`` fetch it); nothing is
downloaded here.
"""
import ctypes
import math
import os
from collections import OrderedDict

import torch

from ... import _hip
from ...engine import FlatWeightsMixin, HipEngine

WEIGHTS_FILE = "transnetv2-pytorch-weights.pth"
DILATIONS = (1, 2, 4, 8)
BN_EPS = 1e-3
LOOKUP = 101
HEAD_IN = 128 + 128 + 3 * 6 * 256


class OptionNotSupported(NotImplementedError, TypeError):
    """The reference spells this ``raise NotImplemented(...)``, which is a TypeError at run time; callers that catch either the
    intended or the actual exception keep working."""


def block_channels(F=16, L=3):
    """(input channels, F') of the L stacked blocks."""
    return [(3 if i == 0 else F * 2 ** (i - 1) * 4, F * 2 ** i) for i in range(L)]


def state_dict_shapes(F=16, L=3, S=2, D=1024):
    """Reference key -> shape, in the reference's own order."""
    shapes = OrderedDict()
    for b, (cin, f) in enumerate(block_channels(F, L)):
        for layer in range(S):
            c = cin if layer == 0 else 4 * f
            p = f"SDDCNN.{b}.DDCNN.{layer}."
            for d in DILATIONS:
                shapes[p + f"Conv3D_{d}.layers.0.weight"] = (2 * f, c, 1, 3, 3)
                shapes[p + f"Conv3D_{d}.layers.1.weight"] = (f, 2 * f, 3, 1, 1)
            for k in ("weight", "bias", "running_mean", "running_var"):
                shapes[p + "bn." + k] = (4 * f,)
            shapes[p + "bn.num_batches_tracked"] = ()
    feat = sum(f * 4 for _, f in block_channels(F, L))
    shapes["frame_sim_layer.projection.weight"] = (128, feat)
    shapes["frame_sim_layer.projection.bias"] = (128,)
    shapes["frame_sim_layer.fc.weight"] = (128, LOOKUP)
    shapes["frame_sim_layer.fc.bias"] = (128,)
    shapes["color_hist_layer.fc.weight"] = (128, LOOKUP)
    shapes["color_hist_layer.fc.bias"] = (128,)
    shapes["fc1.weight"] = (D, block_channels(F, L)[-1][1] * 4 * 3 * 6 + 256)
    shapes["fc1.bias"] = (D,)
    for head in ("cls_layer1", "cls_layer2"):
        shapes[head + ".weight"] = (1, D)
        shapes[head + ".bias"] = (1,)
    return shapes


def _init_weights():
    sd = OrderedDict()
    for key, shape in state_dict_shapes().items():
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.zeros((), dtype=torch.long)
        elif ".bn." in key:
            sd[key] = torch.ones(shape) if key.endswith(("bn.weight", "running_var")) else torch.zeros(shape)
        elif key.endswith(".bias"):
            sd[key] = torch.zeros(shape)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[key] = torch.randn(shape) * math.sqrt(1.0 / fan_in)
    return sd


def pack_weights(sd):
    """Reference state dict -> the packed fp32 tensors ``nunif_hip_transnetv2_create`` takes (layout: include/nunif_hip.h).
    BatchNorm3d (eps 1e-3, running statistics) is folded into the temporal kernels and a bias, in float64."""
    out = OrderedDict()
    for b, (cin, f) in enumerate(block_channels()):
        for layer in range(2):
            c = cin if layer == 0 else 4 * f
            p = f"SDDCNN.{b}.DDCNN.{layer}."
            bn = {k: sd[p + "bn." + k].double() for k in ("weight", "bias", "running_mean", "running_var")}
            scale = bn["weight"] / torch.sqrt(bn["running_var"] + BN_EPS)
            ws, wt = [], []
            for i, d in enumerate(DILATIONS):
                w0 = sd[p + f"Conv3D_{d}.layers.0.weight"].double()[:, :, 0]            # [2f, c, 3, 3]
                ws.append(w0.permute(2, 3, 1, 0).reshape(9 * c, 2 * f))
                w1 = sd[p + f"Conv3D_{d}.layers.1.weight"].double()[:, :, :, 0, 0]      # [f, 2f, 3]
                w1 = w1.permute(2, 1, 0).reshape(6 * f, f) * scale[i * f:(i + 1) * f]
                wt.append(torch.nn.functional.pad(w1, (0, max(f, 32) - f)))
            ws = torch.cat(ws, dim=1)
            kpad = -(-9 * c // 16) * 16
            out[f"b{b}.l{layer}.ws"] = torch.nn.functional.pad(ws, (0, 0, 0, kpad - 9 * c))
            out[f"b{b}.l{layer}.wt"] = torch.stack(wt)
            out[f"b{b}.l{layer}.bias"] = bn["bias"] - bn["running_mean"] * scale
    out["proj.wt"] = sd["frame_sim_layer.projection.weight"].t()
    out["proj.b"] = sd["frame_sim_layer.projection.bias"]
    out["sim.wt"] = sd["frame_sim_layer.fc.weight"].t()
    out["sim.b"] = sd["frame_sim_layer.fc.bias"]
    out["hist.wt"] = sd["color_hist_layer.fc.weight"].t()
    out["hist.b"] = sd["color_hist_layer.fc.bias"]
    out["fc1.wt"] = sd["fc1.weight"].t()
    out["fc1.b"] = sd["fc1.bias"]
    for i in (1, 2):
        out[f"cls{i}.w"] = sd[f"cls_layer{i}.weight"].reshape(-1)
        out[f"cls{i}.b"] = sd[f"cls_layer{i}.bias"]
    return OrderedDict((k, v.to(torch.float32).contiguous()) for k, v in out.items())


def weights_path(model_dir=None):
    from ...iw3.stereo_model_factory import default_model_dir
    return os.path.join(model_dir or default_model_dir(), "checkpoints", WEIGHTS_FILE)


class TransNetV2(FlatWeightsMixin, torch.nn.Module):
    def __init__(self,
                 F=16, L=3, S=2, D=1024,
                 use_many_hot_targets=True,
                 use_frame_similarity=True,
                 use_color_histograms=True,
                 use_mean_pooling=False,
                 dropout_rate=0.5,
                 use_convex_comb_reg=False,  # not supported
                 use_resnet_features=False,  # not supported
                 use_resnet_like_top=False,  # not supported
                 frame_similarity_on_last_layer=False):  # not supported
        super().__init__()
        if use_resnet_features or use_resnet_like_top or use_convex_comb_reg or frame_similarity_on_last_layer:
            raise OptionNotSupported("Some options not implemented in Pytorch version of Transnet!")
        if ((F, L, S, D) != (16, 3, 2, 1024) or not use_many_hot_targets or not use_frame_similarity
                or not use_color_histograms or use_mean_pooling):
            raise NotImplementedError(
                "the HIP engine builds TransNetV2 only in the geometry of TransNetV2(): F=16, L=3, S=2, D=1024, frame similarity, "
                "colour histograms and the many-hot head on, no mean pooling")
        self._setup_weights(_init_weights())
        self.eval()

    def _make_engine(self, device):
        return HipEngine(device, pack_weights(self._weights), "nunif_hip_transnetv2_create", "nunif_hip_transnetv2_destroy", 16,
                         label="TransNetV2")

    def load(self, map_location="cpu", model_dir=None):
        path = weights_path(model_dir)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found (no downloads here: copy the reference's {WEIGHTS_FILE} there, "
                                    "or pass model_dir=)")
        self.load_state_dict(torch.load(path, map_location=map_location, weights_only=True))
        return self

    def _run(self, inputs, sigmoid):
        if self.training:
            raise RuntimeError("the HIP engine is inference-only; call .eval()")
        assert torch.is_tensor(inputs) and inputs.dtype in {torch.float32, torch.float16}
        if inputs.ndim == 4 and inputs.shape[1:] == (3, 27, 48):
            inputs = inputs.unsqueeze(0)
        else:
            assert inputs.ndim == 5 and inputs.shape[2:] == (3, 27, 48), "incorrect input type and/or shape"
        eng = self.engine()
        dev = eng.device
        x = inputs.to(device=dev, dtype=torch.float32).contiguous()
        B, T = x.shape[:2]
        if T < 1 or B < 1:
            raise ValueError("TransNetV2 needs at least one frame")
        out = torch.empty((3 if sigmoid else 2, B, T), dtype=torch.float32, device=dev)
        eng.call(_hip.lib().nunif_hip_transnetv2_forward, eng.handle, ctypes.c_void_p(x.data_ptr()), B, T,
                 ctypes.c_void_p(out[0].data_ptr()), ctypes.c_void_p(out[1].data_ptr()),
                 ctypes.c_void_p(out[2].data_ptr()) if sigmoid else None)
        return out

    def forward(self, inputs):
        out = self._run(inputs, False)
        return out[0].unsqueeze(-1), {"many_hot": out[1].unsqueeze(-1)}

    @torch.inference_mode()
    def predict(self, inputs):
        """sigmoid(one_hot) as ``[B, T]`` (``shot_boundary_detection.py:44-45``), fused into the head kernel."""
        return self._run(inputs, True)[2]
