"""``--depth-model Any_V3_Mono`` / ``Any_V3_Mono_01`` on the HIP engine: everything ``iw3/depth_anything_v3_model.py`` (reference)
wraps around the Depth-Anything-3 mono backbone.

``_forward`` :27-58 keeps the reference's signature; its post-processing (sky mask and weight, the all-sky test, the shifted
reciprocal, the 0.99 quantile of ``raw_output``) is one launch group without a host synchronisation (``nunif_hip_da3_disparity``,
nunif_amd/csrc/da3_disparity.hip).  ``batch_infer`` :61-118 is the engine's ``batch_preprocess``, ``DepthAA``, ``dilate_edge`` and the
flip merge of ``depth_anything_model.py``.  The backbone is an external ``torch.hub`` net and is not restated: ``load_model`` takes it
from a local checkout (``NUNIF_DA3_HUB``) or as ``backbone=``, any callable that answers ``{"depth": [B,1?,H,W], "sky": ...}`` for a
``(B, 1, C, H, W)`` input, and never touches the network.

Divergence: with ``raw_output`` an image without one non-sky pixel makes the reference raise (``torch.quantile`` of an empty
tensor); the engine cannot stop the host and answers zeros for that image.
"""
import ctypes
import os
from os import path

import torch

from .. import _hip
from ..nunif.device import autocast
from .base_depth_model import BaseDepthModel
from .depth_anything_model import batch_preprocess
from .depth_scaler import EMAMinMaxScaler
from .dilation import dilate_edge, edge_dilation_is_enabled
from .stereo_model_factory import default_model_dir

HUB_ENV = "NUNIF_DA3_HUB"
DEPTH_AA_FILE = "iw3_depth_aa_20250530.pth"
SHIFT = 0.2                            # _forward :47

NAME_MAP = {
    "Any_V3_Mono": "da3mono-large",
    "Any_V3_Mono_01": "da3mono-large",
}
MODEL_FILES = {
    "Any_V3_Mono": path.join(default_model_dir(), "checkpoints", "da3mono-large.safetensors"),
    "Any_V3_Mono_01": path.join(default_model_dir(), "checkpoints", "da3mono-large.safetensors"),
}
AA_SUPPORTED_MODELS = {
    "Any_V3_Mono",
    "Any_V3_Mono_01",
}


def _maps(t, B, H, W, name):
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: tensor must live on a ROCm device (got {t.device}); there is no CPU fallback")
    return t.reshape(B, 1, H, W).to(torch.float32).contiguous()


def disparity_stage(depth, sky, sky_thresh=0.3, raw_output=False, shift=SHIFT, return_workspace=False):
    """depth, sky [B,H,W] or [B,1,H,W] -> [B,1,H,W]: ``_forward`` :33-56 for the whole batch."""
    B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    d, s = _maps(depth, B, H, W, "da3_disparity"), _maps(sky, B, H, W, "da3_disparity")
    lib = _hip.lib()
    out = torch.empty_like(d)
    ws = torch.empty(lib.nunif_hip_da3_disparity_workspace_bytes(B, H, W), dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        _hip.check(lib.nunif_hip_da3_disparity(ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(s.data_ptr()), B, H, W, float(sky_thresh),
                                               float(shift), 1 if raw_output else 0, ctypes.c_void_p(out.data_ptr()),
                                               ctypes.c_void_p(ws.data_ptr()), ws.numel(), _hip.current_stream_ptr(d.device)))
    return (out, ws) if return_workspace else out


def disparity_debug_stats(ws, B):
    """Tests only: (lower and upper order statistic and quantile [B,3], non-sky counts [B]) of the raw call that ran on ``ws``."""
    stats = torch.empty((B, 3), dtype=torch.float32, device=ws.device)
    counts = torch.empty((B,), dtype=torch.int32, device=ws.device)
    with torch.cuda.device(ws.device):
        _hip.check(_hip.lib().nunif_hip_da3_disparity_debug_stats(ctypes.c_void_p(ws.data_ptr()), B, ctypes.c_void_p(stats.data_ptr()),
                                                                  ctypes.c_void_p(counts.data_ptr()), _hip.current_stream_ptr(ws.device)))
    return stats, counts


def _forward(model, x, enable_amp, sky_thresh=0.3, raw_output=False):
    amp_dtype = torch.bfloat16 if (x.device.type == "cuda" and torch.cuda.is_bf16_supported()) else None
    with autocast(device=x.device, enabled=enable_amp, dtype=amp_dtype):
        out = model(x.unsqueeze(1))  # (B, S, C, H, W)
    depth, sky = out["depth"], out["sky"]
    disparity_model = getattr(model, "disparity_model", None)
    if disparity_model is not None and not raw_output:
        # the trained stage in place of the fixed shift: its own sky rule (depth == max), no sky map
        B, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
        return disparity_model(_maps(depth, B, H, W, "da3mono_disparity"))
    return disparity_stage(depth, sky, sky_thresh=sky_thresh, raw_output=raw_output)


@torch.inference_mode()
def batch_infer(model, im, flip_aug=True, low_vram=False, enable_amp=False,
                output_device="cpu", device=None, edge_dilation=2, depth_aa=None,
                limit_resolution=False,
                raw_output=False,
                **kwargs):
    device = device if device is not None else model.device
    if not torch.is_tensor(im):
        raise ValueError("batch_infer expects a CHW or BCHW float tensor in [0,1]")
    assert im.ndim == 3 or im.ndim == 4
    batch = im.ndim == 4
    x = (im if batch else im.unsqueeze(0)).to(device)
    x = batch_preprocess(x, model.prep_lower_bound, limit_resolution=limit_resolution)
    if not low_vram:
        if flip_aug:
            x = torch.cat([x, torch.flip(x, dims=[3])], dim=0)
        out = _forward(model, x, enable_amp, raw_output=raw_output)
    else:
        out = _forward(model, x, enable_amp, raw_output=raw_output)
        if flip_aug:
            out = torch.cat([out, _forward(model, torch.flip(x, dims=[3]), enable_amp, raw_output=raw_output)], dim=0)
    if depth_aa is not None:
        out = depth_aa.infer(out)
    if edge_dilation_is_enabled(edge_dilation):
        out = dilate_edge(out, edge_dilation) if not raw_output else -dilate_edge(-out, edge_dilation)
    if flip_aug:
        a, b = out.chunk(2, dim=0)
        out = (a + torch.flip(b, dims=[3])) * 0.5
    if not batch:
        assert out.shape[0] == 1
        out = out.squeeze(0)
    return out.to(output_device)


class DepthAnythingV3MonoModel(BaseDepthModel):
    def __init__(self, model_type):
        super().__init__(model_type)
        self.depth_aa = None
        self.raw_output = False

    def create_depth_scaler(self):
        if self.model_type == "Any_V3_Mono":
            # Max=1 scaling
            return EMAMinMaxScaler(decay=0, buffer_size=1, mode="max")
        elif self.model_type == "Any_V3_Mono_01":
            # Max=1 and Min=0 scaling
            return EMAMinMaxScaler(decay=0, buffer_size=1, mode="minmax")

    def load_model(self, model_type, resolution=None, device=None, raw_output=False, backbone=None, depth_aa=None,
                   disparity_model=None):
        """``backbone`` hands over the network (tests, a caller that holds the hub object); without it the hub entry point is loaded
        from the local checkout ``NUNIF_DA3_HUB`` names.  ``disparity_model``: a ``DA3MonoDisparity`` that replaces the fixed
        ``shift = 0.2`` stage.  Nothing here reaches the network."""
        self.depth_aa = depth_aa
        if depth_aa is None and model_type in AA_SUPPORTED_MODELS:
            p = path.join(default_model_dir(), "checkpoints", DEPTH_AA_FILE)
            if path.exists(p):                        # optional: only needed for infer(depth_aa=True)
                from ..nunif.models import load_model
                self.depth_aa = load_model(p, weights_only=True)[0].eval().to(device)
        if backbone is None:
            hub = os.getenv(HUB_ENV)
            if not hub or not path.exists(path.join(hub, "hubconf.py")):
                raise FileNotFoundError(f"{model_type}: the Depth-Anything-3 backbone is an external hub net; set {HUB_ENV} to a local "
                                        "checkout of nagadomi/Depth-Anything-3_iw3 (no downloads here) or pass backbone=")
            backbone = torch.hub.load(hub, "load_model", model_name=NAME_MAP[model_type], source="local", verbose=False,
                                      trust_repo=True)
        model = backbone
        model.prep_lower_bound = resolution or 392
        if model.prep_lower_bound % 14 != 0:
            # From GUI, 512 -> 518
            model.prep_lower_bound += (14 - model.prep_lower_bound % 14)
        model.device = device
        model.disparity_model = disparity_model
        self.raw_output = raw_output
        return model

    def infer(self, x, tta=False, low_vram=False, enable_amp=True, edge_dilation=0, depth_aa=False, **kwargs):
        if not torch.is_tensor(x):
            raise ValueError("infer expects a CHW or BCHW float tensor in [0,1]")
        if depth_aa and self.depth_aa is None:
            raise ValueError(f"depth_aa=True needs {DEPTH_AA_FILE} in the model directory (or load(depth_aa=model))")
        if x.device.type != "cuda":
            x = x.to(self.device)
        return batch_infer(
            self.model, x, flip_aug=tta, low_vram=low_vram,
            enable_amp=enable_amp,
            output_device=x.device,
            device=x.device,
            edge_dilation=edge_dilation,
            depth_aa=self.depth_aa if depth_aa else None,
            raw_output=self.raw_output,
            limit_resolution=self.limit_resolution,
        )

    @classmethod
    def get_name(cls):
        return "DepthAnythingV3Mono"

    @classmethod
    def has_checkpoint_file(cls, model_type):
        return cls.supported(model_type) and path.exists(MODEL_FILES[model_type])

    @classmethod
    def supported(cls, model_type):
        return model_type in MODEL_FILES

    @classmethod
    def get_model_path(cls, model_type):
        return MODEL_FILES[model_type]

    def is_metric(self):
        return False

    @classmethod
    def multi_gpu_supported(cls, model_type):
        return True

    @classmethod
    def force_update(cls):
        pass

    def infer_raw(self, *args, **kwargs):
        return batch_infer(self.model, *args, **kwargs)
