"""``--depth-model ZoeD_Any_N / ZoeD_Any_K`` on the HIP engine.  Mirrors ``iw3/zoedepth_model.py``: the name tables :12-20,
``_forward`` :23-27, ``batch_preprocess`` :30-85, ``batch_infer`` :88-148 and ``ZoeDepthModel`` :151-245 — for the two names
whose backbone is Depth-Anything V1 ViT-L (``DepthAnythingMetricDepth`` of the hub repository ``nagadomi/Depth-Anything_iw3``).
The BEiT names (``ZoeD_N / ZoeD_K / ZoeD_NK``) are not carried: ``supported`` refuses them and the factory raises ``ValueError``.

The network is not in the reference tree.  Encoder and DPT neck are the engine's Depth-Anything (``depth_anything.hip``,
``nunif_hip_depth_anything_forward_features`` leaves the six maps ZoeDepth's ``DepthAnythingCore`` hooks); the metric-bins head is
``zoedepth_head.hip``, pinned in float64 against HuggingFace ``ZoeDepthMetricDepthEstimationHead`` (tests/zoedepth_ref.py).

Checkpoint keys.  The engine takes ``pretrained.*`` / ``depth_head.*`` (Depth-Anything layout) and ``metric_head.*`` (HuggingFace
names, checked against the live class).  ``translate_state_dict`` also takes the PUBLISHED ZoeDepth names; the installed
``transformers`` ships no ``convert_zoedepth_to_hf.py``, so that table is restated from the published module layout
(``_net.0`` / ``_net.2`` of the Sequential MLPs) and is UNVERIFIED — see COVERAGE.md.

``attractor_alpha`` is 1000 as in the published Depth-Anything metric configuration.  (HuggingFace's attractor layer calls
``inv_attractor`` with its defaults, alpha 300, whatever the configuration says: the float64 pin uses 300 for that reason.)
"""
import ctypes
import os
import re

import torch

from .. import _hip
from ..engine import HipEngine
from . import _ops
from .base_depth_model import BaseDepthModel
from .dilation import dilate_edge, edge_dilation_is_enabled
from .stereo_model_factory import default_model_dir

MODEL_FILE_NAMES = {
    "ZoeD_Any_N": "depth_anything_metric_depth_indoor.pt",
    "ZoeD_Any_K": "depth_anything_metric_depth_outdoor.pt",
}
DEPTH_ANYTHING_MODELS = {"ZoeD_Any_N": "indoor", "ZoeD_Any_K": "outdoor"}
HEAD_PREFIX = "metric_head."
ATTRACTOR_ALPHA, MIN_TEMP, MAX_TEMP = 1000.0, 0.0212, 50.0

# published ZoeDepth name -> engine name (regular expressions, first match wins); UNVERIFIED against the released files
PUBLISHED_KEY_TABLE = (
    (r"^core\.core\.(pretrained\..*)$", r"\1"),
    (r"^core\.core\.(depth_head\..*)$", r"\1"),
    (r"^conv2\.(weight|bias)$", HEAD_PREFIX + r"conv2.\1"),
    (r"^(seed_bin_regressor|seed_projector)\._net\.0\.(weight|bias)$", HEAD_PREFIX + r"\1.conv1.\2"),
    (r"^(seed_bin_regressor|seed_projector)\._net\.2\.(weight|bias)$", HEAD_PREFIX + r"\1.conv2.\2"),
    (r"^(projectors|attractors)\.(\d)\._net\.0\.(weight|bias)$", HEAD_PREFIX + r"\1.\2.conv1.\3"),
    (r"^(projectors|attractors)\.(\d)\._net\.2\.(weight|bias)$", HEAD_PREFIX + r"\1.\2.conv2.\3"),
    (r"^(conditional_log_binomial\.mlp\.[02]\.(?:weight|bias))$", HEAD_PREFIX + r"\1"),
)


def translate_state_dict(state_dict):
    """Published ZoeDepth names -> the engine's; a dict already in the engine's layout passes unchanged.  A ``{"model": ...}``
    wrapper (the released ``.pt`` files) is opened."""
    if "model" in state_dict and isinstance(state_dict["model"], dict):
        state_dict = state_dict["model"]
    out = {}
    for k, v in state_dict.items():
        if k.startswith(("pretrained.", "depth_head.", HEAD_PREFIX)):
            out[k] = v
            continue
        for pat, rep in PUBLISHED_KEY_TABLE:
            if re.match(pat, k):
                out[re.sub(pat, rep, k)] = v
                break
    return out


def preprocess_geometry(height, width, h_height=392, v_height=518, ensure_multiple_of=14):
    """The integer part of ``batch_preprocess`` :32-72 -> (frame_h, frame_w, pad_h, pad_w)."""
    mod = ensure_multiple_of
    target_height = h_height if width > height else v_height
    if target_height < height:
        new_h = target_height
        new_w = int(new_h / height * width)
        if new_w % mod != 0:
            new_w += (mod - new_w % mod)
        if new_h % mod != 0:
            new_h += (mod - new_h % mod)
    else:
        new_h, new_w = height, width
        if new_w % mod != 0:
            new_w -= new_w % mod
        if new_h % mod != 0:
            new_h -= new_h % mod
    pad_src_h = int((height * 0.5) ** 0.5 * 3)
    pad_src_w = int((width * 0.5) ** 0.5 * 3)
    pad_scale_h = pad_src_h / (height + pad_src_h * 2)
    pad_scale_w = pad_src_w / (width + pad_src_w * 2)
    if new_h > new_w:
        pad_h = round(new_h * pad_scale_h)
        frame_h = new_h - pad_h * 2
        frame_w = int(width * (frame_h / height))
        frame_w += frame_w % 2
        pad_w = (new_h - frame_w) // 2
    else:
        pad_h = round(new_h * pad_scale_h)
        pad_w = round(new_w * pad_scale_w)
        frame_h = new_h - pad_h * 2
        frame_w = new_w - pad_w * 2
    return frame_h, frame_w, pad_h, pad_w


def resolution_heights(resolution=None, mod=14):
    """The ``--resolution`` rule of ``load_model`` :190-199 -> (prep_h_height, prep_v_height): 392 / 518 without one, else the
    resolution rounded up to a multiple of 14 for both."""
    if resolution is None:
        return 392, 518
    if resolution % mod != 0:
        resolution += (mod - resolution % mod)
    return resolution, resolution


def pad_normalize(x, pad_w, pad_h):
    """``reflection_pad2d_loop(x, [pad_w, pad_w, pad_h, pad_h])`` + ``clamp_(0, 1)`` + ``(x - 0.5) / 0.5`` in one kernel."""
    x = _ops._cuda_f32(x, "zoedepth pad_normalize")
    b, c, h, w = x.shape
    y = torch.empty((b, c, h + 2 * pad_h, w + 2 * pad_w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _hip.check(_hip.lib().nunif_hip_zoedepth_pad_normalize(_ops._p(x), _ops._p(y), b * c, h, w, pad_w, pad_w, pad_h, pad_h,
                                                               _hip.current_stream_ptr(x.device)))
    return y


def batch_preprocess(x, h_height=392, v_height=518, ensure_multiple_of=14):
    """x: BCHW float32 0-1 on the device -> (normalised padded batch, pad_h, pad_w)."""
    frame_h, frame_w, pad_h, pad_w = preprocess_geometry(x.shape[2], x.shape[3], h_height, v_height, ensure_multiple_of)
    x = _ops.resize_aa(x, (frame_h, frame_w), mode="bilinear", align_corners=False)
    return pad_normalize(x, pad_w, pad_h), pad_h, pad_w


class HipZoeDepthHead(HipEngine):
    """ZoeDepth's metric-bins head (``nunif_hip_zoedepth_head_*``) on the six maps of a ``_hip.DaFeatures``."""

    def __init__(self, head_state_dict, device="cuda:0", alpha=ATTRACTOR_ALPHA, min_temp=MIN_TEMP, max_temp=MAX_TEMP):
        super().__init__(device, head_state_dict, "nunif_hip_zoedepth_head_create", "nunif_hip_zoedepth_head_destroy",
                         ctypes.c_float(alpha), ctypes.c_float(min_temp), ctypes.c_float(max_temp), label="ZoeDepth head")

    def features_from_maps(self, outconv, bottleneck, blocks):
        """NCHW maps (any float dtype) -> (``_hip.DaFeatures``, the NHWC fp16 device tensors it points into: keep them alive)."""
        keep = [t.to(self.device).permute(0, 2, 3, 1).contiguous().half() for t in (outconv, bottleneck, *blocks)]
        f = _hip.DaFeatures()
        f.outconv, f.bottleneck = keep[0].data_ptr(), keep[1].data_ptr()
        f.bh, f.bw, f.channels = keep[1].shape[1], keep[1].shape[2], keep[1].shape[3]
        for i, t in enumerate(keep[2:]):
            f.blocks[i], f.rh[i], f.rw[i] = t.data_ptr(), t.shape[1], t.shape[2]
        return f, keep

    @torch.inference_mode()
    def forward(self, feats, rel):
        """rel: the relative depth [B,h,w] fp32 on the device -> nan_to_num(metric depth) [B,h,w]."""
        rel = rel.to(device=self.device, dtype=torch.float32).contiguous()
        b, h, w = rel.shape
        out = torch.empty_like(rel)
        self.call(_hip.lib().nunif_hip_zoedepth_head_forward, self.handle, ctypes.byref(feats), ctypes.c_void_p(rel.data_ptr()),
                  ctypes.c_void_p(out.data_ptr()), b, h, w)
        return out

    def debug_taps(self):
        """The bin centres of the last forward: [seed, after attractor 0 .. 3], each [B,64,h,w] fp32."""
        taps = []
        for i in range(5):
            dims = (ctypes.c_int32 * 3)()
            self.call(_hip.lib().nunif_hip_zoedepth_head_debug_taps, self.handle, i, None, dims)
            t = torch.empty((dims[0], dims[1], dims[2], 64), dtype=torch.float32, device=self.device)
            self.call(_hip.lib().nunif_hip_zoedepth_head_debug_taps, self.handle, i, ctypes.c_void_p(t.data_ptr()), None)
            taps.append(t.permute(0, 3, 1, 2).contiguous())
        return taps


class HipZoeDepthAny:
    """Depth-Anything V1 core + ZoeDepth metric-bins head: ``model(x[B,3,h,w]) -> nan_to_num(metric_depth) [B,h,w]``."""

    def __init__(self, state_dict, device="cuda:0", alpha=ATTRACTOR_ALPHA, min_temp=MIN_TEMP, max_temp=MAX_TEMP):
        from .depth_anything_v2 import HipDepthAnythingV2
        core = {k: v for k, v in state_dict.items() if k.startswith(("pretrained.", "depth_head."))}
        head = {k[len(HEAD_PREFIX):]: v for k, v in state_dict.items() if k.startswith(HEAD_PREFIX)}
        if not core or not head:
            raise ValueError("ZoeD_Any checkpoint: expected pretrained.* / depth_head.* / metric_head.* tensors")
        n_blocks = sum(1 for k in core if k.startswith("pretrained.blocks.") and k.endswith(".attn.qkv.weight"))
        # DPT_DINOv2 (Depth-Anything V1): get_intermediate_layers(x, 4) = the last four blocks
        self.core = HipDepthAnythingV2(core, device, taps=tuple(range(n_blocks - 4, n_blocks)))
        self.device = self.core.device
        self.head = HipZoeDepthHead(head, self.device, alpha, min_temp, max_temp)
        self.prep_mod, self.prep_h_height, self.prep_v_height = 14, 392, 518

    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def forward_features(self, x):
        """-> (relative depth [B,h,w], ``_hip.DaFeatures`` into the core's workspace: valid until its next call)."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        b, c, h, w = x.shape
        if c != 3 or h % 14 or w % 14:
            raise ValueError(f"expected [B,3,h,w] with h, w multiples of 14, got {tuple(x.shape)}")
        pos = self.core._pos(h // 14, w // 14)
        rel = torch.empty((b, h, w), dtype=torch.float32, device=self.device)
        feats = _hip.DaFeatures()
        self.core.call(_hip.lib().nunif_hip_depth_anything_forward_features, self.core.handle, ctypes.c_void_p(x.data_ptr()),
                       ctypes.c_void_p(pos.data_ptr()), ctypes.c_void_p(rel.data_ptr()), b, h, w, ctypes.byref(feats))
        return rel, feats

    @torch.inference_mode()
    def __call__(self, x):
        rel, feats = self.forward_features(x)
        return self.head.forward(feats, rel)


@torch.inference_mode()
def batch_infer(model, im, flip_aug=True, low_vram=False, enable_amp=False, output_device=None, device=None,
                edge_dilation=0, **kwargs):
    """``batch_infer`` :88-148.  ``low_vram`` / ``enable_amp`` are accepted and have nothing to switch on the engine.
    ``output_device=None`` (the default) leaves the result on the engine's device — the convention of this package's depth models
    (``depth_anything_model.batch_infer``, ``DepthAnythingModel.infer``): the frame pipeline consumes the depth there; the
    reference defaults to "cpu".  Pass ``output_device="cpu"`` for the reference's default."""
    device = device if device is not None else model.device
    if not torch.is_tensor(im):
        raise ValueError("batch_infer expects a CHW or BCHW float tensor in [0,1]")
    assert im.ndim == 3 or im.ndim == 4
    batch = im.ndim == 4
    x = (im if batch else im.unsqueeze(0)).to(device)
    x, pad_h, pad_w = batch_preprocess(x, h_height=model.prep_h_height, v_height=model.prep_v_height,
                                       ensure_multiple_of=model.prep_mod)
    if flip_aug:
        x = torch.cat([x, torch.flip(x, dims=[3])], dim=0)
    out = model(x).unsqueeze(1)                                        # nan_to_num is the head kernel's last step
    out = out[:, :, pad_h:out.shape[2] - pad_h, pad_w:out.shape[3] - pad_w]
    if edge_dilation_is_enabled(edge_dilation):
        out = dilate_edge(-out, edge_dilation)                         # :124-127: dilate_edge works in negative space
    else:
        out = -out
    if flip_aug:
        a, b = out.chunk(2, dim=0)
        out = (a + torch.flip(b, dims=[3])) * 0.5
    z = out if batch else out.squeeze(0)
    return z if output_device is None else z.to(output_device)


class ZoeDepthModel(BaseDepthModel):
    model_dir = None                    # None: default_model_dir()

    def __init__(self, model_type):
        super().__init__(model_type)

    @classmethod
    def _path(cls, model_type):
        return os.path.join(cls.model_dir or default_model_dir(), "checkpoints", MODEL_FILE_NAMES[model_type])

    def load_model(self, model_type, resolution=None, device=None, state_dict=None, **kwargs):
        """``state_dict`` lets a caller hand over weights it already holds (tests, tools)."""
        if model_type not in MODEL_FILE_NAMES:
            raise NotImplementedError(f"{model_type}: not a ZoeD_Any name ({sorted(MODEL_FILE_NAMES)})")
        if state_dict is None:
            p = self._path(model_type)
            if not os.path.exists(p):
                raise FileNotFoundError(f"{p} not found (no downloads here: copy the published checkpoint there)")
            state_dict = torch.load(p, map_location="cpu", weights_only=True)
        model = HipZoeDepthAny(translate_state_dict(state_dict), device)
        model.prep_h_height, model.prep_v_height = resolution_heights(resolution, model.prep_mod)
        return model

    def infer(self, x, tta=False, low_vram=False, enable_amp=True, edge_dilation=0, **kwargs):
        """The result is on the device of ``x`` (reference :211-212), a host tensor included: it is moved to the engine and the
        depth comes back to the host."""
        if not torch.is_tensor(x):
            raise ValueError("infer expects a CHW or BCHW float tensor in [0,1]")
        out_device = x.device
        if x.device.type != "cuda":
            x = x.to(self.device)
        return batch_infer(self.model, x, flip_aug=tta, low_vram=low_vram, enable_amp=enable_amp, output_device=out_device,
                           device=x.device, edge_dilation=edge_dilation)

    @classmethod
    def get_name(cls):
        return "ZoeDepth"

    @classmethod
    def has_checkpoint_file(cls, model_type="ZoeD_N"):
        return cls.supported(model_type) and os.path.exists(cls._path(model_type))

    @classmethod
    def supported(cls, model_type="ZoeD_N"):
        return model_type in MODEL_FILE_NAMES

    @classmethod
    def get_model_path(cls, model_type):
        return cls._path(model_type)

    def is_metric(self):
        return True

    @classmethod
    def multi_gpu_supported(cls, model_type):
        return model_type not in {"ZoeD_Any_N", "ZoeD_Any_K"}

    @classmethod
    def force_update(cls):
        pass

    def infer_raw(self, *args, **kwargs):
        return batch_infer(self.model, *args, **kwargs)
