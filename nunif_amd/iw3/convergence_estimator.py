"""``--convergence-mode sod_v1``: the per-frame convergence estimator on the HIP engine.

Mirrors ``iw3/convergence_estimator.py`` (reference) ``ConvergenceEstimator`` :11-84: the constructor, ``reset``,
``__call__(rgb, depth, reset_pts=None)`` and the static ``depth_position_from_ratio``.  The saliency net is
``nunif_amd.iw3.models.sod_v1.SODV1``; the masked quantiles with the rule of :41-59 are ONE launch for the batch
(``nunif_hip_sod_v1_depth_position``: no boolean indexing, no host read) and the EMA across frames :69-82 is one small launch on a
device state (``nunif_hip_sod_v1_ema``).  The result is ``[B,1,1,1]`` fp32 on the device, the convergence tensor every warp of
``nunif_amd.iw3.utils.apply_divergence`` reads per frame.

The reference fetches its checkpoint by URL; here the same file name is looked up in the model directory
(``stereo_model_factory.resolve``).  ``state_dict=`` builds the net from a state dict instead (tests).
"""
import ctypes

import torch

from .. import _hip
from ..nunif.device import create_device
from ..nunif.models import load_model
from .models.sod_v1 import SODV1
from .stereo_model_factory import resolve

SOD_FILE = "iw3_sod_v1_20260125.pth"


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class ConvergenceEstimator():
    def __init__(self, convergence, device_id, enable_ema=False, decay=0.9, compile=False, state_dict=None, model_dir=None):
        self.device = create_device(device_id)
        if state_dict is not None:
            self.model = SODV1()
            self.model.load_state_dict(state_dict)
            self.model = self.model.to(self.device)
        else:
            self.model, _ = load_model(resolve(SOD_FILE, model_dir), device_ids=[device_id], weights_only=True)
        self.model = self.model.eval().fuse().compile(mode=compile)
        self.convergence = convergence
        self.enable_ema = enable_ema
        self.decay = decay
        self._state = None                 # device [2]: the EMA and whether it holds a value (convergence_ema of the reference)

    @property
    def convergence_ema(self):
        if self._state is None:
            return None
        ema, has = self._state.tolist()    # a host read, for inspection only; __call__ never takes it
        return torch.tensor(ema, device=self.device).reshape(1, 1, 1) if has else None

    def reset(self, enable_ema=None, decay=None):
        if enable_ema is not None:
            self.enable_ema = enable_ema
        if decay is not None:
            self.decay = decay
        self._state = None

    @staticmethod
    def depth_position_from_ratio(saliency_map, depth, pos):
        if saliency_map.device.type != "cuda":
            raise RuntimeError("depth_position_from_ratio: tensors must live on a ROCm device; there is no CPU fallback")
        B = depth.shape[0]
        sal = saliency_map.detach().to(torch.float32).reshape(B, -1).contiguous()
        d = depth.detach().to(device=sal.device, dtype=torch.float32).reshape(B, -1).contiguous()
        assert sal.shape == d.shape
        out = torch.empty((B,), dtype=torch.float32, device=sal.device)
        with torch.cuda.device(sal.device):
            _hip.check(_hip.lib().nunif_hip_sod_v1_depth_position(_p(sal), _p(d), B, sal.shape[1], float(pos), _p(out),
                                                                  _hip.current_stream_ptr(sal.device)))
        return out.reshape(B, 1, 1, 1)

    def __call__(self, rgb, depth, reset_pts=None):
        rgb = rgb.to(self.device)
        depth = depth.to(self.device)
        with torch.inference_mode():
            saliency_map, depth_scaled = self.model.infer(rgb, depth)
            z_pos = self.depth_position_from_ratio(saliency_map, depth_scaled, self.convergence)
            if self.enable_ema:
                B = z_pos.shape[0]
                reset_pts = reset_pts if reset_pts is not None else [False] * B
                if self._state is None:
                    self._state = torch.zeros((2,), dtype=torch.float32, device=self.device)
                out = torch.empty_like(z_pos)
                zf, of = z_pos.reshape(-1), out.reshape(-1)
                with torch.cuda.device(self.device):
                    for i0 in range(0, B, 64):
                        n = min(64, B - i0)
                        mask = sum(1 << i for i in range(n) if reset_pts[i0 + i])
                        _hip.check(_hip.lib().nunif_hip_sod_v1_ema(_p(zf[i0:]), _p(of[i0:]), n, _p(self._state), float(self.decay),
                                                                   mask, _hip.current_stream_ptr(self.device)))
                z_pos = out
        return z_pos
