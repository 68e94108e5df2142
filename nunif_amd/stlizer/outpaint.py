"""The border step of stlizer's pass 4 for ``--border outpaint`` / ``expand_outpaint`` on the HIP engine.

:class:`OutpaintBorder` is ``stabilizer_callback`` of ``stlizer/multipass_pipeline.py`` (reference) from line 447 to 474, i.e.
everything after ``KU.apply_transform`` (and, for ``outpaint``, the crop of the padding): the NaN mask, the outpaint network and
the EMA frame buffer.  The reference's callback is a closure whose inner loop cannot be rebound, so this class is the engine-side
public form; under ``nunif_amd.install()`` the reference CLI gets the network on the engine (through the model registry) and keeps
its own torch loop for the buffer.

One call is two ``nunif_hip_outpaint_buffer_step`` launches around one ``infer``: no boolean-mask gather or scatter, no host
synchronisation.
"""
import ctypes

import torch

from .. import _hip


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def blend_weight(buffer_decay, fps):
    """``--buffer-decay`` -> the weight of the old buffer in the EMA (multipass_pipeline.py:456-458)."""
    d = (1.0 - buffer_decay) * (29.97 / float(fps))
    d = min(max(0.5, d), 1.0)
    return 1.0 - d


def buffer_step(frames, coarse=None, buffer=None, reset=None, decay=0.0):
    """``nunif_hip_outpaint_buffer_step``.  Without ``coarse``: ``(frames with NaN -> 0, isnan(frames[:, 0:1]) as uint8)``.  With
    ``coarse``: the EMA over the batch, ``buffer`` [3, H, W] updated in place, returns the composited, clamped frames."""
    if frames.device.type != "cuda":
        raise RuntimeError(f"buffer_step: the HIP engine needs a ROCm device tensor (got {frames.device}); there is no CPU fallback")
    f = frames.to(torch.float32).contiguous()
    B, C, H, W = f.shape
    assert C == 3
    out = torch.empty_like(f)
    mask = None
    if coarse is None:
        mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=f.device)
    else:
        coarse = coarse.to(device=f.device, dtype=torch.float32).contiguous()
        assert coarse.shape == f.shape and buffer.shape == f.shape[1:] and buffer.dtype == torch.float32 and buffer.is_contiguous()
        reset = torch.as_tensor(reset, dtype=torch.uint8).to(f.device).contiguous()
        assert reset.shape == (B,)
    with torch.cuda.device(f.device):
        _hip.check(_hip.lib().nunif_hip_outpaint_buffer_step(_ptr(f), _ptr(coarse), _ptr(buffer), _ptr(reset), float(decay), B, H, W,
                                                             _ptr(out), _ptr(mask), _hip.current_stream_ptr(f.device)))
    return out if coarse is not None else (out, mask)


class OutpaintBorder:
    """``border = OutpaintBorder(model, buffer_decay, fps)``; ``frames = border(z, scene_weight)`` for every batch ``z`` [B, 3, H, W]
    that ``apply_transform(..., padding_mode="border")`` made from NaN-padded frames; ``scene_weight`` holds the batch's B values
    of pass 3.  ``buffer_decay`` is the raw ``--buffer-decay``: above 0 the frames come from the EMA buffer (:455-471), otherwise
    from ``infer(composite=True)`` (:473)."""

    def __init__(self, model, buffer_decay, fps, max_size=640):
        self.model = model
        self.raw_decay = float(buffer_decay)
        self.decay = blend_weight(self.raw_decay, fps) if self.raw_decay > 0.0 else 0.0
        self.max_size = max_size
        self.buffer = None

    def reset(self):
        self.buffer = None

    @torch.inference_mode()
    def __call__(self, z, scene_weight=None):
        zeroed, mask = buffer_step(z)
        if not self.raw_decay > 0.0:
            return self.model.infer(zeroed, mask, max_size=self.max_size, composite=True).to(z.dtype)
        B = z.shape[0]
        sw = [1.0] * B if scene_weight is None else [float(v) for v in scene_weight]
        assert len(sw) == B
        reset = [w < 0.01 for w in sw]
        if self.buffer is None:
            self.buffer = torch.empty(tuple(z.shape[1:]), dtype=torch.float32, device=z.device)
            reset[0] = True
        coarse = self.model.infer(zeroed, mask, max_size=self.max_size, composite=False)
        return buffer_step(z, coarse, self.buffer, reset, self.decay).to(z.dtype)
