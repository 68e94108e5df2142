"""Film grain on the HIP engine: ``rgb_noise_like`` / ``apply_rgb_noise`` with the reference's signatures
(``nunif/utils/rgb_noise.py:5-39``), plus the lower-level calls the waifu2x video stream uses (``grain.hip``).

The noise comes from a counter-based generator (Philox-4x32-10) keyed by ``(seed, counter, element coordinates)``; it has the
reference's distribution but NOT torch's values for a given seed.  ``rgb_noise_like`` takes its seed from torch's default
generator (``torch.initial_seed()``) and numbers its calls, so ``torch.manual_seed(s)`` followed by the same sequence of calls
repeats a run.  There is no CPU path: CPU tensors raise.
"""
import ctypes

import torch

from ... import _hip

_MASK64 = (1 << 64) - 1


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _device_f32(t, name):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise RuntimeError(f"{name}: tensor must live on a ROCm device; there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: float32 expected, got {t.dtype}")
    return t.contiguous()


def _next_counter(device):
    """(seed, counter) of this call.  The seed is torch's (``torch.initial_seed()``); the call counter is kept in the device's
    default generator as its Philox offset, four per call: ``torch.manual_seed`` resets it — the same seed followed by the same
    calls repeats a run, inside one process too — and torch's own random calls in between move it on, never back."""
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    offset = gen.get_offset()
    gen.set_offset(offset + 4)
    return torch.initial_seed() & _MASK64, offset // 4


def generate(shape, device, level=2, seed=0, counter=0, component=0):
    """The generator itself: fp32 noise of ``shape`` ([3,H,W] or [B,3,H,W]) for ``(seed, counter)``.
    component 0: ``rgb_noise_like``'s result for ``level``; 1: the full-resolution term alone; 2: the upsampled half-resolution
    term alone; 3: the half-resolution grid itself (shape[..., H // 2, W // 2])."""
    shape = tuple(shape)
    assert len(shape) in (3, 4) and level in (1, 2) and component in (0, 1, 2, 3)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("rgb_noise: the generator runs on a ROCm device; there is no CPU fallback")
    h, w = shape[-2:]
    planes = 1
    for s in shape[:-2]:
        planes *= s
    out_shape = shape[:-2] + (h // 2, w // 2) if component == 3 else shape
    out = torch.empty(out_shape, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _hip.check(_hip.lib().nunif_hip_rgb_noise(_p(out), planes, h, w, level, component, seed & _MASK64, counter,
                                                  _hip.current_stream_ptr(device)))
    return out


def rgb_noise_like(base, level=2):
    assert level in {1, 2}
    base = _device_f32(base, "rgb_noise_like")
    assert base.ndim in (3, 4)
    seed, counter = _next_counter(base.device)
    return generate(base.shape, base.device, level=level, seed=seed, counter=counter)


def apply_rgb_noise(rgb, noise, strength=0.2,
                    gamma=2.2,
                    light_decay=True, light_decay_strength=0.8):
    assert 0 <= light_decay_strength and light_decay_strength <= 1
    rgb = _device_f32(rgb, "apply_rgb_noise")
    noise = _device_f32(noise, "apply_rgb_noise")
    if noise.shape != rgb.shape:
        noise = noise.expand_as(rgb).contiguous()
    out = torch.empty_like(rgb)
    with torch.cuda.device(rgb.device):
        _hip.check(_hip.lib().nunif_hip_apply_rgb_noise(_p(rgb), _p(noise), _p(out), rgb.numel(), float(strength), float(gamma),
                                                        1 if light_decay else 0, float(light_decay_strength),
                                                        _hip.current_stream_ptr(rgb.device)))
    return out


def blend_noise_buffer(buf, noise, speed, first):
    """``waifu2x/ui_utils.py:169-174`` in place: ``buf = noise`` when ``first`` else ``buf * (1 - speed) + noise * speed``."""
    assert buf.shape == noise.shape and buf.is_contiguous() and buf.dtype == torch.float32 and buf.device.type == "cuda"
    noise = _device_f32(noise, "blend_noise_buffer")
    with torch.cuda.device(buf.device):
        _hip.check(_hip.lib().nunif_hip_grain_blend(_p(buf), _p(noise), buf.numel(), float(speed), 1 if first else 0,
                                                    _hip.current_stream_ptr(buf.device)))
    return buf


def grain_video_step(rgb, noise_buffer, out, bits=8, level=2, seed=0, counter=0, speed=0.8, first=False, strength=0.2,
                     gamma=2.2, light_decay=True, light_decay_strength=0.8):
    """One frame of the video loop in one launch (``ui_utils.py:167-177``): draw the noise of ``(seed, counter)``, update
    ``noise_buffer`` [3,H,W] in place, apply the grain to ``rgb`` [3,H,W] and write the quantised HWC frame into ``out``
    (uint8, or int16 holding the uint16 bit pattern; a device tensor or a pinned host tensor)."""
    rgb = _device_f32(rgb, "grain_video_step")
    _, h, w = rgb.shape
    assert noise_buffer.shape == rgb.shape and noise_buffer.is_contiguous() and noise_buffer.dtype == torch.float32
    assert noise_buffer.device == rgb.device
    assert out.shape == (h, w, 3) and out.is_contiguous() and (out.device.type == "cuda" or out.is_pinned())
    assert out.dtype == (torch.uint8 if bits == 8 else torch.int16)
    with torch.cuda.device(rgb.device):
        _hip.check(_hip.lib().nunif_hip_grain_video_step(
            _p(rgb), _p(noise_buffer), _p(out), h, w, bits, level, seed & _MASK64, counter, float(speed), 1 if first else 0,
            float(strength), float(gamma), 1 if light_decay else 0, float(light_decay_strength),
            _hip.current_stream_ptr(rgb.device)))
    return out
