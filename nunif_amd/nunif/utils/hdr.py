"""HDR (BT.2020, PQ / HLG) -> SDR (bt709 / bt601) tone mapping on the HIP engine (nunif_amd/csrc/hdr.hip): what the reference's
``hdr2sdr`` (``nunif/utils/video.py:309-416``) computes between its ``to_ndarray`` and its ``from_ndarray``, in one launch.

The rgb48 frame is a device tensor or a PINNED host tensor (read zero-copy); the result is one of three forms:

``u16``    HWC, the uint16 pattern the reference's function returns (``:398``), device or pinned host memory;
``chw``    CHW fp32 ``float(u16) / 65535``: what ``VU.to_tensor`` (``:218-223``) makes of the reference's frame — the model's input;
``debug``  HWC fp32, the value before ``* 65535`` (tests).

An HDR source that enters as the decoder's planes (``yuv420p10le``, BT.2020) takes ``hdr2sdr_planes`` / ``hdr_yuv_entry``
(nunif_amd/csrc/hdr_planes.hip): the plane gather of ``pixfmt.yuv_to_tensor`` and the map in one launch, bit-equal to
``pixfmt.yuv_to_tensor(..., frame_out=rgb48)`` followed by ``hdr2sdr_tensor(rgb48, ...)`` without the rgb48 frame.  This is the
engine-side API's entry (``FrameRing``, ``Waifu2xVideoStream``, ``PipelineOps``); the installed ``process_video`` route keeps
calling ``hdr2sdr(av_frame, ...)``.

There is no CPU fallback: a frame that is neither on a ROCm device nor pinned raises.
"""
import ctypes

import torch

from ... import _hip
from . import pixfmt

MAX_DIM = 8192
COLOR_TRC_SMPTE2084, COLOR_TRC_ARIB_STD_B67 = 16, 18             # video.py:24-25
COLORSPACES = {"bt709": 709, "bt601": 601}
FORMS = {"u16": 0, "chw": 1, "debug": 2}


def _params(color_trc, pq_exposure, pq_white_point, hlg_exposure, hlg_white_point, hlg_saturation_gain):
    if color_trc == COLOR_TRC_SMPTE2084:
        return _hip.Hdr2SdrParams(float(pq_exposure), float(pq_white_point), float(hlg_saturation_gain))
    return _hip.Hdr2SdrParams(float(hlg_exposure), float(hlg_white_point), float(hlg_saturation_gain))


def _check_names(color_trc, output_colorspace):
    if output_colorspace not in COLORSPACES:
        raise ValueError(f"output_colorspace must be 'bt709' or 'bt601', got {output_colorspace!r}")
    if color_trc not in (COLOR_TRC_SMPTE2084, COLOR_TRC_ARIB_STD_B67):
        raise ValueError(f"color_trc must be {COLOR_TRC_SMPTE2084} (SMPTE 2084) or {COLOR_TRC_ARIB_STD_B67} (ARIB STD-B67), "
                         f"got {color_trc!r}")


def constants(color_trc, output_colorspace, pq_exposure=110.0, pq_white_point=5.0,
              hlg_exposure=1.2, hlg_white_point=0.8, hlg_saturation_gain=0.9):
    """(matrix as 9 floats row major, hable_map(white point)): the kernel's fp32 arguments.  Host only."""
    _check_names(color_trc, output_colorspace)
    p = _params(color_trc, pq_exposure, pq_white_point, hlg_exposure, hlg_white_point, hlg_saturation_gain)
    matrix, white = (ctypes.c_float * 9)(), ctypes.c_float()
    _hip.check(_hip.lib().nunif_hip_hdr2sdr_constants(int(color_trc), COLORSPACES[output_colorspace], ctypes.byref(p), matrix,
                                                      ctypes.byref(white)))
    return list(matrix), white.value


def _on_device_or_pinned(t, device, what):
    if t.device.type == "cuda":
        return t.device
    if not (t.is_pinned() and device is not None):
        raise RuntimeError(f"hdr2sdr_tensor: {what} must live on a ROCm device or in pinned host memory (with device=...); "
                           "there is no CPU fallback")
    return torch.device(device)


def hdr2sdr_tensor(rgb48, color_trc, output_colorspace, pq_exposure=110.0, pq_white_point=5.0,
                   hlg_exposure=1.2, hlg_white_point=0.8, hlg_saturation_gain=0.9, form="u16", out=None, device=None):
    """``rgb48`` [H, W, 3] int16 (the uint16 bit pattern, as the rest of the frame edge holds it) or uint16 -> the tone-mapped frame.
    ``out``: the destination (device, or pinned host memory for the ``u16`` form); by default a new tensor on the device."""
    _check_names(color_trc, output_colorspace)
    if form not in FORMS:
        raise ValueError(f"form must be one of {sorted(FORMS)}, got {form!r}")
    if not isinstance(rgb48, torch.Tensor) or rgb48.dtype not in (torch.int16, torch.uint16):
        raise ValueError(f"hdr2sdr_tensor needs an rgb48 frame as an int16 / uint16 tensor, got {getattr(rgb48, 'dtype', type(rgb48))}")
    if rgb48.dim() != 3 or rgb48.shape[2] != 3 or not rgb48.is_contiguous():
        raise ValueError(f"hdr2sdr_tensor needs a contiguous [H, W, 3] frame, got {tuple(rgb48.shape)}")
    h, w, _ = rgb48.shape
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f"a frame of {h} x {w} is outside H, W <= {MAX_DIM}")
    dev = _on_device_or_pinned(rgb48, device, "the frame")
    shape, dtype = ((h, w, 3), torch.int16) if form == "u16" else ((3, h, w), torch.float32) if form == "chw" else \
        ((h, w, 3), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    else:
        if _on_device_or_pinned(out, dev, "out") != dev:
            raise RuntimeError(f"hdr2sdr_tensor: out is on {out.device}, the frame on {dev}")
        if tuple(out.shape) != shape or not out.is_contiguous() or \
                out.dtype not in ((torch.int16, torch.uint16) if form == "u16" else (torch.float32,)):
            raise ValueError(f"hdr2sdr_tensor: out must be a contiguous {shape} {dtype} tensor for form {form!r}")
    p = _params(color_trc, pq_exposure, pq_white_point, hlg_exposure, hlg_white_point, hlg_saturation_gain)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().nunif_hip_hdr2sdr(ctypes.c_void_p(rgb48.data_ptr()), ctypes.c_void_p(out.data_ptr()), h, w,
                                                int(color_trc), COLORSPACES[output_colorspace], ctypes.byref(p), FORMS[form],
                                                _hip.current_stream_ptr(dev)))
    return out


def hdr_entry(color_trc, output_colorspace, **params):
    """An ``enter_fn(hwc, device=...)`` for :class:`nunif_amd.frame_ring.FrameRing` (with ``in_bits=16``): the rgb48 frame in the
    ring's pinned buffer arrives at ``process_fn`` as the tone-mapped CHW fp32 tensor — one PCIe crossing, one kernel."""
    _check_names(color_trc, output_colorspace)
    constants(color_trc, output_colorspace, **params)              # a wrong parameter name fails here, not on the first frame

    def enter(hwc, device=None):
        return hdr2sdr_tensor(hwc, color_trc, output_colorspace, form="chw", device=device, **params)
    enter.color_trc, enter.output_colorspace, enter.params = color_trc, output_colorspace, dict(params)
    return enter


PLANES_FORMAT, PLANES_MATRIX = "yuv420p10le", "bt2020"          # the one planar form an HDR source has (video.py:318)
_DEFAULTS = dict(pq_exposure=110.0, pq_white_point=5.0, hlg_exposure=1.2, hlg_white_point=0.8, hlg_saturation_gain=0.9)


def _known(params):
    unknown = sorted(set(params) - set(_DEFAULTS))
    if unknown:
        raise TypeError(f"unknown tone-mapping parameter(s) {unknown}; the parameters are {sorted(_DEFAULTS)}")
    return params


def hdr2sdr_planes(planes, layout, full_range, color_trc, output_colorspace, *, form="chw", out=None, device=None, **params):
    """The planes of one HDR frame (flat uint8 tensor in ``layout``, device or pinned; ``yuv420p10le``, BT.2020 by definition) ->
    the tone-mapped frame in ``form``, in one launch.  ``params``: ``pq_exposure`` ... ``hlg_saturation_gain`` as for
    :func:`hdr2sdr_tensor`; ``out`` as there."""
    _check_names(color_trc, output_colorspace)
    if form not in FORMS:
        raise ValueError(f"form must be one of {sorted(FORMS)}, got {form!r}")
    if not isinstance(layout, pixfmt.PlaneLayout) or layout.format != PLANES_FORMAT:
        raise ValueError(f"hdr2sdr_planes needs a PlaneLayout of format {PLANES_FORMAT!r}, got "
                         f"{getattr(layout, 'format', layout)!r}")
    pixfmt._check_buffer(planes, layout, "planes")
    p = _params(color_trc, **dict(_DEFAULTS, **_known(params)))
    h, w = layout.height, layout.width
    if planes.device.type == "cuda":
        dev = planes.device
    elif planes.is_pinned() and device is not None:
        dev = torch.device(device)
    else:
        raise RuntimeError("hdr2sdr_planes: the planes must live on a ROCm device or in pinned host memory (with device=...); "
                           "there is no CPU fallback")
    shape, dtype = ((h, w, 3), torch.int16) if form == "u16" else ((3, h, w), torch.float32) if form == "chw" else \
        ((h, w, 3), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    else:
        if _on_device_or_pinned(out, dev, "out") != dev:
            raise RuntimeError(f"hdr2sdr_planes: out is on {out.device}, the planes on {dev}")
        if tuple(out.shape) != shape or not out.is_contiguous() or \
                out.dtype not in ((torch.int16, torch.uint16) if form == "u16" else (torch.float32,)):
            raise ValueError(f"hdr2sdr_planes: out must be a contiguous {shape} {dtype} tensor for form {form!r}")
    cp = layout._c_planes(planes)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().nunif_hip_yuv_hdr_to_tensor(ctypes.byref(cp), pixfmt.FORMATS[layout.format], h, w,
                                                          int(bool(full_range)), int(color_trc), COLORSPACES[output_colorspace],
                                                          ctypes.byref(p), FORMS[form], ctypes.c_void_p(out.data_ptr()),
                                                          _hip.current_stream_ptr(dev)))
    return out


def hdr_yuv_entry(layout, full_range, color_trc, output_colorspace, **params):
    """The planar twin of :func:`hdr_entry`: an ``enter_fn(buf, device=...)`` for ``FrameRing(in_bytes=layout)``.  The HDR planes in
    the ring's pinned buffer arrive at ``process_fn`` as the tone-mapped CHW fp32 tensor — 3 bytes per pixel over PCIe, one kernel."""
    _check_names(color_trc, output_colorspace)
    if not isinstance(layout, pixfmt.PlaneLayout) or layout.format != PLANES_FORMAT:
        raise ValueError(f"hdr_yuv_entry needs a PlaneLayout of format {PLANES_FORMAT!r}, got {getattr(layout, 'format', layout)!r}")
    constants(color_trc, output_colorspace, **_known(params))      # a wrong parameter fails here, not on the first frame

    def enter(buf, device=None):
        return hdr2sdr_planes(buf, layout, full_range, color_trc, output_colorspace, form="chw", device=device, **params)
    enter.layout, enter.matrix, enter.full_range = layout, PLANES_MATRIX, bool(full_range)
    enter.color_trc, enter.output_colorspace, enter.params = color_trc, output_colorspace, dict(params)
    return enter


def planar_entry_refusal(in_format, in_matrix, entry):
    """Why ``in_format`` / ``in_matrix`` together with the HDR ``entry`` is not the one planar HDR form the engine has, or None."""
    if in_format == PLANES_FORMAT and in_matrix == PLANES_MATRIX and \
            all(hasattr(entry, a) for a in ("color_trc", "output_colorspace", "params")):
        return None
    return (f"in_format= together with hdr= is accepted in one form only: in_format={PLANES_FORMAT!r}, in_matrix={PLANES_MATRIX!r} "
            f"and an hdr entry from nunif_amd.nunif.utils.hdr.hdr_entry (got in_format={in_format!r}, in_matrix={in_matrix!r}"
            f"{'' if hasattr(entry, 'color_trc') else ', a callable without color_trc / output_colorspace / params'})")
