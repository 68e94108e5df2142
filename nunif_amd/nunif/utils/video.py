"""``hdr2sdr`` of ``nunif/utils/video.py`` (reference :309-416) on the HIP engine.

``process_video``'s ``input_reformatter`` (:1025-1036) calls it for every decoded frame of a BT.2020 PQ / HLG source that is written
to a bt709 / bt601 output.  The reference uploads the rgb48 frame, runs about thirty eager passes over it, truncates and downloads;
here the frame is copied into a pinned buffer, one kernel (nunif_amd/csrc/hdr.hip) reads it there and writes the uint16 result into
a second pinned buffer, and that buffer becomes the output frame: nothing is staged on the device.

Only this function is the engine's: the decode loop, ``configure_colorspace`` and everything else of the reference's module stay
its own.  ``av`` is imported inside the function, so this module loads without PyAV.
"""
import threading

import numpy as np
import torch

from . import hdr as _hdr

COLORSPACE_BT2020 = 9                                            # video.py:71
COLOR_TRC_ARIB_STD_B67, COLOR_TRC_SMPTE2084 = 18, 16             # video.py:72-73

_hdr_lock = threading.Lock()
_hdr_buffers = {}                     # device -> [pinned in, pinned out] (flat int16, grown by size), used under the lock


def _pinned(device, shape):
    n = shape[0] * shape[1] * shape[2]
    bufs = _hdr_buffers.get(device)
    if bufs is None or bufs[0].numel() < n:
        bufs = _hdr_buffers[device] = [torch.empty(n, dtype=torch.int16).pin_memory() for _ in range(2)]
    return [b[:n].view(shape) for b in bufs]


def hdr2sdr(
        av_frame, color_trc, output_colorspace,
        pq_exposure=110.0, pq_white_point=5.0,
        hlg_exposure=1.2, hlg_white_point=0.8, hlg_saturation_gain=0.9,
        device="cpu"
):
    assert output_colorspace in {"bt709", "bt601"}
    assert av_frame.colorspace == COLORSPACE_BT2020
    assert color_trc in {COLOR_TRC_SMPTE2084, COLOR_TRC_ARIB_STD_B67}

    device = torch.device(device)
    if device.type != "cuda":
        from ... import install as inst
        ref = inst.original("nunif.utils.video", "hdr2sdr")
        if ref is None:
            raise RuntimeError(f"nunif_amd hdr2sdr needs a ROCm device (got {device}); there is no CPU fallback")
        return ref(av_frame, color_trc, output_colorspace, pq_exposure=pq_exposure, pq_white_point=pq_white_point,
                   hlg_exposure=hlg_exposure, hlg_white_point=hlg_white_point, hlg_saturation_gain=hlg_saturation_gain,
                   device=device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())

    import av
    from av.video.reformatter import ColorRange, Colorspace

    rgb_ndarray = av_frame.to_ndarray(format="rgb48le",
                                      src_color_range=av_frame.color_range,
                                      dst_color_range=ColorRange.JPEG)
    with _hdr_lock:
        src, dst = _pinned(device, rgb_ndarray.shape)
        np.copyto(src.numpy(), rgb_ndarray.view(np.int16))
        _hdr.hdr2sdr_tensor(src, color_trc, output_colorspace, pq_exposure=pq_exposure, pq_white_point=pq_white_point,
                            hlg_exposure=hlg_exposure, hlg_white_point=hlg_white_point,
                            hlg_saturation_gain=hlg_saturation_gain, form="u16", out=dst, device=device)
        torch.cuda.current_stream(device).synchronize()
        # from_ndarray copies the pixels into the frame's own planes: the pinned buffer is free again when it returns
        output_frame = av.video.frame.VideoFrame.from_ndarray(dst.numpy().view(np.uint16), format="rgb48le")

    if output_colorspace == "bt709":
        output_frame.colorspace = Colorspace.ITU709
    else:
        output_frame.colorspace = Colorspace.ITU601
    output_frame.color_range = ColorRange.JPEG

    output_frame.pts = av_frame.pts
    output_frame.dts = av_frame.dts
    output_frame.time_base = av_frame.time_base
    output_frame.opaque = av_frame.opaque

    return output_frame
