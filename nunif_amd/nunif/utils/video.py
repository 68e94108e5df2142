"""``hdr2sdr`` of ``nunif/utils/video.py`` (reference :309-416) on the HIP engine.

``process_video``'s ``input_reformatter`` (:1025-1036) calls it for every decoded frame of a BT.2020 PQ / HLG source that is written
to a bt709 / bt601 output.  The reference uploads the rgb48 frame, runs about thirty eager passes over it, truncates and downloads;
here the frame is copied into a pinned buffer, one kernel (nunif_amd/csrc/hdr.hip) reads it there and writes the uint16 result into
a second pinned buffer, and that buffer becomes the output frame: nothing is staged on the device.

``configure_colorspace`` (reference :763-854) runs the reference's own function and then, where both ends are planar YUV formats the
engine converts itself (nunif_amd/csrc/pixfmt.hip) and the frame callback is the engine's, takes the two host swscale calls out of
``process_video``'s loop: ``rgb24_options`` becomes ``{}`` (``input_reformatter`` :1038-1041 hands the decoded frame through),
``reformatter`` the identity, and what the callback needs is recorded under ``config.state["engine_pixfmt"]``.

The decode loop and everything else of the reference's module stay its own.  ``av`` is imported inside the functions, so this module
loads without PyAV.
"""
import threading

import numpy as np
import torch

from . import hdr as _hdr

COLORSPACE_BT2020 = 9                                            # video.py:71
COLOR_TRC_ARIB_STD_B67, COLOR_TRC_SMPTE2084 = 18, 16             # video.py:72-73

# ---- pixel formats: configure_colorspace ---------------------------------------------------------------------------------------
ENGINE_CALLBACK = "engine_frame_callback"      # config.state key an engine callback sets: "I take and return planar frames"
ENGINE_PIXFMT = "engine_pixfmt"                # config.state key configure_colorspace answers with
_MATRIX_OF = {1: "bt709", 5: "bt601", 6: "bt601", COLORSPACE_BT2020: "bt2020"}   # AVCOL_SPC_*: BT709, BT470BG, SMPTE170M, BT2020_NCL
_RANGE_MPEG, _RANGE_JPEG = 1, 2                                                  # AVCOL_RANGE_*
_HDR2SDR_TARGETS = {"bt709", "bt709-tv", "bt709-pc", "bt601", "bt601-tv", "bt601-pc"}            # video.py:1028-1029


def declare_engine_callback(config, vf="", turns=0):
    """Called by an engine frame callback's owner on the ``VideoOutputConfig`` its ``config_callback`` returns, BEFORE
    ``process_video`` reaches ``configure_colorspace``: the callback accepts the decoder's planar frames and returns the encoder's.
    Not declared (the reference's rgb route stays) with a software ``--vf`` — the filter graph may hand on another pixel format than
    the stream's — and with a quarter turn, which the planar entry does not have.  Returns whether it was declared."""
    config.state.pop(ENGINE_PIXFMT, None)
    declared = not (vf or "").strip() and not turns
    if declared:
        config.state[ENGINE_CALLBACK] = True
    else:
        config.state.pop(ENGINE_CALLBACK, None)
    return declared


def _engine_pixfmt(output_stream, input_stream, config):
    from . import pixfmt
    if output_stream is None or input_stream is None or not config.state.get(ENGINE_CALLBACK):
        return None
    options = config.state.get("rgb24_options")
    if not options:                                          # unknown source range or matrix, rgb24 / gbrp, "unspecified"
        return None
    in_format, out_format = getattr(input_stream, "pix_fmt", None), config.pix_fmt
    if pixfmt._ALIASES.get(in_format, in_format) not in pixfmt.FORMATS or \
            pixfmt._ALIASES.get(out_format, out_format) not in pixfmt.FORMATS:
        return None
    ctx = output_stream.codec_context
    try:
        in_range, in_space = int(options["src_color_range"]), int(options["src_colorspace"])
        # the matrix the reference's reformatter converts to (:809-814, :835-838) is the one it names for the rgb frame in between
        out_range, out_space = int(ctx.color_range), int(options["dst_colorspace"])
    except (KeyError, TypeError, ValueError):
        return None
    if in_space not in _MATRIX_OF or out_space not in _MATRIX_OF or \
            in_range not in (_RANGE_MPEG, _RANGE_JPEG) or out_range not in (_RANGE_MPEG, _RANGE_JPEG):
        return None
    if input_stream.codec_context.color_trc in (COLOR_TRC_SMPTE2084, COLOR_TRC_ARIB_STD_B67) and \
            config.colorspace in _HDR2SDR_TARGETS:           # input_reformatter sends these frames through hdr2sdr (:1026-1036)
        return None
    if out_format in pixfmt._ALIASES and out_range != _RANGE_JPEG:      # a yuvj* name the caller chose, with a limited-range tag
        return None
    # out_format is the NAME the reference settled on (a yuvj* alias for 8-bit full range, :753-758): process_video opens the
    # encoder with it (:1018), and the frames the callback returns must carry the same name or the encoder converts them again
    return dict(in_format=pixfmt._ALIASES.get(in_format, in_format), in_matrix=_MATRIX_OF[in_space],
                in_full_range=in_range == _RANGE_JPEG,
                out_format=out_format, out_matrix=_MATRIX_OF[out_space], out_full_range=out_range == _RANGE_JPEG)


def _identity(frame):
    return frame


def configure_colorspace(output_stream, input_stream, config):
    from ... import install as inst
    ref = inst.original("nunif.utils.video", "configure_colorspace")
    if ref is None:
        raise RuntimeError("nunif_amd configure_colorspace runs on top of the reference's own: call nunif_amd.install() first")
    config.state.pop(ENGINE_PIXFMT, None)
    ret = ref(output_stream, input_stream, config)
    plan = _engine_pixfmt(output_stream, input_stream, config)
    if plan is not None:
        config.state[ENGINE_PIXFMT] = plan
        config.state["rgb24_options"] = {}
        config.state["reformatter"] = _identity
    return ret


# ---- HDR -> SDR ----------------------------------------------------------------------------------------------------------------
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
