"""Planar YUV <-> the model's CHW fp32 tensor on the HIP engine (nunif_amd/csrc/pixfmt.hip): the two pixel-format conversions the
reference's ``process_video`` (``nunif/utils/video.py``) does with host libswscale around every frame —
``frame.reformat(**rgb24_options)`` (``:1038-1039``) + ``to_tensor`` (``:218-223``) going in, ``to_frame`` (``:259-269``) +
``reformatter(new_frame)`` (``:1084``) coming out — each as one launch that reads / writes the planes where they are.

A frame is three planes in ONE flat byte buffer (a device tensor, or a PINNED host tensor read / written zero-copy), described by a
:class:`PlaneLayout`: format, size and the byte pitch of each plane (PyAV's ``plane.line_size``).  Formats ``yuv420p``, ``yuv444p``,
``yuv420p10le``; a ``yuvj*`` name is the same layout (pass ``full_range=True``).  Matrix ``bt601`` / ``bt709`` / ``bt2020``.

The arithmetic is the ITU definition in fp32 with linear chroma resampling for the MPEG-2 / H.264 default chroma position, NOT
swscale's fixed point ("Pixel formats").  There is no CPU fallback: a buffer that is neither on a ROCm device nor pinned
raises.
"""
import ctypes

import numpy as np
import torch

from ... import _hip

MAX_DIM = 8192
FORMATS = {"yuv420p": 0, "yuv444p": 1, "yuv420p10le": 2}
_ALIASES = {"yuvj420p": "yuv420p", "yuvj444p": "yuv444p"}           # video.py:753-758: the same layout, full range
MATRICES = {"bt601": 601, "bt709": 709, "bt2020": 2020}


def _check_names(fmt, matrix):
    if fmt not in FORMATS:
        raise ValueError(f"format must be one of {sorted(FORMATS)} (or a yuvj* alias), got {fmt!r}")
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")


class PlaneLayout:
    """Where the three planes of one frame lie in a flat byte buffer.  ``pitches``: the byte pitch of each plane (default: packed
    rows rounded up to 64 bytes, so that every row allows the kernels' wide accesses); planes follow one another, each starting on
    a 64-byte boundary."""

    def __init__(self, format, width, height, pitches=None):
        format = _ALIASES.get(format, format)
        if format not in FORMATS:
            raise ValueError(f"format must be one of {sorted(FORMATS)} (or a yuvj* alias), got {format!r}")
        width, height = int(width), int(height)
        if not (1 <= width <= MAX_DIM and 1 <= height <= MAX_DIM):
            raise ValueError(f"a frame of {height} x {width} is outside H, W <= {MAX_DIM}")
        self.format, self.width, self.height = format, width, height
        self.bits = 10 if format == "yuv420p10le" else 8
        self.sample_bytes = 2 if self.bits > 8 else 1
        sub = format != "yuv444p"
        self.chroma_width = (width + 1) // 2 if sub else width
        self.chroma_height = (height + 1) // 2 if sub else height
        self.plane_widths = (width, self.chroma_width, self.chroma_width)
        self.plane_heights = (height, self.chroma_height, self.chroma_height)
        if pitches is None:
            pitches = [-(-w * self.sample_bytes // 64) * 64 for w in self.plane_widths]
        pitches = tuple(int(p) for p in pitches)
        if len(pitches) != 3:
            raise ValueError("pitches: one byte pitch per plane")
        for p, w in zip(pitches, self.plane_widths):
            if p < w * self.sample_bytes or p % self.sample_bytes:
                raise ValueError(f"a pitch of {p} bytes cannot hold a row of {w} samples of {self.sample_bytes} bytes")
        self.pitches = pitches
        self.offsets, off = [], 0
        for p, h in zip(pitches, self.plane_heights):
            self.offsets.append(off)
            off += -(-p * h // 64) * 64
        self.offsets = tuple(self.offsets)
        self.nbytes = off

    @property
    def numpy_dtype(self):
        return np.uint16 if self.sample_bytes == 2 else np.uint8

    def __eq__(self, other):
        return isinstance(other, PlaneLayout) and (self.format, self.width, self.height, self.pitches) == \
            (other.format, other.width, other.height, other.pitches)

    def __hash__(self):
        return hash((self.format, self.width, self.height, self.pitches))

    def __repr__(self):
        return f"PlaneLayout({self.format!r}, {self.width}, {self.height}, pitches={self.pitches})"

    def views(self, buf):
        """The three planes of the flat uint8 numpy array ``buf`` as [rows, samples] views (uint8 or uint16), padding excluded."""
        out = []
        for off, p, w, h in zip(self.offsets, self.pitches, self.plane_widths, self.plane_heights):
            plane = buf[off:off + p * h].reshape(h, p)
            out.append(plane.view(self.numpy_dtype)[:, :w] if self.sample_bytes == 2 else plane[:, :w])
        return out

    def pack(self, planes, buf=None, fill=0):
        """Three [rows, samples] arrays -> a flat uint8 numpy array in this layout (padding = ``fill``), or into ``buf``."""
        if buf is None:
            buf = np.full(self.nbytes, fill, dtype=np.uint8)
        for dst, src in zip(self.views(buf), planes):
            np.copyto(dst, src)
        return buf

    def _c_planes(self, buf):
        p = _hip.PixfmtPlanes()
        base = buf.data_ptr()
        for i in range(3):
            p.data[i] = base + self.offsets[i]
            p.pitch[i] = self.pitches[i]
        return p


def constants(matrix, full_range, bits, direction):
    """(9 coefficients row major, 3 offsets): the kernels' fp32 arguments.  ``direction`` 0: rgb = M (yuv - off); 1: yuv = M rgb +
    off.  Host only."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    if bits not in (8, 10) or direction not in (0, 1):
        raise ValueError("bits must be 8 or 10 and direction 0 or 1")
    m, off = (ctypes.c_float * 9)(), (ctypes.c_float * 3)()
    _hip.check(_hip.lib().nunif_hip_pixfmt_constants(MATRICES[matrix], int(bool(full_range)), bits, direction, m, off))
    return list(m), list(off)


def _on_device_or_pinned(t, device, what):
    if t.device.type == "cuda":
        return t.device
    if not (t.is_pinned() and device is not None):
        raise RuntimeError(f"pixfmt: {what} must live on a ROCm device or in pinned host memory (with device=...); "
                           "there is no CPU fallback")
    return torch.device(device)


def _check_buffer(planes, layout, what):
    if not isinstance(layout, PlaneLayout):
        raise ValueError("layout must be a PlaneLayout")
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or planes.dim() != 1 or not planes.is_contiguous() \
            or planes.numel() < layout.nbytes:
        raise ValueError(f"{what} must be a flat contiguous uint8 tensor of at least layout.nbytes = {layout.nbytes} bytes")


def yuv_to_tensor(planes, layout, matrix, full_range, device=None, out=None, frame_out=None, debug=False):
    """The planes of one frame (flat uint8 tensor in ``layout``, device or pinned) -> CHW fp32 [3, H, W] in [0, 1] on the device.
    ``frame_out``: also write the HWC rgb24 (uint8) / rgb48 (int16 or uint16, for the 10-bit format) frame, device or pinned, in
    the same launch — byte for byte ``to_frame`` of the tensor.  ``debug``: no clamp (tests)."""
    _check_names(layout.format if isinstance(layout, PlaneLayout) else None, matrix)
    _check_buffer(planes, layout, "planes")
    dev = _on_device_or_pinned(planes, device, "the planes")
    h, w = layout.height, layout.width
    if out is None:
        out = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    elif out.device != dev or tuple(out.shape) != (3, h, w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous fp32 [3, {h}, {w}] tensor on {dev}")
    frame_ptr = None
    if frame_out is not None:
        if debug:
            raise ValueError("frame_out is not available together with debug")
        want = (torch.uint8,) if layout.bits == 8 else (torch.int16, torch.uint16)
        if _on_device_or_pinned(frame_out, dev, "frame_out") != dev:
            raise RuntimeError(f"frame_out is on {frame_out.device}, the planes on {dev}")
        if tuple(frame_out.shape) != (h, w, 3) or frame_out.dtype not in want or not frame_out.is_contiguous():
            raise ValueError(f"frame_out must be a contiguous [{h}, {w}, 3] tensor of {want[0]}")
        frame_ptr = ctypes.c_void_p(frame_out.data_ptr())
    p = layout._c_planes(planes)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().nunif_hip_yuv_to_tensor(ctypes.byref(p), FORMATS[layout.format], h, w, MATRICES[matrix],
                                                      int(bool(full_range)), 1 if debug else 0, ctypes.c_void_p(out.data_ptr()),
                                                      frame_ptr, _hip.current_stream_ptr(dev)))
    return out


def tensor_to_yuv(x, layout, matrix, full_range, out=None):
    """CHW fp32 [3, H, W] on the device -> the planes of ``layout`` in a flat uint8 tensor (``out``: device or pinned; by default a
    new zeroed device tensor).  Clamp to [0, 1], matrix, range, chroma downsample, round half up.  Padding bytes are not written."""
    _check_names(layout.format if isinstance(layout, PlaneLayout) else None, matrix)
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("tensor_to_yuv: x must live on a ROCm device; there is no CPU fallback")
    h, w = layout.height, layout.width
    if x.dim() != 3 or tuple(x.shape) != (3, h, w):
        raise ValueError(f"tensor_to_yuv: x must be [3, {h}, {w}], got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    if out is None:
        out = torch.zeros(layout.nbytes, dtype=torch.uint8, device=x.device)
    else:
        _check_buffer(out, layout, "out")
        if _on_device_or_pinned(out, x.device, "out") != x.device:
            raise RuntimeError(f"tensor_to_yuv: out is on {out.device}, x on {x.device}")
    p = layout._c_planes(out)
    with torch.cuda.device(x.device):
        _hip.check(_hip.lib().nunif_hip_tensor_to_yuv(ctypes.c_void_p(x.data_ptr()), h, w, FORMATS[layout.format], MATRICES[matrix],
                                                      int(bool(full_range)), ctypes.byref(p), _hip.current_stream_ptr(x.device)))
    return out


def yuv_entry(layout, matrix, full_range):
    """An ``enter_fn(buf, device=...)`` for :class:`nunif_amd.frame_ring.FrameRing` (with ``in_bytes=layout.nbytes``): the planes in
    the ring's pinned buffer arrive at ``process_fn`` as the CHW fp32 tensor — 1.5 (3) bytes per pixel over PCIe, one kernel."""
    _check_names(layout.format, matrix)
    constants(matrix, full_range, layout.bits, 0)

    def enter(buf, device=None):
        return yuv_to_tensor(buf, layout, matrix, full_range, device=device)
    enter.layout, enter.matrix, enter.full_range = layout, matrix, bool(full_range)
    return enter


def yuv_leave(layout, matrix, full_range):
    """A ``leave_fn(y, bits, out=buf)`` for :class:`FrameRing` (with ``out_bytes=layout.nbytes``): the result leaves as the
    encoder's planes.  ``bits`` is the ring's; the depth written is the layout's."""
    _check_names(layout.format, matrix)
    constants(matrix, full_range, layout.bits, 1)

    def leave(y, bits=None, out=None):
        return tensor_to_yuv(y, layout, matrix, full_range, out=out)
    leave.layout, leave.matrix, leave.full_range = layout, matrix, bool(full_range)
    return leave


def from_av_frame(frame, buf=None):
    """An ``av.VideoFrame`` in one of the three formats -> (pinned flat uint8 tensor, PlaneLayout).  The planes are copied with
    numpy, plane by plane, at the frame's own ``line_size``; ``buf``: a pinned tensor to reuse."""
    import av  # noqa: F401  (the frame's type; this module loads without PyAV)
    layout = PlaneLayout(frame.format.name, frame.width, frame.height, [pl.line_size for pl in frame.planes[:3]])
    if buf is None or buf.numel() < layout.nbytes:
        buf = torch.empty(layout.nbytes, dtype=torch.uint8).pin_memory()
    dst = buf.numpy()
    for pl, off, pitch, h in zip(frame.planes, layout.offsets, layout.pitches, layout.plane_heights):
        np.copyto(dst[off:off + pitch * h], np.frombuffer(pl, dtype=np.uint8, count=pitch * h))
    return buf, layout


def copy_av_planes(frame, layout, views):
    """The planes of an ``av.VideoFrame`` (anything with ``planes`` that expose the buffer protocol and ``line_size``) -> the three
    [rows, samples] numpy views of ``layout`` (``PlaneLayout.views`` of a pinned buffer, ``FrameRing.input_buffer()``), row by row
    at the frame's own pitch."""
    for pl, dst, w, h in zip(frame.planes, views, layout.plane_widths, layout.plane_heights):
        src = np.frombuffer(pl, dtype=np.uint8, count=pl.line_size * h).reshape(h, pl.line_size)[:, :w * layout.sample_bytes]
        np.copyto(dst, src.view(layout.numpy_dtype) if layout.sample_bytes == 2 else src)


def to_av_frame(planes, layout, template=None, format=None):
    """The planes in a flat (pinned) uint8 tensor -> a new ``av.VideoFrame``; each row is copied at the new frame's own
    ``line_size``.  ``format``: the frame's pixel format NAME where it is not the layout's — a ``yuvj*`` alias for full-range codes:
    an encoder opened as ``yuvj420p`` converts a frame that calls itself ``yuv420p``, range and all.  ``template``: a frame whose
    pts, dts, time_base and opaque are carried over."""
    import av
    if format is not None and _ALIASES.get(format, format) != layout.format:
        raise ValueError(f"to_av_frame: {format!r} is not a name of the layout's format {layout.format!r}")
    frame = av.VideoFrame(layout.width, layout.height, format or layout.format)
    src = planes.numpy() if isinstance(planes, torch.Tensor) else planes
    for pl, off, pitch, w, h in zip(frame.planes, layout.offsets, layout.pitches, layout.plane_widths, layout.plane_heights):
        row = w * layout.sample_bytes
        dst = np.frombuffer(pl, dtype=np.uint8, count=pl.line_size * h).reshape(h, pl.line_size)
        np.copyto(dst[:, :row], src[off:off + pitch * h].reshape(h, pitch)[:, :row])
    if template is not None:
        frame.pts, frame.dts, frame.time_base = template.pts, template.dts, template.time_base
        if hasattr(template, "opaque"):
            frame.opaque = template.opaque
    return frame
