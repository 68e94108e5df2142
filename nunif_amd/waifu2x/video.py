"""The waifu2x video loop on the HIP engine: what ``waifu2x/ui_utils.py`` ``process_video``'s ``frame_callback`` (:154-177)
does per frame, without its blocking copies and pointwise ATen chain.

    numpy HWC frame --FrameRing (pinned, zero-copy)--> frame_to_tensor [+ quarter turn] --> ctx.convert -->
    [film grain: noise, noise-buffer blend, apply] + quantise, ONE launch --> pinned HWC frame --> numpy

``Waifu2xVideoStream`` is a ``frame -> frame | None`` callback as ``VU.process_video`` expects: the ring holds ``depth`` frames
in flight, so the first calls return ``None`` and ``callback(None)`` at the end of the stream returns the frames still inside,
in order (``nunif/utils/video.py:567-574`` ``get_new_frames`` accepts ``None``, one frame or a list).  It works on numpy frames;
``av.VideoFrame`` objects are converted at the outermost edge only (``av_callback``), as ``iw3/frame_pipeline.py`` does.
"""
import numpy as np
import torch

from ..frame_ring import FrameRing
from ..iw3 import _ops
from ..iw3.frame_pipeline import pix_fmt_requires_16bit
from ..nunif.utils import hdr as hdr_utils
from ..nunif.utils import pixfmt, rgb_noise


def _frame_pixels(frame):
    if isinstance(frame, np.ndarray):
        return frame
    if hasattr(frame, "data") and not callable(frame.data):                 # frame_pipeline.HostFrame
        return frame.data
    if hasattr(frame, "format") and hasattr(frame.format, "components"):    # PyAV: nunif/utils/video.py:226-233
        return frame.to_ndarray(format="rgb48le" if frame.format.components[0].bits > 8 else "rgb24")
    return frame.to_ndarray()


class Waifu2xVideoStream:
    def __init__(self, ctx, args, device=None, depth=3, seed=None, use_16bit=None, hdr=None,
                 in_format=None, in_matrix="bt709", in_full_range=False,
                 out_format=None, out_matrix="bt709", out_full_range=False):
        """``ctx``: a loaded ``Waifu2x`` context; ``args``: the reference's argparse namespace (``method``, ``noise_level``,
        ``tile_size``, ``batch_size``, ``tta``, ``disable_amp``, ``rotate_left`` / ``rotate_right``, ``grain``,
        ``grain_strength``, ``grain_speed``, ``pix_fmt``).  ``seed``: the grain seed; by default torch's
        ``torch.initial_seed()`` at construction, so ``torch.manual_seed`` makes a run repeatable.  ``use_16bit``: the output
        depth when the caller has already asked ``VU.pix_fmt_requires_16bit(args.pix_fmt)``; by default the engine's own copy of
        that rule.  The depth of the frames going in is each frame's own (uint8 or uint16), as in ``VU.to_tensor``.  ``hdr``: an
        entry from ``nunif_amd.nunif.utils.hdr.hdr_entry`` — the frames going in are then the rgb48 frames of a BT.2020 PQ / HLG
        source as decoded, and the tone mapping of ``VU.hdr2sdr`` is the ring's entry step (not together with a quarter turn).
        Together with ``in_format="yuv420p10le"`` and ``in_matrix="bt2020"`` the frames going in are that source's planes instead,
        and the entry step is the fused ``hdr.hdr_yuv_entry`` built from the entry's curve, colorspace and parameters.

        ``in_format`` (``yuv420p`` / ``yuv444p`` / ``yuv420p10le`` or a ``yuvj*`` alias, with ``in_matrix`` and ``in_full_range``):
        the frames going in are the decoder's planes, each a pair ``(flat uint8 array, pixfmt.PlaneLayout)``, and the conversion
        to rgb is the ring's entry step (``nunif_amd.nunif.utils.pixfmt``; not with a quarter turn; with ``hdr`` in the one form above).
        ``out_format`` (with ``out_matrix`` / ``out_full_range``): the frames coming out are the encoder's planes, flat uint8
        arrays in ``self.out_layout``; the film grain then runs as launches of its own in front of the conversion."""
        self.ctx, self.args = ctx, args
        self.device = torch.device(device if device is not None else ctx.device)
        if self.device.type != "cuda":
            raise RuntimeError("Waifu2xVideoStream needs a ROCm device; there is no CPU path")
        self.depth = depth
        if use_16bit is None:
            use_16bit = pix_fmt_requires_16bit(getattr(args, "pix_fmt", None))
        self.bits = 16 if use_16bit else 8
        self.turns = 1 if getattr(args, "rotate_left", False) else 3 if getattr(args, "rotate_right", False) else 0
        self.hdr = hdr
        if hdr is not None and self.turns:
            raise ValueError("Waifu2xVideoStream: hdr= cannot be combined with --rotate-left / --rotate-right: the tone-mapping "
                             "entry has no quarter turn; tone-map with VU.hdr2sdr first and pass the SDR frames")
        self._set_pixfmt(in_format, in_matrix, in_full_range, out_format, out_matrix, out_full_range)
        self._config = None                # a VideoOutputConfig whose state may name the formats at the first frame: bind_config
        self.out_layout = None
        self._yuv_enter = self._yuv_leave = None
        self.grain = bool(getattr(args, "grain", False))
        self.grain_strength = float(getattr(args, "grain_strength", 0.2))
        self.grain_speed = float(getattr(args, "grain_speed", 0.8))
        self.seed = (torch.initial_seed() if seed is None else int(seed)) & ((1 << 64) - 1)
        self.frame_counter = 0             # frames that have passed the leave step: the generator's counter
        self.noise_buffer = None           # [3, Ho, Wo] fp32, lives on the ring's leave stream
        self.frames_in = self.frames_out = 0
        self._ring = None
        self._in_shape = self._in_bits = None

    def _set_pixfmt(self, in_format=None, in_matrix="bt709", in_full_range=False,
                    out_format=None, out_matrix="bt709", out_full_range=False):
        for name, fmt, matrix in (("in", in_format, in_matrix), ("out", out_format, out_matrix)):
            if fmt is not None:
                if pixfmt._ALIASES.get(fmt, fmt) not in pixfmt.FORMATS:
                    raise ValueError(f"Waifu2xVideoStream: {name}_format must be one of {sorted(pixfmt.FORMATS)}, got {fmt!r}")
                if matrix not in pixfmt.MATRICES:
                    raise ValueError(f"Waifu2xVideoStream: {name}_matrix must be one of {sorted(pixfmt.MATRICES)}, got {matrix!r}")
        if in_format is not None and self.turns:
            raise ValueError("Waifu2xVideoStream: in_format= cannot be combined with --rotate-left / --rotate-right: the planar "
                             "entry has no quarter turn; pass rgb frames")
        if in_format is not None and self.hdr is not None:
            refusal = hdr_utils.planar_entry_refusal(pixfmt._ALIASES.get(in_format, in_format), in_matrix, self.hdr)
            if refusal:
                raise ValueError(f"Waifu2xVideoStream: {refusal}")
        self.in_format, self.in_matrix = pixfmt._ALIASES.get(in_format, in_format), in_matrix
        self.in_full_range = bool(in_full_range) or (in_format or "").startswith("yuvj")
        self.out_format, self.out_matrix = pixfmt._ALIASES.get(out_format, out_format), out_matrix
        self.out_pix_fmt = out_format      # the name as given (a yuvj* alias stays): what av_callback calls the frames it returns
        self.out_full_range = bool(out_full_range) or (out_format or "").startswith("yuvj")

    def bind_config(self, config, vf=""):
        """For the owner of a ``VU.process_video`` run, on the ``VideoOutputConfig`` its ``config_callback`` returns: declares this
        stream as an engine frame callback (not with a software ``--vf``, a quarter turn or ``hdr=``).  Where the engine's
        ``configure_colorspace`` then records ``config.state["engine_pixfmt"]``, the stream takes its six format options from
        there at its first frame: ``process_video`` hands it the decoder's frames and encodes the planes it returns."""
        from ..nunif.utils.video import declare_engine_callback
        if self._ring is not None:
            raise RuntimeError("Waifu2xVideoStream.bind_config: the stream has already taken frames")
        turns = self.turns or self.hdr is not None or self.in_format is not None or self.out_format is not None
        self._config = config if declare_engine_callback(config, vf=vf, turns=turns) else None

    def _read_config(self):
        from ..nunif.utils.video import ENGINE_PIXFMT
        config, self._config = self._config, None
        plan = config.state.get(ENGINE_PIXFMT)
        if plan:
            self._set_pixfmt(**plan)

    # ---- geometry -------------------------------------------------------------------------------------------------------
    def scale(self):
        method = self.args.method
        return 4 if method in ("scale4x", "noise_scale4x") else 1 if method == "noise" else 2

    def output_shape(self, in_shape):
        """(H, W, 3) of the frame that comes out for an (H, W, 3) frame going in."""
        h, w = in_shape[:2]
        if self.turns:
            h, w = w, h
        s = self.scale()
        return (h * s, w * s, 3)

    # ---- the three steps the ring runs ----------------------------------------------------------------------------------
    def _enter(self, hwc, device=None):
        if self._yuv_enter is not None:
            return self._yuv_enter(hwc, device=device)
        if self.hdr is not None:
            return self.hdr(hwc, device=device)
        return _ops.frame_to_tensor(hwc, device=device, turns=self.turns)

    def _convert(self, rgb):
        a = self.args
        out, _ = self.ctx.convert(rgb, None, a.method, a.noise_level, a.tile_size, a.batch_size, a.tta,
                                  enable_amp=not a.disable_amp, output_device=rgb.device)
        return out

    def _leave(self, y, bits, out=None):
        if self._yuv_leave is not None:
            if self.grain:                              # ui_utils.py:167-177 as launches of their own, then the planes
                y = y.to(torch.float32).contiguous()
                first = self.noise_buffer is None or self.noise_buffer.shape != y.shape
                if first:
                    self.noise_buffer = torch.empty_like(y)
                noise = rgb_noise.generate(tuple(y.shape), y.device, level=2, seed=self.seed, counter=self.frame_counter)
                rgb_noise.blend_noise_buffer(self.noise_buffer, noise, self.grain_speed, first)
                y = rgb_noise.apply_rgb_noise(y, self.noise_buffer, strength=self.grain_strength)
                self.frame_counter += 1
            return self._yuv_leave(y, bits, out=out)
        if not self.grain:
            return _ops.to_frame(y, bits, out=out)
        y = y.to(torch.float32).contiguous()
        if out is None:
            out = torch.empty((y.shape[1], y.shape[2], 3), dtype=torch.uint8 if bits == 8 else torch.int16, device=y.device)
        first = self.noise_buffer is None or self.noise_buffer.shape != y.shape          # ui_utils.py:169-171
        if first:
            self.noise_buffer = torch.empty_like(y)
        rgb_noise.grain_video_step(y, self.noise_buffer, out, bits=bits, level=2, seed=self.seed, counter=self.frame_counter,
                                   speed=self.grain_speed, first=first, strength=self.grain_strength)
        self.frame_counter += 1
        return out

    # ---- the callback ---------------------------------------------------------------------------------------------------
    def _open(self, in_shape, in_bits):
        self._in_shape, self._in_bits = tuple(in_shape), in_bits
        out_shape = self.output_shape(in_shape)
        in_layout = self._in_layout if self.in_format is not None else None
        if in_layout is None:
            self._yuv_enter = None
        elif self.hdr is not None:                      # the HDR planes of the decoder: gather and tone map in one launch
            self._yuv_enter = hdr_utils.hdr_yuv_entry(in_layout, self.in_full_range, self.hdr.color_trc, self.hdr.output_colorspace,
                                                      **self.hdr.params)
        else:
            self._yuv_enter = pixfmt.yuv_entry(in_layout, self.in_matrix, self.in_full_range)
        if self.out_format is not None:
            self.out_layout = pixfmt.PlaneLayout(self.out_format, out_shape[1], out_shape[0])
            self._yuv_leave = pixfmt.yuv_leave(self.out_layout, self.out_matrix, self.out_full_range)
        self._ring = FrameRing(self._convert, self._in_shape, out_shape, device=self.device,
                               depth=self.depth, bits=self.bits, in_bits=in_bits, enter_fn=self._enter, leave_fn=self._leave,
                               in_bytes=in_layout, out_bytes=self.out_layout)

    def drain(self):
        outs = self._ring.drain() if self._ring is not None else []
        self.frames_out += len(outs)
        return outs

    @torch.inference_mode()
    def __call__(self, frame):
        """One numpy HWC frame (uint8 or uint16, whatever the output depth is) in; ``None``, one frame or a list of frames out,
        always in submission order.  ``None`` in: the end of the stream — returns what the ring still holds."""
        if self._config is not None:
            self._read_config()
        if frame is None:
            return self.drain() or None
        if self.in_format is not None:
            return self._call_planar(frame)
        frame = _frame_pixels(frame)
        if frame.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"unsupported frame dtype {frame.dtype}")
        in_bits = 16 if frame.dtype == np.uint16 else 8      # a 10-bit source keeps its depth whatever the output pixel format is
        if self.hdr is not None and in_bits != 16:
            raise ValueError("Waifu2xVideoStream: hdr= needs rgb48 (uint16) frames")
        flushed = []
        if self._ring is None or tuple(frame.shape) != self._in_shape or in_bits != self._in_bits:
            flushed = self.drain()                      # a new frame size or depth: everything in flight leaves first
            self._open(frame.shape, in_bits)
        self.frames_in += 1
        out = self._ring.submit(np.ascontiguousarray(frame))
        if out is not None:
            self.frames_out += 1
            flushed.append(out)
        if not flushed:
            return None
        return flushed[0] if len(flushed) == 1 else flushed

    def _call_av_planar(self, frame):
        """A decoded PyAV frame: its planes are copied row by row, at the frame's own ``line_size``, straight into the ring's next
        pinned slot — the one host copy of the planar route."""
        name = pixfmt._ALIASES.get(frame.format.name, frame.format.name)
        if name != self.in_format:
            raise ValueError(f"Waifu2xVideoStream: the frame's format is {frame.format.name}, the stream was opened for "
                             f"{self.in_format}")
        layout = pixfmt.PlaneLayout(name, frame.width, frame.height)
        flushed = []
        if self._ring is None or getattr(self, "_in_layout", None) != layout:
            flushed = self.drain()
            self._in_layout = layout
            self._open((layout.height, layout.width, 3), 8)
        self.frames_in += 1
        pixfmt.copy_av_planes(frame, layout, self._ring.input_buffer())
        out = self._ring.submit(None)
        if out is not None:
            self.frames_out += 1
            flushed.append(out)
        if not flushed:
            return None
        return flushed[0] if len(flushed) == 1 else flushed

    def _call_planar(self, frame):
        if hasattr(frame, "planes") and hasattr(frame, "format"):
            return self._call_av_planar(frame)
        try:
            buf, layout = frame
        except (TypeError, ValueError):
            raise ValueError("Waifu2xVideoStream: with in_format= a frame is a pair (flat uint8 array, PlaneLayout)") from None
        if not isinstance(layout, pixfmt.PlaneLayout) or layout.format != self.in_format:
            raise ValueError(f"Waifu2xVideoStream: the frame's layout is {layout!r}, the stream was opened for {self.in_format}")
        buf = np.asarray(buf)
        if buf.dtype != np.uint8 or buf.ndim != 1 or buf.size < layout.nbytes:
            raise ValueError(f"Waifu2xVideoStream: the planes must be a flat uint8 array of {layout.nbytes} bytes")
        flushed = []
        if self._ring is None or getattr(self, "_in_layout", None) != layout:
            flushed = self.drain()
            self._in_layout = layout
            self._open((layout.height, layout.width, 3), 8)
        self.frames_in += 1
        out = self._ring.submit(buf[:layout.nbytes])
        if out is not None:
            self.frames_out += 1
            flushed.append(out)
        if not flushed:
            return None
        return flushed[0] if len(flushed) == 1 else flushed

    def av_callback(self, to_frame, to_planar_frame=None):
        """The same callback for a PyAV loop: ``to_frame`` is the reference's ``VU.to_frame`` (numpy HWC -> ``av.VideoFrame``).
        With ``out_format`` the planes that come out are wrapped by ``to_planar_frame(planes, layout, format=name)`` instead, ``name`` being ``out_format`` as it was given (by default
        ``pixfmt.to_av_frame``); with ``in_format`` the frames going in are the decoder's own ``av.VideoFrame`` s."""
        def wrap(out):
            if self.out_format is not None:             # asked per frame: bind_config settles the formats at the first one
                return (to_planar_frame or pixfmt.to_av_frame)(out, self.out_layout, format=self.out_pix_fmt)
            return to_frame(out)

        def callback(frame):
            out = self(frame)
            if out is None:
                return None
            if isinstance(out, list):
                return [wrap(o) for o in out]
            return wrap(out)
        return callback

    def test_callback(self, to_frame):
        """``VU.process_video``'s size probe (``video.py:1006-1012``): a blank frame of the output size, without touching the
        ring, the noise buffer or the frame counter."""
        def callback(frame):
            if frame is None:
                return None
            shape = self.output_shape(_frame_pixels(frame).shape)
            return to_frame(np.zeros(shape, dtype=np.uint16 if self.bits == 16 else np.uint8))
        return callback
