"""Frame scheduler of the iw3 video path: batching, depth -> normalise -> stereo -> quantise, ordered output.

What it replaces in the reference:

* ``VU.FrameCallbackPool`` (``nunif/utils/video.py:1622-1757``) — batches decoded frames and hands them to a thread
  pool, one worker per device replica;
* ``iw3.utils.bind_batch_frame_callback`` (``iw3/utils.py:709-831``) — the per-batch body: ``preprocess_image`` ->
  ``depth_model.infer`` -> ``minmax_normalize`` (EMA look-ahead, flush at scene cuts) -> ``apply_divergence`` /
  ``apply_rgbd`` -> ``postprocess_image`` -> ``VU.to_frame``; four locks (``depth_lock``, ``sbs_lock`` and two
  ``TicketLock`` s, ``nunif/utils/ticket_lock.py``) put the worker threads back in frame order.

Here nothing is threaded, so there is nothing to re-order and no lock exists:

* inside one GPU the two halves of a batch run on two HIP streams as a software pipeline — the depth stage of batch
  k+1 (stream D: preprocess, depth net, the sequential min-max state) overlaps the stereo stage of batch k (stream S:
  warp / side model, output format, quantise); hand-over is one HIP event per batch (`_StagePipeline`);
* across GPUs it is one process per GPU (``stereo_frames_sharded``): batch b belongs to rank ``b mod world``.  Frames are
  independent except for the EMA min-max recurrence, which only needs two scalars per frame: every round the ranks
  all-gather their frames' (min, max) — 8 bytes per frame over RCCL — and each rank replays the *same* recurrence
  (``EMAMinMaxScaler`` itself, fed with two-element tensors) to obtain the (lo, hi) of its own frames.  The output is
  bit-identical to a single process walking the frames in order.  Finished, already-quantised frames go to the I/O rank
  with one gather.  Models with temporal state (VideoDepthAnything, the video inpaint queue) do not shard by frame:
  shard those by scene segment — this function refuses them.

The reference call signatures are kept: ``bind_batch_frame_callback(depth_model, side_model, segment_pts, args)``
returns ``(frame_callback, preprocess_callback)`` and ``FrameCallbackPool`` takes the reference's constructor
arguments, so ``iw3/utils.py:1137-1153`` reads the same.  A decoded frame is anything with ``.pts`` and either
``.to_ndarray()`` (PyAV) or ``.data`` (``HostFrame``); results are quantised HWC uint8 / uint16 tensors (what
``VU.to_frame`` wraps into an ``av.VideoFrame``), left on the device unless ``to_host=True``.

The device functions are looked up in a ``PipelineOps`` table whose defaults are the HIP engine (no CPU fallback: they
raise for CPU tensors).  The ``-m "not gpu"`` tests pass torch-CPU stand-ins to exercise the host logic against the
reference's own scheduler (``tests/golden/frame_pool.npz``).
"""
import os

import torch
import torch.distributed as dist

from ..parallel import shard_indices
from .depth_scaler import EMAMinMaxScaler


class HostFrame:
    """Minimal stand-in for ``av.VideoFrame`` at this boundary: HWC uint8 / uint16 pixels + presentation time stamp."""

    def __init__(self, data, pts):
        self.data, self.pts = data, pts

    def to_ndarray(self, format=None):
        return self.data


def chunks(array, n):
    """iw3/utils.py:62-64."""
    for i in range(0, len(array), n):
        yield array[i:i + n]


class PipelineOps:
    """Device functions used by the scheduler.  Defaults: the HIP engine (``nunif_amd.iw3.utils``)."""

    def __init__(self, to_tensor=None, preprocess_image=None, apply_divergence=None, apply_rgbd=None,
                 postprocess_image=None, to_frame=None, hdr=None,
                 in_format=None, in_matrix="bt709", in_full_range=False,
                 out_format=None, out_matrix="bt709", out_full_range=False):
        """``in_format`` / ``in_matrix`` / ``in_full_range``: the frames going in are the decoder's planes (``frame.data`` is a
        pair ``(flat uint8 array or tensor, pixfmt.PlaneLayout)`` of that format) and ``to_tensor`` is the engine's planar entry;
        ``out_format`` / ``out_matrix`` / ``out_full_range``: a stereo pair leaves as the encoder's planes (a flat uint8 tensor in
        ``out_layout(h, w)``) instead of an HWC frame.  By default both ends are rgb, as before.  ``hdr``: an entry from
        ``nunif_amd.nunif.utils.hdr.hdr_entry`` — the planes are those of a BT.2020 PQ / HLG source and the planar entry tone-maps
        them in the same launch; only with ``in_format="yuv420p10le"`` and ``in_matrix="bt2020"``."""
        from . import utils as U
        from ..nunif.utils import pixfmt
        for name, fmt, matrix in (("in", in_format, in_matrix), ("out", out_format, out_matrix)):
            if fmt is not None and pixfmt._ALIASES.get(fmt, fmt) not in pixfmt.FORMATS:
                raise ValueError(f"PipelineOps: {name}_format must be one of {sorted(pixfmt.FORMATS)}, got {fmt!r}")
            if fmt is not None and matrix not in pixfmt.MATRICES:
                raise ValueError(f"PipelineOps: {name}_matrix must be one of {sorted(pixfmt.MATRICES)}, got {matrix!r}")
        if in_format is not None and to_tensor is not None:
            raise ValueError("PipelineOps: in_format= replaces to_tensor; pass one of them")
        if out_format is not None and to_frame is not None:
            raise ValueError("PipelineOps: out_format= replaces to_frame; pass one of them")
        if hdr is not None:
            from ..nunif.utils import hdr as hdr_utils
            refusal = hdr_utils.planar_entry_refusal(pixfmt._ALIASES.get(in_format, in_format), in_matrix, hdr)
            if refusal:
                raise ValueError(f"PipelineOps: {refusal}")
        self.hdr = hdr
        self.in_format, self.in_matrix = pixfmt._ALIASES.get(in_format, in_format), in_matrix
        self.in_full_range = bool(in_full_range) or (in_format or "").startswith("yuvj")
        self.out_format, self.out_matrix = pixfmt._ALIASES.get(out_format, out_format), out_matrix
        self.out_pix_fmt = out_format      # the name as given (a yuvj* alias stays): what an av.VideoFrame of the planes is called
        self.out_full_range = bool(out_full_range) or (out_format or "").startswith("yuvj")
        self._config = None                # a VideoOutputConfig whose state may name the formats at the first frame: bind_config
        self._own_edges = to_tensor is None and to_frame is None
        self._staging, self._staged = [], 0
        self.to_tensor = to_tensor or self._to_tensor
        self.preprocess_image = preprocess_image or U.preprocess_image
        self.apply_divergence = apply_divergence or U.apply_divergence
        self.apply_rgbd = apply_rgbd or U.apply_rgbd
        self.postprocess_image = postprocess_image or U.postprocess_image
        self.to_frame = to_frame or U.to_frame_tensor
        # with both defaults in place a stereo pair leaves through U.postprocess_to_frame (compose + quantise fused where the
        # format allows); a caller's own postprocess_image / to_frame keep the two-step route
        self._fused_out = U.postprocess_to_frame if (postprocess_image is None and to_frame is None) else None

    def bind_config(self, config, vf=""):
        """For the owner of a ``VU.process_video`` run whose frame callback comes from one of the binders below, on the
        ``VideoOutputConfig`` its ``config_callback`` returns: declares the callback as the engine's (not with a software ``--vf``,
        nor with a caller's own ``to_tensor`` / ``to_frame`` or formats given up front).  Where the engine's
        ``configure_colorspace`` then records ``config.state["engine_pixfmt"]``, the six format options are taken from there at
        the first frame: the scheduler is handed the decoder's frames and returns the encoder's planes."""
        from ..nunif.utils.video import declare_engine_callback
        fixed = not self._own_edges or self.in_format is not None or self.out_format is not None or self.hdr is not None
        self._config = config if declare_engine_callback(config, vf=vf, turns=fixed) else None

    def _settle(self):
        if self._config is not None:
            from ..nunif.utils.video import ENGINE_PIXFMT
            config, self._config = self._config, None
            plan = config.state.get(ENGINE_PIXFMT)
            if plan:                    # names as configure_colorspace records them: already checked
                from ..nunif.utils import pixfmt
                self.in_format, self.in_matrix, self.in_full_range = plan["in_format"], plan["in_matrix"], plan["in_full_range"]
                self.out_pix_fmt, self.out_matrix, self.out_full_range = \
                    plan["out_format"], plan["out_matrix"], plan["out_full_range"]
                self.out_format = pixfmt._ALIASES.get(self.out_pix_fmt, self.out_pix_fmt)

    def _to_tensor(self, frame, device=None):
        from . import utils as U
        self._settle()
        if self.in_format is not None:
            return self._planes_to_tensor(frame, device=device)
        return U.to_tensor(_frame_pixels(frame), device=device)

    def _pinned_slot(self, nbytes):
        """One of four pinned staging buffers, handed out in turn; the kernel that read a buffer zero-copy on its last turn has
        finished before it is written again (its event)."""
        i, self._staged = self._staged % 4, self._staged + 1
        if len(self._staging) <= i:
            self._staging.append([torch.empty(nbytes, dtype=torch.uint8).pin_memory(), None])
        slot = self._staging[i]
        if slot[1] is not None:                      # before the buffer is written OR dropped: the host allocator knows nothing of
            slot[1].synchronize()                    # a kernel's zero-copy read
            slot[1] = None
        if slot[0].numel() < nbytes:
            slot[0] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        return slot

    def _planes_to_tensor(self, frame, device=None):
        """The planes always reach the kernel in device or PINNED memory, read zero-copy: a pinned or device tensor as it is; a
        numpy array, an unpinned tensor or a decoded ``av.VideoFrame`` through one host copy into a pinned staging buffer."""
        import numpy as np
        from ..nunif.utils import pixfmt
        slot = None
        if hasattr(frame, "planes") and hasattr(frame, "format") and not isinstance(getattr(frame, "data", None), tuple):
            name = pixfmt._ALIASES.get(frame.format.name, frame.format.name)
            layout = pixfmt.PlaneLayout(name, frame.width, frame.height) if name in pixfmt.FORMATS else name
            if layout != name and name == self.in_format:
                slot = self._pinned_slot(layout.nbytes)
                pixfmt.copy_av_planes(frame, layout, layout.views(slot[0].numpy()))
                buf = slot[0]
        else:
            try:
                buf, layout = frame.data
            except (AttributeError, TypeError, ValueError):
                raise ValueError("PipelineOps: with in_format= a frame's data is a pair (flat uint8 buffer, PlaneLayout)") from None
        if not isinstance(layout, pixfmt.PlaneLayout) or layout.format != self.in_format:
            raise ValueError(f"PipelineOps: the frame's layout is {layout!r}, the scheduler was opened for {self.in_format}")
        if slot is None and not (torch.is_tensor(buf) and (buf.is_cuda or buf.is_pinned())):
            if device is None or torch.device(device).type != "cuda":
                raise RuntimeError("PipelineOps: the planar entry needs a ROCm device; there is no CPU fallback")
            host = buf.numpy() if torch.is_tensor(buf) else np.asarray(buf)
            if host.dtype != np.uint8 or host.ndim != 1 or host.size < layout.nbytes:
                raise ValueError(f"PipelineOps: the planes must be a flat uint8 buffer of {layout.nbytes} bytes")
            slot = self._pinned_slot(layout.nbytes)
            np.copyto(slot[0].numpy()[:layout.nbytes], host[:layout.nbytes])
            buf = slot[0]
        if self.hdr is not None:
            from ..nunif.utils import hdr as hdr_utils
            x = hdr_utils.hdr2sdr_planes(buf, layout, self.in_full_range, self.hdr.color_trc, self.hdr.output_colorspace,
                                         form="chw", device=device, **self.hdr.params)
        else:
            x = pixfmt.yuv_to_tensor(buf, layout, self.in_matrix, self.in_full_range, device=device)
        if slot is not None:
            slot[1] = torch.cuda.Event()
            slot[1].record(torch.cuda.current_stream(x.device))
        return x

    def out_layout(self, height, width):
        """The layout of the planes ``stereo_out`` writes for an output image of ``height`` x ``width``."""
        from ..nunif.utils import pixfmt
        return pixfmt.PlaneLayout(self.out_format, width, height)

    def stereo_out(self, left_eye, right_eye, args, use_16bit=False):
        """One stereo pair -> the output frame: ``to_frame(postprocess_image(left, right, args))``."""
        self._settle()
        if self.out_format is not None:
            from ..nunif.utils import pixfmt
            sbs = self.postprocess_image(left_eye, right_eye, args)
            layout = self.out_layout(sbs.shape[-2], sbs.shape[-1])
            planes = pixfmt.tensor_to_yuv(sbs, layout, self.out_matrix, self.out_full_range)
            planes.plane_layout = layout             # for whoever wraps the planes into a frame: bind_av_frame_callback
            return planes
        if self._fused_out is not None:
            return self._fused_out(left_eye, right_eye, args, use_16bit=use_16bit)
        return self.to_frame(self.postprocess_image(left_eye, right_eye, args), use_16bit=use_16bit)


def _frame_pixels(frame):
    if hasattr(frame, "data") and not callable(frame.data):
        return frame.data
    if hasattr(frame, "format") and hasattr(frame.format, "components"):     # PyAV: nunif/utils/video.py:226-233
        return frame.to_ndarray(format="rgb48le" if frame.format.components[0].bits > 8 else "rgb24")
    return frame.to_ndarray()


def pix_fmt_requires_16bit(pix_fmt):
    """nunif/utils/video.py:272-279."""
    return pix_fmt in {"yuv420p10le", "p010le", "yuv422p10le", "yuv444p10le", "yuv420p12le", "yuv422p12le",
                       "yuv444p12le", "yuv444p16le", "gbrp16le", "gbrp12le", "gbrp10le", "rgb48le"}


class _StagePipeline:
    """Two HIP streams per device: D (depth stage) and S (stereo stage).  ``depth_stage`` / ``stereo_stage`` are context managers
    that order the stage behind its producer (D waits for the caller's upload stream, S waits for D) and ``record_stream`` every
    tensor that crosses, so the caching allocator cannot recycle it while the other stream still reads it; ``stereo_done`` is the
    event a consumer waits on."""

    def __init__(self, device, enabled):
        self.enabled = bool(enabled) and torch.device(device).type == "cuda"
        self.device = torch.device(device)
        if self.enabled:
            self.depth_stream = torch.cuda.Stream(self.device)
            self.stereo_stream = torch.cuda.Stream(self.device)

    def depth_stage(self, inputs=()):
        if not self.enabled:
            return _NullContext()
        cur = torch.cuda.current_stream(self.device)
        self.depth_stream.wait_stream(cur)             # the batch was uploaded on the caller's stream
        for t in inputs:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(self.depth_stream)
        return torch.cuda.stream(self.depth_stream)

    def stereo_stage(self, inputs=()):
        if not self.enabled:
            return _NullContext()
        self.stereo_stream.wait_stream(self.depth_stream)
        for t in inputs:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(self.stereo_stream)
        return torch.cuda.stream(self.stereo_stream)

    def stereo_done(self):
        """Event after everything queued on S so far (None without streams).  The consumer waits on THIS, so the caller's
        stream — which only uploads frames — never waits for the stereo stage and batch k+1's depth stage can start."""
        if not self.enabled:
            return None
        ev = torch.cuda.Event()
        ev.record(self.stereo_stream)
        return ev


class FrameList(list):
    """A list of output frames + the HIP event after which they are complete (None: complete on the current stream)."""
    event = None


class _NullContext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _stack(tensors):
    """``torch.stack`` of the per-frame tensors of a batch: device tensors go through the engine's own copy kernel (one launch,
    or no copy at all when they are consecutive slices of one buffer) instead of ATen's CatArrayBatchedCopy."""
    tensors = list(tensors)
    if tensors and torch.is_tensor(tensors[0]) and tensors[0].is_cuda:
        from . import _ops
        return _ops.stack(tensors)
    return torch.stack(tensors)


def bind_batch_frame_callback(depth_model, side_model, segment_pts, args, ops=None):
    """``iw3/utils.py:709-831``.  Returns ``(frame_callback, preprocess_callback)``:
    ``preprocess_callback(x, pts, flush) -> call_args`` and ``frame_callback(call_args) -> [quantised frames]``.

    ``x`` is a B x 3 x H x W float batch (None for the final flush), ``pts`` its time stamps.  Output frames come out in
    input order; with an EMA look-ahead of N frames (``depth_model.get_ema_buffer_size()``) they lag by N - 1 frames
    until a scene cut (``pts in segment_pts``) or the final flush releases them.  Source frames wait in HBM next to
    their depth (the reference parks them in host memory as uint8, :769-775 — 288 GB make that unnecessary; for 8 / 16
    bit sources the values are the same)."""
    ops = ops or PipelineOps()
    segment_pts = set(segment_pts or ())
    src_queue = []                      # (CHW source frame, pts), in frame order
    use_16bit = pix_fmt_requires_16bit(getattr(args, "pix_fmt", None))
    stages = {}                         # device -> _StagePipeline
    tickets = [0]

    def _stage(device):
        key = str(device)
        if key not in stages:
            # (the reference's --cuda-stream flag selects per-THREAD streams, :806-815; there are no threads here, the two
            #  stage streams are always on for a ROCm device unless NUNIF_IW3_STAGE_STREAMS=0)
            stages[key] = _StagePipeline(device, os.environ.get("NUNIF_IW3_STAGE_STREAMS", "1") != "0")
        return stages[key]

    def _stereo(depth_list, device, st, flush=False):
        results = FrameList()
        for depths in chunks(depth_list, args.batch_size):
            depths = [d.to(device) for d in depths]
            # source frames follow their depth: with a look-ahead ring a chunk can hold frames that entered on another device
            pairs = [(x.to(device), t) for x, t in (src_queue.pop(0) for _ in range(len(depths)))]
            reset_pts = [t in segment_pts for _, t in pairs]
            with st.stereo_stage(depths + [x for x, _ in pairs]):
                depths = _stack(depths)
                x_srcs = _stack([x for x, _ in pairs])
                if getattr(args, "rgbd", False) or getattr(args, "half_rgbd", False):
                    left, right = ops.apply_rgbd(x_srcs, depths, mapper=args.mapper)
                else:
                    left, right = ops.apply_divergence(depths, x_srcs, args, side_model, reset_pts=reset_pts)
                if left is None:              # an inpaint side model whose 12-frame queue is still filling
                    continue
                results += [ops.stereo_out(left[i], right[i], args, use_16bit=use_16bit) for i in range(left.shape[0])]
        if flush:
            # end of stream: frames still inside a side model with a temporal queue (the video inpaint FrameQueue) come
            # out here — the reference only sends inpaint methods through the single-frame route, which flushes the side
            # model at iw3/utils.py:658-663; this route accepts them too, so it must not drop the queue's tail
            with st.stereo_stage([]):
                results += _side_flush(side_model, args, ops, use_16bit)
        results.event = st.stereo_done()
        return results

    @torch.inference_mode()
    def frame_callback(call_args):
        x, pts, flush, _ticket = call_args
        if flush:
            device = _device_of(args, depth_model)
            st = _stage(device)
            with st.depth_stage():
                depth_list = depth_model.flush_minmax_normalize()
            return _stereo(depth_list, device, st, flush=True)
        device = x.device
        st = _stage(device)
        reset_ema = [t in segment_pts for t in pts]
        with st.depth_stage([x]):
            x = ops.preprocess_image(x, args)
            for x_, pts_ in zip(x, pts):
                src_queue.append((x_, pts_))
            depth_batch = depth_model.infer(x, tta=getattr(args, "tta", False), low_vram=getattr(args, "low_vram", False),
                                            enable_amp=not getattr(args, "disable_amp", False),
                                            edge_dilation=getattr(args, "edge_dilation", 0),
                                            depth_aa=getattr(args, "depth_aa", False))
            depth_list = depth_model.minmax_normalize(depth_batch, reset_ema=reset_ema)
        return _stereo(depth_list, device, st)

    def preprocess_callback(x, pts, flush):
        tickets[0] += 1                 # kept for signature parity (the reference's enqueue ticket); order is inherent here
        return (x, pts, flush, tickets[0] - 1)

    # what ShardedFrameCallbackPool (one video on N GPUs) needs to run the same stages across ranks
    frame_callback.spec = {"depth_model": depth_model, "side_model": side_model, "segment_pts": segment_pts, "args": args,
                           "ops": ops}
    return frame_callback, preprocess_callback


def _side_flush(side_model, args, ops, use_16bit):
    """Frames still inside a side model with a temporal queue (the video inpaint ``FrameQueue``), iw3/utils.py:658-663."""
    out = []
    if hasattr(side_model, "flush"):
        left, right = side_model.flush(enable_amp=not getattr(args, "disable_amp", False))
        if left is not None:
            out = [ops.stereo_out(le, re, args, use_16bit=use_16bit) for le, re in zip(left, right)]
    return out


def bind_single_frame_callback(depth_model, side_model, segment_pts, args, ops=None):
    """``iw3/utils.py:618-709`` (``--batch-size 1`` / ``--max-workers 0`` route): ``frame_callback(frame) -> [frames]``,
    ``frame_callback(None)`` flushes the scaler and the side model."""
    ops = ops or PipelineOps()
    segment_pts = set(segment_pts or ())
    src_queue = []
    use_16bit = pix_fmt_requires_16bit(getattr(args, "pix_fmt", None))
    infer_kw = lambda: dict(tta=getattr(args, "tta", False), low_vram=getattr(args, "low_vram", False),     # noqa: E731
                            enable_amp=not getattr(args, "disable_amp", False),
                            edge_dilation=getattr(args, "edge_dilation", 0), depth_aa=getattr(args, "depth_aa", False))

    def _postprocess(depths, flush):
        frames = []
        for depth in depths:
            x, t = src_queue.pop(0)
            if getattr(args, "rgbd", False) or getattr(args, "half_rgbd", False):
                left, right = ops.apply_rgbd(x, depth, mapper=args.mapper)
            else:
                left, right = ops.apply_divergence(depth, x, args, side_model, reset_pts=[t in segment_pts])
            if left is None:                  # a side model that is still filling its queue
                continue
            pairs = [(left, right)] if left.ndim == 3 else list(zip(left, right))
            frames += [ops.stereo_out(le, re, args, use_16bit=use_16bit) for le, re in pairs]
        if flush:
            frames += _side_flush(side_model, args, ops, use_16bit)
        return frames

    @torch.inference_mode()
    def frame_callback(frame):
        if frame is None:
            return _postprocess(depth_model.flush_minmax_normalize(), flush=True)
        x = ops.preprocess_image(ops.to_tensor(frame, device=_device_of(args, depth_model)), args)
        src_queue.append((x, frame.pts))
        depth = depth_model.minmax_normalize_chw(depth_model.infer(x, **infer_kw()))
        depths = [depth] if depth is not None else []
        flush = frame.pts in segment_pts
        if flush:
            depths += depth_model.flush_minmax_normalize()
            depth_model.reset_state()
        return _postprocess(depths, flush=flush)

    depth_model.reset()
    return frame_callback


def bind_vda_frame_callback(depth_model, side_model, segment_pts, args, ops=None):
    """``iw3/utils.py:834-926``: the route of depth models that normalise themselves over a window of frames
    (``VideoDepthAnythingModel.infer_with_normalize`` / ``flush_with_normalize``): batches of ``args.batch_size`` frames,
    outputs lag the inputs by the model's window; ``frame_callback(None)`` drains model, scaler and side model."""
    ops = ops or PipelineOps()
    segment_pts = set(segment_pts or ())
    src_queue, batch_queue, pts_queue = [], [], []
    use_16bit = pix_fmt_requires_16bit(getattr(args, "pix_fmt", None))
    kw = lambda: dict(enable_amp=not getattr(args, "disable_amp", False), edge_dilation=getattr(args, "edge_dilation", 0),   # noqa: E731
                      depth_aa=getattr(args, "depth_aa", False))

    def _postprocess(depth_list, flush=False):
        results = []
        for depths in chunks(depth_list, args.batch_size):
            depths = _stack(depths)
            pairs = [src_queue.pop(0) for _ in range(depths.shape[0])]
            x_srcs = _stack([x for x, _ in pairs])
            if getattr(args, "rgbd", False) or getattr(args, "half_rgbd", False):
                left, right = ops.apply_rgbd(x_srcs, depths, mapper=args.mapper)
            else:
                left, right = ops.apply_divergence(depths, x_srcs, args, side_model,
                                                   reset_pts=[t in segment_pts for _, t in pairs])
            if left is not None:
                results += [ops.stereo_out(left[i], right[i], args, use_16bit=use_16bit) for i in range(left.shape[0])]
        if flush:
            results += _side_flush(side_model, args, ops, use_16bit)
        return results

    def _batch_infer():
        x = ops.preprocess_image(_stack(batch_queue), args)
        for x_, t in zip(x, pts_queue):
            src_queue.append((x_, t))
        depth_list = depth_model.infer_with_normalize(x, list(pts_queue), segment_pts, **kw())
        pts_queue.clear()
        batch_queue.clear()
        return _postprocess(depth_list)

    @torch.inference_mode()
    def frame_callback(frame):
        if frame is None:
            results = _batch_infer() if batch_queue else []
            return results + _postprocess(depth_model.flush_with_normalize(**kw()), flush=True)
        batch_queue.append(ops.to_tensor(frame, device=_device_of(args, depth_model)))
        pts_queue.append(frame.pts)
        return _batch_infer() if len(batch_queue) == args.batch_size else None

    depth_model.reset()
    return frame_callback


def bind_av_frame_callback(depth_model, side_model, segment_pts, args, config, to_frame, vf="", to_planar_frame=None):
    """``bind_single_frame_callback`` as the ``frame_callback`` of a ``VU.process_video`` run: decoded ``av.VideoFrame`` s in, a list
    of ``av.VideoFrame`` s out.  ``config``: the ``VideoOutputConfig`` the run's ``config_callback`` returns — call this from
    inside that callback: the op table declares itself on it (``PipelineOps.bind_config``), and where the engine's
    ``configure_colorspace`` answers with ``config.state["engine_pixfmt"]`` the frames enter as the decoder's planes and leave as
    the encoder's, under the pixel-format name the encoder was opened with.  Otherwise they are the rgb frames they were:
    ``to_frame`` is the reference's ``VU.to_frame``.  ``to_planar_frame(planes, layout, format=name)``: by default
    ``pixfmt.to_av_frame``."""
    import numpy as np
    from ..nunif.utils import pixfmt
    ops = PipelineOps()
    ops.bind_config(config, vf=vf)
    inner = bind_single_frame_callback(depth_model, side_model, segment_pts, args, ops=ops)

    def wrap(out):
        layout = getattr(out, "plane_layout", None)
        if layout is not None:
            return (to_planar_frame or pixfmt.to_av_frame)(out.cpu().numpy(), layout, format=ops.out_pix_fmt)
        arr = out.cpu().numpy()                      # a quantised HWC frame; int16 carries the uint16 bit pattern (_ops.to_frame)
        return to_frame(arr.view(np.uint16) if arr.dtype == np.int16 else arr)

    def frame_callback(frame):
        return [wrap(out) for out in inner(frame)]

    frame_callback.ops = ops
    return frame_callback


def _device_of(args, depth_model):
    state = getattr(args, "state", None) or {}
    if "device" in state:
        return torch.device(state["device"])
    return torch.device(depth_model.device) if getattr(depth_model, "device", None) is not None else torch.device("cpu")


class _Pending:
    def __init__(self, frames, device):
        self.frames = frames
        self.event = getattr(frames, "event", None)
        if self.event is None and torch.device(device).type == "cuda":
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(device))

    def done(self):
        return self.event is None or self.event.query()

    def result(self):
        if self.event is not None:
            self.event.synchronize()
        return self.frames


class FrameCallbackPool:
    """``nunif/utils/video.py:1622-1757`` with the reference's constructor arguments.

    ``max_workers`` is the number of *batches in flight on the GPU* (their kernels are queued asynchronously; a batch is
    handed back when its HIP event has fired, or when more than ``max_workers`` are pending); ``max_workers <= 0`` hands a
    batch back in the call that completed it, exactly like the reference's ``_DummyThreadPool`` path.  A LIST of GPUs is
    refused (see ``__init__``): multi-GPU runs are one process per GPU with ``stereo_frames_sharded``."""

    def __init__(self, frame_callback, batch_size, device, max_workers=1, max_batch_queue=2, require_pts=False,
                 skip_pts=-1, require_flush=False, preprocess_callback=None, postprocess_callback=None, use_16bit=False,
                 ops=None, to_host=False):
        devices = list(device) if isinstance(device, (tuple, list)) else [device]
        if len(devices) == 0:
            raise ValueError("FrameCallbackPool needs at least one device")
        # several devices (the reference's ``--gpu 0 1 ...``: one worker thread per device replica, video.py:1650-1700):
        # whole BATCHES go to the devices round-robin; their kernels are queued asynchronously on each device's own
        # streams, so the devices run concurrently from this one thread, and ``pending`` keeps the frame order
        self.devices = [torch.device(d) for d in devices]
        if len(self.devices) > 1 and any(d.type == "cuda" for d in self.devices):
            # Round-robin batches over several GPUs from one thread leaves three orderings open that only hardware can
            # validate (round-2 advisor): depths produced on device B's stage stream are consumed on device A without an
            # event, the EMA scaler's device state is pushed from two devices' streams, and look-ahead chunks mix devices.
            # No multi-GPU box has run this path, so it is refused rather than shipped unvalidated; the supported
            # multi-GPU layout is one process per GPU with ``stereo_frames_sharded``, which is what the
            # reference's ``--gpu 0 1 ...`` maps to here.  (Lists of host "devices" still work: scheduler-order tests.)
            raise NotImplementedError("FrameCallbackPool: several GPUs in one process are not supported; run one process "
                                      "per GPU and use nunif_amd.iw3.frame_pipeline.stereo_frames_sharded")
        self.device = self.devices[0]
        self._next_device = 0
        self.ops = ops or PipelineOps()
        self.frame_callback, self.preprocess_callback = frame_callback, preprocess_callback
        self.postprocess_callback = postprocess_callback
        self.batch_size, self.max_workers, self.max_batch_queue = batch_size, max_workers, max_batch_queue
        self.require_pts, self.require_flush, self.skip_pts = require_pts, require_flush, skip_pts
        self.use_16bit, self.to_host = use_16bit, to_host
        self.frame_queue, self.pts_queue, self.pending = [], [], []

    def make_args(self, batch, pts_batch, flush):
        if self.require_pts and self.require_flush:
            return (batch, pts_batch, flush)
        if self.require_pts:
            return (batch, pts_batch)
        if self.require_flush:
            return (batch, flush)
        return (batch,)

    def submit(self, *call_args, device=None):
        if self.preprocess_callback is not None:
            frames = self.frame_callback(self.preprocess_callback(*call_args))
        else:
            frames = self.frame_callback(*call_args)
        return _Pending(frames, device or self.device)

    def get_results(self, pending):
        frames = pending.result()
        if self.postprocess_callback is not None:
            frames = self.postprocess_callback(frames)
        if frames is None:
            return []
        out = []
        for f in frames:
            if torch.is_tensor(f) and f.is_floating_point():       # a callback that returns CHW float images
                f = self.ops.to_frame(f, use_16bit=self.use_16bit)
            out.append(f.cpu().numpy() if (self.to_host and torch.is_tensor(f)) else f)
        return out

    def _close_batch(self):
        batch = _stack(self.frame_queue)
        pts = list(self.pts_queue)
        self.frame_queue.clear()
        self.pts_queue.clear()
        dev = self.devices[self._next_device]
        self._next_device = (self._next_device + 1) % len(self.devices)
        self.pending.append(self.submit(*self.make_args(batch, pts, False), device=dev))

    def __call__(self, frame):
        if frame is None:
            return self.finish()
        if frame.pts <= self.skip_pts:
            return None
        self.pts_queue.append(frame.pts)
        self.frame_queue.append(self.ops.to_tensor(frame, device=self.devices[self._next_device]))
        if len(self.frame_queue) == self.batch_size:
            self._close_batch()
        if self.pending and (self.max_workers <= 0 or len(self.pending) > self.max_workers or self.pending[0].done()):
            return self.get_results(self.pending.pop(0))
        return None

    def finish(self):
        if self.frame_queue:
            self._close_batch()
        remains = []
        while self.pending:
            remains += self.get_results(self.pending.pop(0))
        if self.require_flush:
            remains += self.get_results(self.submit(*self.make_args(None, None, True)))
        return remains

    def shutdown(self):
        self.pending = []


# ---- across GPUs: one process per GPU ----------------------------------------------------------------------------------
def _replay_scaler(depth_model):
    decay, buffer_size = depth_model.get_ema_state()
    return EMAMinMaxScaler(decay=decay, buffer_size=buffer_size)


class ShardedStereoStream:
    """Depth + stereo over a STREAM of frames sharded across ranks, batch ``b`` on rank ``b mod world`` (module docstring).

    ``push_round(my_frames, round_pts)`` takes one round = up to ``world`` consecutive batches: ``round_pts[r]`` are the time
    stamps of the batch rank ``r`` owns, ``my_frames`` the CHW float tensors of THIS rank's batch (empty when the round is short).
    Per round: depth inference on the own batch, one all-gather of ``[batch_size, 2]`` (min, max) floats per rank, the sequential
    EMA of ``depth_model``'s scaler replayed over ALL frames (every rank replays the same recurrence, so every rank also knows
    which frames of which rank just left the look-ahead), stereo on the own frames that did.  ``deliver()`` moves what became
    ready since the last call to rank ``dst`` (one padded gather) and returns, on ``dst``, the next frames in stream order;
    ``finish()`` flushes the look-ahead.  ``stereo_fn(x_srcs[B,3,H,W], depths[B,1,h,w], reset_pts) -> list of quantised HWC
    frames``.  The output is bit-identical to a single process walking the frames in order."""

    def __init__(self, depth_model, stereo_fn, batch_size, segment_pts=(), group=None, dst=0, infer_kwargs=None, device=None):
        if getattr(depth_model, "has_temporal_state", False):
            raise ValueError("a depth model with temporal state cannot be sharded by frame; shard by scene segment")
        self.group, self.dst = group, dst
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.depth_model, self.stereo_fn, self.batch_size = depth_model, stereo_fn, batch_size
        self.segment_pts = set(segment_pts or ())
        self.infer_kwargs = infer_kwargs or {}
        self.device = torch.device(device) if device is not None else None
        self.replay = _replay_scaler(depth_model)
        self.replay_order = []             # global frame indices waiting inside ``replay``, oldest first
        self.raw = {}                      # my frames: index -> (source, raw depth)
        self.ready = []                    # my frames with their range: (index, lo, hi), in frame order
        self.fresh = []                    # indices (any rank's) that left the look-ahead since the last deliver()
        self.out_local, self.pts, self.owner = {}, {}, {}
        self.n = 0                         # frames seen so far
        self.meta = None                   # (shape, dtype) of an output frame, agreed on at the first delivery
        self.arrived, self.emit_next = {}, 0
        self._pending = []                 # rounds whose (min, max) table is still on its way to the host (ROCm devices)
        self._pinned, self._pin_i = [], 0
        # rounds between queueing a depth batch and replaying it (0: A/B runs).  lag + 1 tables are in flight and lag + 2 pinned
        # buffers rotate, so the value is bounded: anything outside [0, 4] (or not a number) is the default
        try:
            lag = int(os.environ.get("NUNIF_SHARD_LAG", "1"))
        except ValueError:
            lag = 1
        self._lag = lag if 0 <= lag <= 4 else 1

    # -- the replayed recurrence ---------------------------------------------------------------------------------------------
    def _assign(self, results):
        for _, lo, hi in results:
            idx = self.replay_order.pop(0)
            self.fresh.append(idx)
            if idx in self.raw:
                self.ready.append((idx, lo, hi))

    def _feed(self, idx, mn, mx):
        self.replay_order.append(idx)
        _, lo, hi = self.replay.update(torch.stack([mn, mx]), return_minmax=True)
        if lo is not None:
            self._assign([(None, lo, hi)])
        if self.pts[idx] in self.segment_pts:
            self._assign(self.replay.flush(return_minmax=True))
            self.replay.reset()

    def _run_ready(self):
        for group_ in chunks(list(self.ready), self.batch_size):
            xs = torch.stack([self.raw[i][0] for i, _, _ in group_])
            ds = torch.stack([self.replay.normalize(self.raw[i][1], lo, hi) for i, lo, hi in group_])
            outs = self.stereo_fn(xs, ds, [self.pts[i] in self.segment_pts for i, _, _ in group_])
            for (i, _, _), o in zip(group_, outs):
                self.out_local[i] = o
                del self.raw[i]
        self.ready.clear()

    def _dev(self):
        if self.device is None:
            dev = getattr(self.depth_model, "device", None)     # a rank that owns no frame at all still joins the collectives
            self.device = torch.device(dev) if dev is not None else torch.device("cpu")
        return self.device

    # -- the stream ------------------------------------------------------------------------------------------------------------
    def push_round(self, my_frames, round_pts):
        assert 0 < len(round_pts) <= self.world, "a round is at most one batch per rank"
        ids, base = [], self.n
        for r, p in enumerate(round_pts):
            ids.append(list(range(base, base + len(p))))
            for i, t in zip(ids[-1], p):
                self.pts[i], self.owner[i] = t, r
            base += len(p)
        self.n = base
        mine = ids[self.rank] if self.rank < len(ids) else []
        assert len(mine) == len(my_frames), (len(mine), len(my_frames))
        dev = self._dev() if not mine else None
        local = None
        if mine:
            x = torch.stack(list(my_frames))
            if self.device is None:
                self.device = x.device
            dev = x.device
            d = self.depth_model.infer(x, **self.infer_kwargs)
            mm = torch.stack([d.flatten(1).amin(dim=1), d.flatten(1).amax(dim=1)], dim=1).float()
            local = torch.zeros(self.batch_size, 2, dtype=torch.float32, device=dev)
            local[:len(mine)] = mm
            for k, i in enumerate(mine):
                self.raw[i] = (x[k], d[k])
        if local is None:
            local = torch.zeros(self.batch_size, 2, dtype=torch.float32, device=dev)
        if self.world > 1:
            buf = [torch.empty_like(local) for _ in range(self.world)]
            dist.all_gather(buf, local, group=self.group)
            table = torch.stack(buf)
        else:
            table = local[None]
        if table.is_cuda:
            # The (min, max) table travels to the host ASYNCHRONOUSLY and is consumed one round later: the host never waits for the
            # depth network it has just queued — it replays round r - 1 (long finished on the device) and queues those frames' stereo
            # stage while the device runs round r.  (Consumed in the same call, every round cost a host synchronisation with the GPU
            # idle during the ~100 launches of the next forward: 0.69-0.82 instead of ~0.55 ms per 1080p frame on one GPU.)
            n_pin = self._lag + 2                                             # lag + 1 in flight at most, one being filled
            if len(self._pinned) != n_pin or self._pinned[0].shape != table.shape:
                while self._pending:                                         # a shape change (the last, short round) first drains
                    self._consume(self._pending.pop(0))
                self._pinned = [torch.empty(table.shape, dtype=table.dtype, pin_memory=True) for _ in range(n_pin)]
            host = self._pinned[self._pin_i % n_pin]
            self._pin_i += 1
            host.copy_(table, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(table.device))
            self._pending.append((ids, host, ev))
            while len(self._pending) > self._lag:
                self._consume(self._pending.pop(0))
        else:
            self._consume((ids, table, None))

    def _consume(self, entry):
        ids, table, ev = entry
        if ev is not None:
            ev.synchronize()
        for r, b in enumerate(ids):
            for k, i in enumerate(b):
                self._feed(i, table[r][k, 0], table[r][k, 1])
        self._run_ready()

    def finish(self):
        while self._pending:
            self._consume(self._pending.pop(0))
        self._assign(self.replay.flush(return_minmax=True))
        self._run_ready()
        assert not self.raw, "frames left without a range"

    def deliver(self):
        """Everything that left the look-ahead since the last call goes to ``dst``; returns the next frames of the stream there
        (``[]`` on the other ranks, and while a frame of an earlier batch is still outstanding)."""
        fresh, self.fresh = self.fresh, []
        if not fresh:
            return []
        if self.world == 1:
            for i in fresh:
                del self.owner[i], self.pts[i]
            return [self.out_local.pop(i) for i in fresh]          # the recurrence releases frames in stream order
        per = [[i for i in fresh if self.owner[i] == r] for r in range(self.world)]
        for i in fresh:
            del self.owner[i], self.pts[i]
        maxc = max(len(p) for p in per)
        mine = per[self.rank]
        if self.meta is None:                                       # (every rank takes this branch in the same call)
            probe = self.out_local[mine[0]] if mine else None
            meta = [None] * self.world
            dist.all_gather_object(meta, None if probe is None else (tuple(probe.shape), str(probe.dtype)), group=self.group)
            shape, dtype = next(m for m in meta if m is not None)
            self.meta = (shape, getattr(torch, dtype.split(".")[-1]))
        shape, dtype = self.meta
        block = torch.zeros((maxc, *shape), dtype=dtype, device=self._dev())
        for k, i in enumerate(mine):
            block[k] = self.out_local.pop(i)
        # Frames travel as BYTES: 10 / 12 / 16-bit pix_fmts make int16 frames (``use_16bit``, _ops.py to_frame) and neither the
        # nccl nor the gloo process group moves Short tensors ("Unsupported data type")
        wire = block.view(torch.uint8)
        if self.rank != self.dst:
            dist.gather(wire, None, dst=self.dst, group=self.group)
            return []
        parts = [torch.empty_like(wire) for _ in range(self.world)]
        dist.gather(wire, parts, dst=self.dst, group=self.group)
        for r in range(self.world):
            got = parts[r].view(dtype)
            for k, i in enumerate(per[r]):
                self.arrived[i] = got[k]
        out = []
        while self.emit_next in self.arrived:
            out.append(self.arrived.pop(self.emit_next))
            self.emit_next += 1
        return out


def stereo_frames_sharded(frames, pts, segment_pts, depth_model, stereo_fn, batch_size, group=None, dst=0,
                          infer_kwargs=None):
    """Depth + stereo over ``frames`` (sequence of CHW float tensors on the rank's device; entries a rank does not own may
    be None), batch ``b`` on rank ``b mod world``.  ``stereo_fn(x_srcs[B,3,H,W], depths[B,1,h,w], reset_pts) -> list of
    quantised HWC frames``.  Returns the ordered list on ``dst`` (None elsewhere).  The list form of ``ShardedStereoStream``:
    per round one all-gather of ``[batch_size, 2]`` floats per rank and one gather of the frames that left the look-ahead."""
    st = ShardedStereoStream(depth_model, stereo_fn, batch_size, segment_pts, group=group, dst=dst, infer_kwargs=infer_kwargs,
                             device=_any_device(frames, depth_model))
    batches = list(chunks(list(range(len(frames))), batch_size))
    out = []
    for r0 in range(0, len(batches), st.world):
        rb = batches[r0:r0 + st.world]
        mine = rb[st.rank] if st.rank < len(rb) else []
        st.push_round([frames[i] for i in mine], [[pts[i] for i in b] for b in rb])
        out += st.deliver()
    st.finish()
    out += st.deliver()
    if st.world > 1 and st.rank != dst:
        return None
    assert len(out) == len(frames), (len(out), len(frames))
    return out


class ShardedFrameCallbackPool:
    """The reference's ``VU.FrameCallbackPool`` (``nunif/utils/video.py:1622-1757``, same constructor arguments) for ONE video on
    N GPUs, one process per GPU (BASELINE configs[3]): EVERY rank runs the reference's decode loop over the whole file and calls
    this object once per decoded frame; a frame is uploaded and processed only by the rank that owns its batch (batch ``b`` on
    rank ``b mod world``), the EMA normalisation is replayed across the ranks (``ShardedStereoStream``) and the finished frames
    come back, in stream order, from the calls made on rank ``dst`` — the rank whose ``process_video`` encodes.  On the other
    ranks every call returns ``None`` (their encoders see an empty stream; ``nunif_amd.launch`` points them at a scratch file).

    ``frame_callback`` must be the callback of THIS module's ``bind_batch_frame_callback`` (its ``spec`` attribute names the
    depth / side model, the scene cuts and the CLI arguments): the sharded flow runs the same stages in another order, it does
    not call the bound function.  ``to_output(frame_tensor)`` converts a finished HWC tensor for the caller's encoder
    (``av.VideoFrame.from_ndarray`` in the launcher); default: the tensor itself."""

    def __init__(self, frame_callback, batch_size, device, max_workers=1, max_batch_queue=2, require_pts=False, skip_pts=-1,
                 require_flush=False, preprocess_callback=None, postprocess_callback=None, use_16bit=False, ops=None,
                 group=None, dst=0, to_output=None):
        spec = getattr(frame_callback, "spec", None)
        if spec is None:
            raise TypeError("ShardedFrameCallbackPool needs the frame_callback of nunif_amd.iw3.frame_pipeline."
                            "bind_batch_frame_callback (it carries the models and arguments the sharded flow runs)")
        devices = list(device) if isinstance(device, (tuple, list)) else [device]
        if len(devices) != 1:
            raise ValueError("ShardedFrameCallbackPool: one device per process (the launcher binds --gpu <id> per rank)")
        self.device = torch.device(devices[0])
        self.args, self.depth_model, self.side_model = spec["args"], spec["depth_model"], spec["side_model"]
        if hasattr(self.side_model, "flush"):
            raise ValueError("a side model with a temporal queue cannot be sharded by frame; shard by scene segment")
        self.ops = ops or spec["ops"] or PipelineOps()
        self.batch_size, self.skip_pts, self.use_16bit = batch_size, skip_pts, use_16bit
        self.postprocess_callback = postprocess_callback
        self.to_output = to_output or (lambda f: f)
        a = self.args
        self.stream = ShardedStereoStream(
            self.depth_model, self._stereo, batch_size, spec["segment_pts"], group=group, dst=dst, device=self.device,
            infer_kwargs=dict(tta=getattr(a, "tta", False), low_vram=getattr(a, "low_vram", False),
                              enable_amp=not getattr(a, "disable_amp", False), edge_dilation=getattr(a, "edge_dilation", 0),
                              depth_aa=getattr(a, "depth_aa", False)))
        self.rank, self.world = self.stream.rank, self.stream.world
        self.round_pts, self.my_frames, self.count = [[]], [], 0

    def _stereo(self, x_srcs, depths, reset_pts):
        a = self.args
        if getattr(a, "rgbd", False) or getattr(a, "half_rgbd", False):
            left, right = self.ops.apply_rgbd(x_srcs, depths, mapper=a.mapper)
        else:
            left, right = self.ops.apply_divergence(depths, x_srcs, a, self.side_model, reset_pts=reset_pts)
        return [self.ops.stereo_out(left[i], right[i], a, use_16bit=self.use_16bit) for i in range(left.shape[0])]

    def _close_round(self):
        pts = [p for p in self.round_pts if p]
        if pts:
            frames = self.my_frames
            if frames:
                frames = list(self.ops.preprocess_image(_stack(frames), self.args))
            with torch.inference_mode():
                self.stream.push_round(frames, pts)
        self.round_pts, self.my_frames = [[]], []

    def _out(self, frames):
        if self.postprocess_callback is not None:
            frames = self.postprocess_callback(frames)
        return [self.to_output(f) for f in (frames or [])]

    def __call__(self, frame):
        if frame is None:
            return self.finish()
        if frame.pts <= self.skip_pts:
            return None
        if len(self.round_pts[-1]) == self.batch_size:
            self.round_pts.append([])
        owner = len(self.round_pts) - 1
        self.round_pts[-1].append(frame.pts)
        if owner == self.rank:
            self.my_frames.append(self.ops.to_tensor(frame, device=self.device))
        self.count += 1
        if owner == self.world - 1 and len(self.round_pts[-1]) == self.batch_size:
            self._close_round()
            return self._out(self.stream.deliver()) or None
        return None

    def finish(self):
        self._close_round()
        out = self.stream.deliver()
        with torch.inference_mode():
            self.stream.finish()
        return self._out(out + self.stream.deliver())

    def shutdown(self):
        self.my_frames, self.round_pts = [], [[]]


def _any_device(frames, depth_model=None):
    for f in frames:
        if f is not None:
            return f.device
    dev = getattr(depth_model, "device", None)          # a rank that owns no frame at all still joins the collectives
    return torch.device(dev) if dev is not None else torch.device("cpu")
