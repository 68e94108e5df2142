"""Letterbox detection, crop and uncrop of iw3's ``--autocrop`` on the HIP engine.

Mirrors ``nunif/utils/autocrop.py`` (reference) name for name and signature for signature: ``AutoCropDetector`` :6-207,
``autocrop_analyze_video`` :210-249, ``AutoCrop`` :252-360 and ``AutoCropDummy`` :363-371.  The per-row and per-column statistics,
their decisions and the accumulation over frames run in nunif_amd/csrc/autocrop.hip (``nunif_hip_autocrop_stats``), the crop and
uncrop copies in ``nunif_hip_autocrop_crop_pad``.  What the reference decides on the host stays on the host and keeps its own
expressions: ``border_count / frame_count >= threshold`` (an fp32 division and an fp32 comparison: 19 of 20 frames at threshold
0.95 is a border), ``mask_to_slice_*``, ``apply_mod``, ``calc_pad`` and ``calc_crop``.

Frames are ``[3, H, W]`` or ``[B, 3, H, W]`` float tensors on a ROCm device, H <= 4608 and W <= 8192 (larger frames are refused).
There is no CPU fallback: a host tensor is answered by the reference's own class while ``install()`` is active and raises
otherwise.
"""
import ctypes

import torch

from ... import _hip

MAX_H, MAX_W = 4608, 8192
_BLACK_MODES = {"black_tb", "black_lr", "black"}
_TB_MODES = {"black_tb", "black", "flat_tb", "flat"}
_LR_MODES = {"black_lr", "black", "flat_lr", "flat"}
_BAND = 32                           # rows per band of the black column pass (autocrop.hip kBand)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _reference(name, t, what):
    """The reference's own ``name`` for a host tensor while ``install()`` is active; ``None`` for a device tensor."""
    if t.device.type == "cuda":
        return None
    from ...install import original
    ref = original("nunif.utils.autocrop", name)
    if ref is None:
        raise RuntimeError(f"{what}: the HIP engine needs a ROCm device tensor (got {t.device}); there is no CPU fallback")
    return ref


def _frames(frame):
    """``[3,H,W]`` / ``[B,3,H,W]`` of any float dtype -> contiguous fp32 ``[B,3,H,W]``."""
    if frame.ndim == 3:
        frame = frame.unsqueeze(0)
    elif frame.ndim != 4:
        raise ValueError(f"unsupported ndim {frame.ndim}")
    if frame.shape[1] != 3:
        raise ValueError(f"autocrop needs RGB frames, got {frame.shape[1]} channels")
    if not frame.is_floating_point():
        raise ValueError(f"autocrop needs float frames in [0, 1], got {frame.dtype}")
    return frame.to(torch.float32).contiguous()


def _passes(tb, lr):
    return (1 if tb else 0) | (2 if lr else 0)


def _workspace(x, flat, passes):
    if flat or not passes & 2:
        return None, 0
    B, _, H, W = x.shape
    n = B * ((H + _BAND - 1) // _BAND) * W * 16
    return torch.empty(n, dtype=torch.uint8, device=x.device), n


def autocrop_stats(x, black_only, count_tb=None, count_lr=None):
    """Add the decisions of every frame of ``x`` ([B,3,H,W] fp32 contiguous, on the device) to the int32 device counters
    ``count_tb`` [H] and / or ``count_lr`` [W]."""
    B, _, H, W = x.shape
    passes = _passes(count_tb is not None, count_lr is not None)
    work, nbytes = _workspace(x, not black_only, passes)
    with torch.cuda.device(x.device):
        _hip.check(_hip.lib().nunif_hip_autocrop_stats(_ptr(x), B, H, W, 0 if black_only else 1, passes, _ptr(count_tb),
                                                       _ptr(count_lr), _ptr(work), nbytes, _hip.current_stream_ptr(x.device)))


def debug_stats(frame, black_only, tb=True, lr=True):
    """The statistic vectors behind the decisions (tests): a dict with ``row_a`` / ``row_b`` [B,H] and ``col_a`` / ``col_b`` [B,W]
    (mean | median and max deviation | fraction) and the counters ``count_tb`` [H] / ``count_lr`` [W] of this call."""
    x = _frames(frame)
    B, _, H, W = x.shape
    dev = x.device
    passes = _passes(tb, lr)
    out = {}
    if tb:
        out["row_a"], out["row_b"] = (torch.empty((B, H), dtype=torch.float32, device=dev) for _ in range(2))
        out["count_tb"] = torch.zeros((H,), dtype=torch.int32, device=dev)
    if lr:
        out["col_a"], out["col_b"] = (torch.empty((B, W), dtype=torch.float32, device=dev) for _ in range(2))
        out["count_lr"] = torch.zeros((W,), dtype=torch.int32, device=dev)
    work, nbytes = _workspace(x, not black_only, passes)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().nunif_hip_autocrop_debug_stats(
            _ptr(x), B, H, W, 0 if black_only else 1, passes, _ptr(out.get("count_tb")), _ptr(out.get("count_lr")), _ptr(work),
            nbytes, _ptr(out.get("row_a")), _ptr(out.get("row_b")), _ptr(out.get("col_a")), _ptr(out.get("col_b")),
            _hip.current_stream_ptr(dev)))
    return out


def crop_pad(frame, out_h, out_w, y0, x0, pad_top, pad_left, win_h, win_w, pad_value=0.0):
    """``out[..., pad_top + i, pad_left + j] = frame[..., y0 + i, x0 + j]`` over the window, ``pad_value`` elsewhere; ``frame``
    is ``[C,H,W]`` or ``[B,C,H,W]`` of a float dtype on the device, the result is contiguous and of the same dtype."""
    if not frame.is_floating_point():
        raise ValueError(f"autocrop needs float frames, got {frame.dtype}")
    src = frame.to(torch.float32).contiguous()
    sH, sW = src.shape[-2:]
    n = src.numel() // (sH * sW)
    dst = torch.empty(tuple(src.shape[:-2]) + (out_h, out_w), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _hip.check(_hip.lib().nunif_hip_autocrop_crop_pad(_ptr(src), _ptr(dst), n, sH, sW, out_h, out_w, y0, x0, pad_top, pad_left,
                                                          win_h, win_w, float(pad_value), _hip.current_stream_ptr(src.device)))
    return dst.to(frame.dtype)


def _span_without_border(is_border):
    """The slice that keeps everything between the first and the last entry of a flat bool mask that is NOT a border.  An end
    that already sits on the frame edge is ``None``; a mask that is all border or all content asks for no crop at all."""
    n = is_border.numel()
    content = torch.nonzero(torch.logical_not(is_border.reshape(n)), as_tuple=False).reshape(-1)
    if content.numel() in (0, n):
        return slice(None, None)
    first, past_last = int(content[0].item()), int(content[-1].item()) + 1
    return slice(first if first > 0 else None, past_last if past_last < n else None)


def _kept_range(s, length):
    """(first kept index, number of entries dropped behind the last kept one) of slice ``s`` on an axis of ``length``."""
    first, stop, _ = s.indices(length)
    return first, max(0, length - stop)


class AutoCropDetector():
    def __init__(self, mode="black", mod=2, frame_variation_threshold=0.95):
        mode = mode.lower()
        if mode not in _TB_MODES | _LR_MODES:
            raise ValueError(f"unknown autocrop mode {mode!r}")
        self.mode, self.mod = mode, mod
        self.frame_variation_threshold = frame_variation_threshold
        self.black_only = mode in _BLACK_MODES
        self.reset()

    def reset(self):
        self.border_count_tb = self.border_count_lr = None
        self.frame_count = 0

    def _update_on_host(self, ref, frame):
        """One host frame through the reference's own ``detect_*`` (only while ``install()`` is active)."""
        for attr, wanted, fn in (("border_count_tb", _TB_MODES, ref.detect_tb), ("border_count_lr", _LR_MODES, ref.detect_lr)):
            if self.mode not in wanted:
                continue
            hits = fn(frame, black_only=self.black_only).int()
            have = getattr(self, attr)
            if have is not None:
                assert have.shape == hits.shape
                hits = have + hits
            setattr(self, attr, hits)
        self.frame_count += 1

    def update(self, frame):
        """Add one frame ``[3,H,W]`` or a batch ``[B,3,H,W]`` to the border counters: a fixed number of launches for the whole
        batch, no host sync.  The counters live on the frame's device as int32 ``[1,H,1]`` and ``[1,1,W]``."""
        ref = _reference("AutoCropDetector", frame, "AutoCropDetector.update")
        if ref is not None:
            assert frame.ndim in (3, 4)
            for f in (frame if frame.ndim == 4 else [frame]):
                self._update_on_host(ref, f)
            return
        x = _frames(frame)
        B, _, H, W = x.shape
        if self.mode in _TB_MODES:
            if self.border_count_tb is None:
                self.border_count_tb = torch.zeros((1, H, 1), dtype=torch.int32, device=x.device)
            assert self.border_count_tb.shape == (1, H, 1)
        if self.mode in _LR_MODES:
            if self.border_count_lr is None:
                self.border_count_lr = torch.zeros((1, 1, W), dtype=torch.int32, device=x.device)
            assert self.border_count_lr.shape == (1, 1, W)
        autocrop_stats(x, self.black_only, self.border_count_tb, self.border_count_lr)
        self.frame_count += B

    def _host_counts(self):
        """Both counters on the host, in one copy."""
        counts = [c for c in (self.border_count_tb, self.border_count_lr) if c is not None]
        flat = torch.cat([c.flatten() for c in counts]).cpu()
        out, o = [], 0
        for c in (self.border_count_tb, self.border_count_lr):
            if c is None:
                out.append(None)
            else:
                out.append(flat[o:o + c.numel()].view(c.shape))
                o += c.numel()
        return out

    def get_crop(self, frame_variation_threshold=None):
        """(row slice, column slice) of what is not a border in at least ``frame_variation_threshold`` of the frames seen.  The
        share is the reference's fp32 division, compared as fp32, on the host."""
        threshold = frame_variation_threshold or self.frame_variation_threshold
        keep_rows = keep_cols = slice(None)
        if self.frame_count > 0:
            count_tb, count_lr = self._host_counts()
            if count_tb is not None:
                keep_rows = self.apply_mod(self.mask_to_slice_tb(count_tb / self.frame_count >= threshold), self.mod)
            if count_lr is not None:
                keep_cols = self.apply_mod(self.mask_to_slice_lr(count_lr / self.frame_count >= threshold), self.mod)
        return keep_rows, keep_cols

    @classmethod
    def detect(cls, frame, mode="black", mod=2):
        ref = _reference("AutoCropDetector", frame, "AutoCropDetector.detect")
        if ref is not None:
            return ref.detect(frame, mode=mode, mod=mod)
        assert frame.ndim == 3 or (frame.ndim == 4 and frame.shape[0] == 1), "detect takes one frame"
        # one frame: border_count / 1 >= 1.0 is the frame's own mask
        det = cls(mode=mode, mod=mod, frame_variation_threshold=1.0)
        det.update(frame)
        return det.get_crop()

    @staticmethod
    def apply_mod(slice_value, mod):
        """Shrink a slice so that both ends are multiples of ``mod``: the start moves up, the stop moves down."""
        lo, hi = slice_value.start, slice_value.stop
        if lo is not None:
            lo = -(-lo // mod) * mod
        if hi is not None:
            hi = hi // mod * mod
        return slice(lo, hi)

    @classmethod
    def _detect(cls, x, black_only, tb):
        ref = _reference("AutoCropDetector", x, "AutoCropDetector.detect_tb" if tb else "AutoCropDetector.detect_lr")
        if ref is not None:
            return (ref.detect_tb if tb else ref.detect_lr)(x, black_only=black_only)
        frames = _frames(x)
        B, _, H, W = frames.shape
        counts = torch.zeros((B, H if tb else W), dtype=torch.int32, device=frames.device)
        for i in range(B):                                        # one counter per frame: the counter IS the frame's mask
            autocrop_stats(frames[i:i + 1], black_only, counts[i] if tb else None, None if tb else counts[i])
        mask = (counts > 0).view((B, 1, H, 1) if tb else (B, 1, 1, W))
        return mask[0] if x.ndim == 3 else mask

    @classmethod
    def detect_tb(cls, x, black_only):
        return cls._detect(x, black_only, True)

    @classmethod
    def detect_lr(cls, x, black_only):
        return cls._detect(x, black_only, False)

    @classmethod
    def mask_to_slice_tb(cls, mask):
        assert mask.ndim == 3 and mask.shape[0] == 1 and mask.shape[2] == 1, "a row mask is [1, H, 1]"
        return _span_without_border(mask)

    @classmethod
    def mask_to_slice_lr(cls, mask):
        assert mask.ndim == 3 and mask.shape[0] == 1 and mask.shape[1] == 1, "a column mask is [1, 1, W]"
        return _span_without_border(mask)


def autocrop_analyze_video(video_file, mode="black", mod=2, max_frames=40, vf="", device="cuda", batch_size=2, stop_event=None,
                           suspend_event=None, tqdm_fn=None, tqdm_title=None):
    """Sample up to ``max_frames`` key frames of ``video_file`` through the reference's decoder (``nunif.utils.video``: PyAV) into
    the engine's detector; returns ``(row slice, column slice, frame height, frame width)``."""
    try:
        import av  # noqa: F401
        import nunif.utils.video as VU
    except Exception as e:
        raise RuntimeError("autocrop_analyze_video decodes with the reference's nunif.utils.video: it needs PyAV and the nunif "
                           f"checkout on sys.path ({e!r})") from e
    detector = AutoCropDetector(mode=mode, mod=mod)
    largest = [0, 0]                                              # height, width over the batches seen

    def on_batch(x):
        largest[0], largest[1] = max(largest[0], x.shape[-2]), max(largest[1], x.shape[-1])
        detector.update(x)

    pool = VU.FrameCallbackPool(on_batch, batch_size=batch_size, device=device, max_workers=0)
    VU.sample_frames(video_file, pool, num_samples=max_frames, keyframe_only=True, vf=vf, stop_event=stop_event,
                     suspend_event=suspend_event, tqdm_fn=tqdm_fn, title=tqdm_title or "AutoCrop Analysis")
    return (*detector.get_crop(), largest[0], largest[1])


class AutoCrop():
    def __init__(self, slice_h, slice_w, pad, pad_value, crop_range, uncrop_enabled):
        self.slice_h, self.slice_w = slice_h, slice_w
        self.pad, self.pad_value = pad, pad_value
        self.crop_range = crop_range
        self.uncrop_enabled = uncrop_enabled

    def get_slice(self):
        return self.slice_h, self.slice_w

    def get_pad(self):
        return self.pad

    def get_crop(self):
        return self.crop_range

    @staticmethod
    def calc_pad(slice_h, slice_w, H, W):
        """What ``F.pad`` needs to undo the crop: (left, right, top, bottom)."""
        top, bottom = _kept_range(slice_h, H)
        left, right = _kept_range(slice_w, W)
        return (left, right, top, bottom)

    @staticmethod
    def calc_crop(slice_h, slice_w, H, W):
        """The crop as ffmpeg's ``crop=`` filter takes it, (x, y, width, height), or ``None`` for the whole frame."""
        top, bottom = _kept_range(slice_h, H)
        left, right = _kept_range(slice_w, W)
        if top == bottom == left == right == 0:
            return None
        return (left, top, W - left - right, H - top - bottom)

    @classmethod
    def _from_slices(cls, slice_h, slice_w, H, W, pad_value, uncrop_enabled):
        return cls(slice_h=slice_h, slice_w=slice_w, pad=cls.calc_pad(slice_h, slice_w, H, W), pad_value=pad_value,
                   crop_range=cls.calc_crop(slice_h, slice_w, H, W), uncrop_enabled=uncrop_enabled)

    @classmethod
    def from_image(cls, frame, mode="black", mod=2, pad_value=0, uncrop_enabled=True):
        if frame.ndim == 4:
            assert frame.shape[0] == 1, "from_image takes one frame, not a batch"
            frame = frame[0]
        slice_h, slice_w = AutoCropDetector.detect(frame, mode=mode, mod=mod)
        return cls._from_slices(slice_h, slice_w, frame.shape[-2], frame.shape[-1], pad_value, uncrop_enabled)

    @classmethod
    def from_video_file(cls, video_file, mode="black", mod=2, pad_value=0, uncrop_enabled=True, max_frames=40, vf="",
                        device="cuda", batch_size=2, stop_event=None, suspend_event=None, tqdm_fn=None, tqdm_title=None):
        slice_h, slice_w, H, W = autocrop_analyze_video(
            video_file=video_file, mode=mode, mod=mod, max_frames=max_frames, vf=vf, device=device, batch_size=batch_size,
            stop_event=stop_event, suspend_event=suspend_event, tqdm_fn=tqdm_fn, tqdm_title=tqdm_title)
        return cls._from_slices(slice_h, slice_w, H, W, pad_value, uncrop_enabled)

    def crop(self, frame):
        """``frame[..., slice_h, slice_w]`` with contiguous planes (every engine entry wants them): a copy of the window, or the
        frame itself where the window is the whole frame and the planes are contiguous already."""
        if frame.ndim not in (3, 4):
            raise ValueError(f"ndim={frame.ndim} is not supported")
        ref = _reference("AutoCrop", frame, "AutoCrop.crop")
        if ref is not None:
            return ref.crop(self, frame)
        H, W = frame.shape[-2:]
        y0, y1, _ = self.slice_h.indices(H)
        x0, x1, _ = self.slice_w.indices(W)
        if (y0, y1, x0, x1) == (0, H, 0, W) and frame.is_contiguous():
            return frame                                          # no bars found: nothing to move
        if y1 <= y0 or x1 <= x0 or frame.numel() == 0:
            return frame[..., self.slice_h, self.slice_w].contiguous()          # an empty window: nothing to copy
        return crop_pad(frame, y1 - y0, x1 - x0, y0, x0, 0, 0, y1 - y0, x1 - x0)

    def uncrop(self, frame):
        if not self.uncrop_enabled:
            return frame
        ref = _reference("AutoCrop", frame, "AutoCrop.uncrop")
        if ref is not None:
            return ref.uncrop(self, frame)
        if frame.ndim not in (3, 4):
            raise ValueError(f"ndim={frame.ndim} is not supported")
        left, right, top, bottom = self.pad
        assert min(self.pad) >= 0
        if max(self.pad) == 0 and frame.is_contiguous():
            return frame
        H, W = frame.shape[-2:]
        return crop_pad(frame, H + top + bottom, W + left + right, 0, 0, top, left, H, W, pad_value=self.pad_value)


class AutoCropDummy():
    """The crop that crops nothing (``--autocrop`` not given)."""

    def __init__(self):
        pass

    def crop(self, frame):
        return frame

    def uncrop(self, frame):
        return frame
