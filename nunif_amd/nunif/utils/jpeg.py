"""Baseline JPEG frame encoder on the HIP engine (nunif_amd/csrc/jpeg.hip): a device frame in, the bytes of a JFIF stream out.

What crosses to the host per call is 4 bytes per frame (the stream lengths) and then exactly the bytes of the streams, copied into
pinned memory; the uint8 image never leaves the device.  DESIGN.md ("JPEG frame encoder") defines the encoder; every baseline
decoder reads its streams (they carry restart markers, which are the encoder's unit of parallelism).

There is no CPU fallback: a host tensor raises.
"""
import ctypes

import torch

from ... import _hip

MAX_DIM, MAX_BATCH, MAX_RESTART = 8192, 16, 65535
SUBSAMPLINGS = {"420": 420, "444": 444, 420: 420, 444: 444, "4:2:0": 420, "4:4:4": 444}
# MCUs per restart interval when the caller names none: chosen from the table in profiles/jpeg.txt
DEFAULT_RESTART_MCUS = 8


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def quant_tables(quality):
    """(luma, chroma): the IJG-scaled Annex K tables of ``quality`` as two lists of 64, natural order.  Host only."""
    luma, chroma = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 64)()
    _hip.check(_hip.lib().nunif_hip_jpeg_quant_tables(int(quality), luma, chroma))
    return list(luma), list(chroma)


def header(H, W, quality, subsampling=420, restart_mcus=DEFAULT_RESTART_MCUS):
    """The bytes in front of the entropy-coded scan.  Host only."""
    buf = (ctypes.c_uint8 * 1024)()
    n = _hip.lib().nunif_hip_jpeg_header(H, W, int(quality), SUBSAMPLINGS[subsampling], restart_mcus, buf, 1024)
    if n < 0:
        _hip.check(int(n))
    return bytes(buf[:n])


def max_bytes(H, W, subsampling=420, restart_mcus=DEFAULT_RESTART_MCUS):
    """An upper bound of the stream of one H x W frame (-1: a frame the encoder refuses).  Host only."""
    return int(_hip.lib().nunif_hip_jpeg_max_bytes(H, W, SUBSAMPLINGS[subsampling], restart_mcus))


def workspace_bytes(B, H, W, subsampling=420, restart_mcus=DEFAULT_RESTART_MCUS):
    return int(_hip.lib().nunif_hip_jpeg_workspace_bytes(B, H, W, SUBSAMPLINGS[subsampling], restart_mcus))


def _frames(frame):
    if not isinstance(frame, torch.Tensor) or frame.device.type != "cuda":
        raise RuntimeError("JpegEncoder needs a ROCm device tensor "
                           f"(got {getattr(frame, 'device', type(frame))}); there is no CPU fallback")
    if frame.ndim not in (3, 4):
        raise ValueError(f"unsupported ndim {frame.ndim}")
    x = frame if frame.ndim == 4 else frame.unsqueeze(0)
    if x.shape[1] != 3:
        raise ValueError(f"the JPEG encoder needs RGB frames, got {x.shape[1]} channels")
    if not x.is_floating_point():
        raise ValueError(f"the JPEG encoder needs float frames in [0, 1], got {x.dtype}")
    B, _, H, W = x.shape
    if not (1 <= B <= MAX_BATCH and 1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"a batch of {B} frames of {H} x {W} is outside B <= {MAX_BATCH}, H, W <= {MAX_DIM}")
    return x.to(torch.float32).contiguous()


def debug_coefficients(frame, quality=75, subsampling="420"):
    """The quantised coefficients in scan order, int16 ``[B, blocks, 64]`` on the device (tests)."""
    x = _frames(frame)
    B, _, H, W = x.shape
    ss = SUBSAMPLINGS[subsampling]
    m = 16 if ss == 420 else 8
    blocks = -(-H // m) * -(-W // m) * (6 if ss == 420 else 3)
    out = torch.empty((B, blocks, 64), dtype=torch.int16, device=x.device)
    with torch.cuda.device(x.device):
        _hip.check(_hip.lib().nunif_hip_jpeg_debug_coefficients(_ptr(x), B, H, W, int(quality), ss, _ptr(out),
                                                                _hip.current_stream_ptr(x.device)))
    return out


class JpegEncoder():
    """Keeps the workspace, the output buffer and the pinned host buffer of one device, and grows them by size."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"JpegEncoder needs a ROCm device (got {self.device}); there is no CPU fallback")
        self._work = self._out = self._pinned = None
        self._lens = torch.empty(MAX_BATCH, dtype=torch.int32, device=self.device)

    def _grow(self, name, nbytes, **kw):
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8, **kw)
            setattr(self, name, buf)
        return buf

    def encode_device(self, x, quality, ss, restart_mcus, capacity=None):
        """The launches alone: x [B,3,H,W] fp32 contiguous on the device -> (out buffer, capacity per frame, lengths [B] i32),
        all on the device; nothing is synchronised.  ``capacity`` below the bound makes a too long stream answer -1."""
        B, _, H, W = x.shape
        bound = _hip.lib().nunif_hip_jpeg_max_bytes(H, W, ss, restart_mcus)
        need = _hip.lib().nunif_hip_jpeg_workspace_bytes(B, H, W, ss, restart_mcus)
        if bound < 0 or need < 0:
            raise ValueError(f"the JPEG encoder refuses B={B} H={H} W={W} subsampling={ss} restart_mcus={restart_mcus}")
        capacity = bound if capacity is None else int(capacity)
        work = self._grow("_work", need, device=self.device)
        out = self._grow("_out", max(1, B * capacity), device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(_hip.lib().nunif_hip_jpeg_encode(_ptr(x), B, H, W, int(quality), ss, restart_mcus, _ptr(out), capacity,
                                                        _ptr(self._lens), _ptr(work), _hip.current_stream_ptr(self.device)))
        return out, capacity, self._lens[:B]

    def encode(self, frame, quality=75, subsampling="420", restart_mcus=None):
        """``frame`` [3,H,W] -> ``bytes``; [B,3,H,W] -> a list of B ``bytes``."""
        x = _frames(frame)
        if x.device != self.device:
            raise RuntimeError(f"this encoder belongs to {self.device}, the frame is on {x.device}")
        ss = SUBSAMPLINGS[subsampling]
        restart_mcus = DEFAULT_RESTART_MCUS if restart_mcus is None else int(restart_mcus)
        out, capacity, lens = self.encode_device(x, quality, ss, restart_mcus)
        lens = lens.cpu().tolist()                                 # the one read of 4 x B bytes; waits for the launches
        if min(lens) < 0:
            raise RuntimeError(f"JPEG stream longer than its buffer of {capacity} bytes")
        pinned = self._grow("_pinned", sum(lens), pin_memory=True)
        o = 0
        for b, n in enumerate(lens):                               # exactly the used bytes
            pinned[o:o + n].copy_(out[b * capacity:b * capacity + n], non_blocking=True)
            o += n
        torch.cuda.current_stream(self.device).synchronize()
        host = pinned[:o].numpy().tobytes()
        streams, o = [], 0
        for n in lens:
            streams.append(host[o:o + n])
            o += n
        return streams if frame.ndim == 4 else streams[0]
