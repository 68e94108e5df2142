"""Lossless PNG frame encoder on the HIP engine (nunif_amd/csrc/png.hip): device frames in, the bytes of PNG files out.

What crosses to the host per call is 4 bytes per frame (the body lengths) and then exactly the bytes of the bodies, copied into
pinned memory; the image itself never leaves the device.  The signature, IHDR and tEXt chunks are written on the host.
DESIGN.md ("PNG frame encoder") defines the stream; every PNG decoder reads it.

The waifu2x image route (nunif_amd/waifu2x/ui_utils.py) adds three forms whose colour and alpha arrive as two planar fp32
tensors, the way ``Waifu2x.convert`` returns them: RGBA 8, grey 8 and grey + alpha 8, and the ``gAMA`` chunk.

There is no CPU fallback: a host tensor raises.
"""
import ctypes
import struct
import zlib

import torch

from ... import _hip

MAX_DIM, MAX_BATCH = 8192, 16
RGB8_F32, RGB8_U8, GRAY16_F32 = 0, 1, 2
RGBA8_F32, GRAY8_F32, GRAYA8_F32 = 4, 5, 6                       # 3 names no form
PLANES_FORMS = (RGBA8_F32, GRAY8_F32, GRAYA8_F32)
BPP = {RGB8_F32: 3, RGB8_U8: 3, GRAY16_F32: 2, RGBA8_F32: 4, GRAY8_F32: 1, GRAYA8_F32: 2}
N_SYMBOLS, SYMBOL_STRIDE = 335, 336
# rows per stripe when the caller names none: the fastest setting of profiles/png.txt whose file stays within 2 % of the smallest
# on every frame measured there (4 and 8 are faster on noisy frames and cost 15 % and 7 % on a posterised one)
DEFAULT_STRIPE_ROWS = 32


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _text_items(text):
    items = [(str(k), str(v)) for k, v in (text or {}).items()]
    for k, v in items:
        k.encode("latin-1"), v.encode("latin-1")                 # tEXt holds Latin-1
        if "\0" in k or "\0" in v:
            raise ValueError("a PNG text entry cannot hold a zero byte")
    return items


def gamma_chunk(gamma):
    """The ``gAMA`` chunk of ``gamma`` in PNG units (100 000 x the exponent), as ``PngInfo.add(b"gAMA", ...)`` writes it
    (nunif/utils/pil_io.py:294-296, reference)."""
    gamma = int(gamma)
    if not 0 <= gamma < 2 ** 31:
        raise ValueError(f"gamma {gamma} is outside a PNG four-byte unsigned integer")
    data = b"gAMA" + struct.pack(">I", gamma)
    return struct.pack(">I", 4) + data + struct.pack(">I", zlib.crc32(data))


def header(H, W, form, text=None, gamma=None):
    """The bytes in front of the first IDAT: signature, IHDR, ``gAMA`` where ``gamma`` is given, one tEXt chunk per entry of
    ``text``.  Host only."""
    if gamma is not None:
        head = header(H, W, form, text)
        return head[:33] + gamma_chunk(gamma) + head[33:]          # signature 8 + IHDR 25
    items = _text_items(text)
    keys = (ctypes.c_char_p * max(1, len(items)))(*[k.encode("latin-1") for k, _ in items])
    vals = (ctypes.c_char_p * max(1, len(items)))(*[v.encode("latin-1") for _, v in items])
    cap = 8 + 25 + sum(12 + len(k) + 1 + len(v) for k, v in items)
    buf = (ctypes.c_uint8 * cap)()
    n = _hip.lib().nunif_hip_png_header(H, W, int(form), keys, vals, len(items), buf, cap)
    if n < 0:
        _hip.check(int(n))
    return bytes(buf[:n])


def stripe_rows_for(H, stripe_rows=None):
    return max(1, min(int(H), DEFAULT_STRIPE_ROWS if stripe_rows is None else int(stripe_rows)))


def max_bytes(H, W, form, stripe_rows=None):
    """An upper bound of the body (IDATs and IEND) of one H x W frame (-1: a frame the encoder refuses).  Host only."""
    return int(_hip.lib().nunif_hip_png_max_bytes(H, W, int(form), stripe_rows_for(H, stripe_rows)))


def workspace_bytes(B, H, W, form, stripe_rows=None):
    return int(_hip.lib().nunif_hip_png_workspace_bytes(B, H, W, int(form), stripe_rows_for(H, stripe_rows)))


def _frames(frame):
    """-> (x contiguous [B,...], form, B, H, W, single)"""
    if not isinstance(frame, torch.Tensor) or frame.device.type != "cuda":
        raise RuntimeError("PngEncoder needs a ROCm device tensor "
                           f"(got {getattr(frame, 'device', type(frame))}); there is no CPU fallback")
    if frame.ndim not in (3, 4):
        raise ValueError(f"unsupported ndim {frame.ndim}")
    x = frame if frame.ndim == 4 else frame.unsqueeze(0)
    if x.dtype == torch.uint8:
        if x.shape[3] != 3:
            raise ValueError(f"uint8 frames are [B,H,W,3], got {tuple(x.shape)}")
        form, (B, H, W, _) = RGB8_U8, x.shape
    elif x.is_floating_point():
        if x.shape[1] not in (1, 3):
            raise ValueError(f"float frames are [B,3,H,W] (RGB) or [B,1,H,W] (16-bit grey), got {tuple(x.shape)}")
        form, (B, _, H, W) = (RGB8_F32 if x.shape[1] == 3 else GRAY16_F32), x.shape
        x = x.to(torch.float32)
    else:
        raise ValueError(f"the PNG encoder takes uint8 or float frames, got {x.dtype}")
    if not (1 <= B <= MAX_BATCH and 1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"a batch of {B} frames of {H} x {W} is outside B <= {MAX_BATCH}, H, W <= {MAX_DIM}")
    return x.contiguous(), form, B, H, W, frame.ndim == 3


def _planes(frame, alpha, gray):
    """The forms with ``alpha`` or ``gray``: -> (colour contiguous [B,C,H,W] f32, alpha contiguous [B,1,H,W] f32 or None, form,
    B, H, W, single)"""
    if not isinstance(frame, torch.Tensor) or frame.device.type != "cuda":
        raise RuntimeError("PngEncoder needs a ROCm device tensor "
                           f"(got {getattr(frame, 'device', type(frame))}); there is no CPU fallback")
    if frame.ndim not in (3, 4):
        raise ValueError(f"unsupported ndim {frame.ndim}")
    if not frame.is_floating_point():
        raise ValueError(f"alpha= and gray= go with float planar frames, got {frame.dtype}")
    x = frame if frame.ndim == 4 else frame.unsqueeze(0)
    B, C, H, W = x.shape
    if C not in (1, 3) or (C == 1 and not gray):
        raise ValueError(f"float frames are [B,3,H,W], or [B,1,H,W] with gray=True, got {tuple(x.shape)}")
    if not (1 <= B <= MAX_BATCH and 1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"a batch of {B} frames of {H} x {W} is outside B <= {MAX_BATCH}, H, W <= {MAX_DIM}")
    a = None
    if alpha is not None:
        if not isinstance(alpha, torch.Tensor) or not alpha.is_floating_point():
            raise ValueError("alpha is a float tensor [B,1,H,W] (or [1,H,W] with a frame of three dimensions)")
        if alpha.device != frame.device:
            raise RuntimeError(f"the frame is on {frame.device}, its alpha on {alpha.device}")
        a = alpha if alpha.ndim == 4 else alpha.unsqueeze(0)
        if alpha.ndim != frame.ndim or tuple(a.shape) != (B, 1, H, W):
            raise ValueError(f"alpha {tuple(alpha.shape)} does not fit the frame {tuple(frame.shape)}")
        a = a.to(torch.float32).contiguous()
    form = (GRAYA8_F32 if gray else RGBA8_F32) if a is not None else GRAY8_F32
    return x.to(torch.float32).contiguous(), a, form, B, H, W, frame.ndim == 3


def _sources(frame, alpha, gray):
    """-> (x, alpha or None, form, B, H, W, single) for every form"""
    if alpha is None and not gray:
        x, form, B, H, W, single = _frames(frame)
        return x, None, form, B, H, W, single
    return _planes(frame, alpha, gray)


def debug_filtered(frame, alpha=None, gray=False):
    """The filtered bytes, uint8 ``[B, H, 1 + W * bpp]`` on the device, the filter type in column 0 (tests)."""
    x, a, form, B, H, W, _ = _sources(frame, alpha, gray)
    out = torch.empty((B, H, 1 + W * BPP[form]), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        if form in PLANES_FORMS:
            _hip.check(_hip.lib().nunif_hip_png_debug_filtered_planes(_ptr(x), _ptr(a) if a is not None else None, x.shape[1], form,
                                                                      B, H, W, _ptr(out), _hip.current_stream_ptr(x.device)))
        else:
            _hip.check(_hip.lib().nunif_hip_png_debug_filtered(_ptr(x), form, B, H, W, _ptr(out),
                                                               _hip.current_stream_ptr(x.device)))
    return out


def debug_codes(frame, stripe_rows=None, alpha=None, gray=False):
    """(histograms, code lengths): int32 ``[B, stripes, 335]`` each, on the device: 286 literal / length symbols, 30 distance
    symbols, 19 code-length symbols (tests).  With ``alpha`` the two sources go in as one tensor, the alpha plane last; a grey
    frame is one plane here."""
    x, a, form, B, H, W, _ = _sources(frame, alpha, gray)
    if form in (GRAY8_F32, GRAYA8_F32) and x.shape[1] != 1:
        raise ValueError("debug_codes takes the grey forms from one plane")
    if a is not None:
        x = torch.cat([x, a], dim=1).contiguous()
    S = stripe_rows_for(H, stripe_rows)
    stripes = -(-H // S)
    need = _hip.lib().nunif_hip_png_workspace_bytes(B, H, W, form, S)
    if need < 0:
        raise ValueError(f"the PNG encoder refuses B={B} H={H} W={W} stripe_rows={S}")
    work = torch.empty(need, dtype=torch.uint8, device=x.device)
    hist = torch.empty((B, stripes, SYMBOL_STRIDE), dtype=torch.int32, device=x.device)
    lens = torch.empty_like(hist)
    with torch.cuda.device(x.device):
        _hip.check(_hip.lib().nunif_hip_png_debug_codes(_ptr(x), form, B, H, W, S, _ptr(hist), _ptr(lens), _ptr(work),
                                                        _hip.current_stream_ptr(x.device)))
    return hist[..., :N_SYMBOLS], lens[..., :N_SYMBOLS]


class PngEncoder():
    """Keeps the workspace, the output buffer and the pinned host buffer of one device, and grows them by size."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"PngEncoder needs a ROCm device (got {self.device}); there is no CPU fallback")
        self._work = self._out = self._pinned = None
        self._lens = torch.empty(MAX_BATCH, dtype=torch.int32, device=self.device)

    def _grow(self, name, nbytes, **kw):
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8, **kw)
            setattr(self, name, buf)
        return buf

    def encode_device(self, x, form, stripe_rows, capacity=None, alpha=None):
        """The launches alone: x contiguous on the device -> (out buffer, capacity per frame, lengths [B] i32), all on the
        device; nothing is synchronised.  ``capacity`` below the bound makes a too long body answer -1.  The forms 4..6 take
        ``x`` [B,C,H,W] f32 and, where they have one, ``alpha`` [B,1,H,W] f32, both contiguous."""
        if form == RGB8_U8:
            B, H, W, _ = x.shape
        else:
            B, _, H, W = x.shape
        bound = _hip.lib().nunif_hip_png_max_bytes(H, W, form, stripe_rows)
        need = _hip.lib().nunif_hip_png_workspace_bytes(B, H, W, form, stripe_rows)
        if bound < 0 or need < 0:
            raise ValueError(f"the PNG encoder refuses B={B} H={H} W={W} form={form} stripe_rows={stripe_rows}")
        capacity = bound if capacity is None else int(capacity)
        work = self._grow("_work", need, device=self.device)
        out = self._grow("_out", max(1, B * capacity), device=self.device)
        with torch.cuda.device(self.device):
            if form in PLANES_FORMS:
                _hip.check(_hip.lib().nunif_hip_png_encode_planes(_ptr(x), _ptr(alpha) if alpha is not None else None, x.shape[1],
                                                                  form, B, H, W, stripe_rows, _ptr(out), capacity,
                                                                  _ptr(self._lens), _ptr(work),
                                                                  _hip.current_stream_ptr(self.device)))
            else:
                _hip.check(_hip.lib().nunif_hip_png_encode(_ptr(x), form, B, H, W, stripe_rows, _ptr(out), capacity,
                                                           _ptr(self._lens), _ptr(work), _hip.current_stream_ptr(self.device)))
        return out, capacity, self._lens[:B]

    def encode(self, frame, text=None, stripe_rows=None, *, alpha=None, gray=False, gamma=None):
        """``frame`` [3,H,W] / [1,H,W] float or [H,W,3] uint8 -> ``bytes``; with a batch dimension -> a list of B ``bytes``.
        Each is a whole PNG file: the host-written header (with the ``text`` entries) and the device-written body.  ``text`` is a
        dict for all frames or a list of one dict per frame.

        ``alpha`` (float [1,H,W], or [B,1,H,W] with a batch; the same device) makes the file RGBA; ``gray=True`` makes it 8-bit
        grey, or grey + alpha: three planes go through PIL's ``convert("L")`` on their quantised bytes, one plane is quantised as
        it is.  Without either a call means what it always did: one float plane is 16-bit grey.  ``gamma`` (PNG units) adds a
        ``gAMA`` chunk behind IHDR."""
        x, a, form, B, H, W, single = _sources(frame, alpha, gray)
        if x.device != self.device:
            raise RuntimeError(f"this encoder belongs to {self.device}, the frame is on {x.device}")
        texts = list(text) if isinstance(text, (list, tuple)) else [text] * B
        if len(texts) != B:
            raise ValueError(f"{len(texts)} text entries for {B} frames")
        heads = [header(H, W, form, t, gamma) for t in texts]
        out, capacity, lens = self.encode_device(x, form, stripe_rows_for(H, stripe_rows), alpha=a)
        lens = lens.cpu().tolist()                                 # the one read of 4 x B bytes; waits for the launches
        if min(lens) < 0:
            raise RuntimeError(f"PNG body longer than its buffer of {capacity} bytes")
        pinned = self._grow("_pinned", sum(lens), pin_memory=True)
        o = 0
        for b, n in enumerate(lens):                               # exactly the used bytes
            pinned[o:o + n].copy_(out[b * capacity:b * capacity + n], non_blocking=True)
            o += n
        torch.cuda.current_stream(self.device).synchronize()
        host = pinned[:o].numpy().tobytes()
        files, o = [], 0
        for head, n in zip(heads, lens):
            files.append(head + host[o:o + n])
            o += n
        return files[0] if single else files
