"""The restatement of the PNG encoder's three plane forms (RGBA 8, grey 8, grey + alpha 8: nunif_amd/csrc/png.hip forms 4..6) in
plain Python / numpy.  What does not depend on the form comes from tests/png_ref.py as it is: the row filter, the deflate stripes,
CRC-32 and Adler-32.  Here: the quantisation of the planar sources (the reference's quantize256 on every plane; PIL's integer
``convert("L")`` on the quantised bytes where a grey form has three colour planes), the header with the colour types 6 / 0 / 4 and
the ``gAMA`` chunk, the body and the bound.
"""
import struct

import numpy as np

import png_ref as R

RGBA8_F32, GRAY8_F32, GRAYA8_F32 = 4, 5, 6
FORMS = [RGBA8_F32, GRAY8_F32, GRAYA8_F32]
BPP = {RGBA8_F32: 4, GRAY8_F32: 1, GRAYA8_F32: 2}
COLOUR_TYPE = {RGBA8_F32: 6, GRAY8_F32: 0, GRAYA8_F32: 4}
PIL_MODE = {RGBA8_F32: "RGBA", GRAY8_F32: "L", GRAYA8_F32: "LA"}
HAS_ALPHA = {RGBA8_F32: True, GRAY8_F32: False, GRAYA8_F32: True}


def quantize256(x):
    """nunif/transforms/functional.py:9-12 (reference): x 255, round half to even, clamp to 0..255; fp32 throughout."""
    v = np.rint(np.asarray(x, np.float32) * np.float32(255))
    return np.clip(v, 0, 255).astype(np.uint8)


def pil_l(r, g, b):
    """PIL's ``Image.convert("L")`` on bytes (ITU-R 601-2 luma in 16-bit fixed point, rounded)."""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def quantise_planes(colour, alpha, form):
    """One frame -> its raw PNG rows, uint8 [H, W * bpp].  ``colour`` f32 [3,H,W] or [1,H,W], ``alpha`` f32 [1,H,W] or None."""
    c = quantize256(colour)
    if form == RGBA8_F32:
        assert c.shape[0] == 3
        planes = [c[0], c[1], c[2]]
    else:
        planes = [pil_l(c[0], c[1], c[2]) if c.shape[0] == 3 else c[0]]
    assert (alpha is not None) == HAS_ALPHA[form]
    if alpha is not None:
        planes.append(quantize256(alpha)[0])
    pix = np.stack(planes, axis=2)                                        # [H, W, bpp]
    return np.ascontiguousarray(pix).reshape(pix.shape[0], -1)


def pixels(colour, alpha, form):
    """What a decoder has to give back: uint8 [H,W,4], [H,W] or [H,W,2]."""
    raw = quantise_planes(colour, alpha, form)
    return raw if form == GRAY8_F32 else raw.reshape(raw.shape[0], -1, BPP[form])


def gamma_chunk(gamma):
    return R.chunk(b"gAMA", struct.pack(">I", gamma))


def header(H, W, form, text=None, gamma=None):
    """Signature, IHDR, gAMA where a gamma is given, one tEXt chunk per entry of ``text``.  Takes the old forms too."""
    if form in BPP:
        out = R.SIGNATURE + R.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[form], 0, 0, 0))
    else:
        out = R.header(H, W, form)
    if gamma is not None:
        out += gamma_chunk(gamma)
    for k, v in (text or {}).items():
        out += R.chunk(b"tEXt", str(k).encode("latin-1") + b"\0" + str(v).encode("latin-1"))
    return out


def filtered(colour, alpha, form):
    return R.filter_rows(quantise_planes(colour, alpha, form), BPP[form])


def body(colour, alpha, form, stripe_rows):
    """The IDAT chunks, one per stripe, and IEND."""
    bpp = BPP[form]
    f = filtered(colour, alpha, form)
    parts = R.stripes(f, stripe_rows)
    out = b""
    for k, d in enumerate(parts):
        last = k == len(parts) - 1
        data = (b"\x78\x01" if k == 0 else b"") + R.deflate_stripe(d, bpp, last)
        if last:
            data += struct.pack(">I", R.adler32(f.tobytes()))
        out += R.chunk(b"IDAT", data)
    return out + R.chunk(b"IEND", b"")


def encode(colour, alpha, form, stripe_rows, text=None, gamma=None):
    H, W = np.asarray(colour).shape[1:]
    return header(H, W, form, text, gamma) + body(colour, alpha, form, stripe_rows)


def stripe_codes(colour, alpha, form, stripe_rows):
    bpp = BPP[form]
    return [R.StripeCodes(R.tokens(d, bpp)) for d in R.stripes(filtered(colour, alpha, form), stripe_rows)]


def max_bytes(H, W, form, stripe_rows):
    """tests/png_ref.py max_bytes with the row of the form: 1 + W x bpp filtered bytes."""
    if form not in BPP:
        return R.max_bytes(H, W, form, stripe_rows)
    if not (1 <= H <= R.MAX_DIM and 1 <= W <= R.MAX_DIM and 1 <= stripe_rows <= H):
        return -1
    row = 1 + W * BPP[form]
    total = 2 + 4 + 12
    for r in range(0, H, stripe_rows):
        n = min(stripe_rows, H - r) * row
        total += (3 + 14 + 57 + 316 * 7 + 15 * n + 15 + 3 + 7) // 8 + 4 + 12
    return total


def workspace_bytes(B, H, W, form, stripe_rows):
    """The workspace DESIGN.md lays out: per frame and stripe the filtered bytes (a stripe's slot padded to 16 bytes), per row two
    u32 Adler sums, per stripe 336 i32 of histogram and of code lengths, 288 u32 of codes, 160 u32 of block header and 4 i32 of
    sizes, per frame 4 u32; every part starts on a multiple of 256 bytes."""
    bpp = BPP.get(form) or R.BPP.get(form)
    if bpp is None or not (1 <= B <= R.MAX_BATCH and 1 <= H <= R.MAX_DIM and 1 <= W <= R.MAX_DIM and 1 <= stripe_rows <= H):
        return -1
    ns = B * -(-H // stripe_rows)
    slot = -(-((1 + W * bpp) * stripe_rows) // 16) * 16
    total = 0
    for part in (ns * slot, B * H * 8, ns * 336 * 4, ns * 336 * 4, ns * 288 * 4, ns * 160 * 4, ns * 16, B * 16):
        total = -(-(total + part) // 256) * 256
    return total
