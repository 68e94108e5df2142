"""The baseline JPEG encoder of nunif_amd/csrc/jpeg.hip restated on the CPU (helper, no tests): steps 1-5 of DESIGN.md ("JPEG frame
encoder") in numpy, in float64 or in float32, and step 6 (the entropy coder) and the header in plain Python, written from ITU T.81
(annexes A, B, C, F and K) and the JFIF 1.02 specification.  The tests compare the library with this file and this file with
PIL / libjpeg; the test inputs and the PIL yardsticks live here too, so that the CPU and the GPU tests share them."""
import io

import numpy as np

HEADER_BYTES = 629
MAX_BLOCK_BITS = 22 + 63 * 26

# T.81 figure A.6: zigzag position -> natural index
ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8 if (i // 8 + i % 8) % 2 else i % 8))), dtype=np.int64)

# T.81 tables K.1, K.2 (natural order)
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
CHROMA_Q = np.array([17, 18, 24, 47] + [99] * 4 + [18, 21, 26, 66] + [99] * 4 + [24, 26, 56] + [99] * 5 + [47, 66] + [99] * 6 +
                    [99] * 32, dtype=np.int64)

# T.81 tables K.3 - K.6
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def huffman_codes(bits, vals):
    """T.81 annex C: symbol -> (code, length)."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


DC_CODES = (huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def quant_tables(quality):
    """The IJG scaling of the Annex K tables, clamped to 1..255; natural order."""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def mcu_size(subsampling):
    return {420: 16, 444: 8}[subsampling]


def blocks_per_mcu(subsampling):
    return {420: 6, 444: 3}[subsampling]


def geometry(H, W, subsampling):
    m = mcu_size(subsampling)
    return -(-H // m), -(-W // m)


def interval_bound(mcus, bpm):
    return 2 * ((mcus * bpm * MAX_BLOCK_BITS + 7) // 8) + 2


def max_bytes(H, W, subsampling, restart_mcus):
    my, mx = geometry(H, W, subsampling)
    bpm = blocks_per_mcu(subsampling)
    full, tail = divmod(my * mx, restart_mcus)
    return HEADER_BYTES + full * interval_bound(restart_mcus, bpm) + (interval_bound(tail, bpm) if tail else 0)


def to_uint8_values(x):
    """Step 1, always in fp32: the two operations of the reference's to_uint8 after the clamp."""
    x = np.asarray(x, dtype=np.float32)
    return np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255))


def dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    d = 0.5 * np.cos((2 * n + 1) * k * np.pi / 16)
    d[0] = np.sqrt(1.0 / 8.0)
    return d


def coefficients(x, quality, subsampling, dtype=np.float64):
    """Steps 1-5 on one frame x [3,H,W] in ``dtype``.  Returns (q, quot): the quantised coefficients and the quotients c / Q
    before rounding, both [blocks, 64] in scan order (MCU by MCU, Y00 Y01 Y10 Y11 Cb Cr or Y Cb Cr, zigzag inside a block)."""
    u = to_uint8_values(x).astype(dtype)
    _, H, W = u.shape
    my, mx = geometry(H, W, subsampling)
    ms = mcu_size(subsampling)
    c = lambda v: dtype(v)                                        # noqa: E731
    r, g, b = u
    y = c(0.299) * r + c(0.587) * g + c(0.114) * b
    cb = c(-0.299 / 1.772) * r - c(0.587 / 1.772) * g + c(0.5) * b + c(128)
    cr = c(0.5) * r - c(0.587 / 1.402) * g - c(0.114 / 1.402) * b + c(128)
    planes = [np.pad(p, ((0, my * ms - H), (0, mx * ms - W)), mode="edge") for p in (y, cb, cr)]
    if subsampling == 420:
        for i in (1, 2):
            p = planes[i]
            planes[i] = ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])) * c(0.25)
    d = dct_matrix().astype(dtype)
    tables = quant_tables(quality)

    def blocks(p, table):
        h, w = p.shape
        t = (p - c(128)).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)          # [by, bx, 8, 8]
        t = np.matmul(d, np.matmul(t, d.T))                                          # rows first, then columns
        quot = t / table.reshape(8, 8).astype(dtype)
        return quot.reshape(h // 8, w // 8, 64)[:, :, ZIGZAG]

    yq, cbq, crq = blocks(planes[0], tables[0]), blocks(planes[1], tables[1]), blocks(planes[2], tables[1])
    if subsampling == 420:
        yq = yq.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
    else:
        yq = yq.reshape(my, mx, 1, 64)
    quot = np.concatenate([yq, cbq.reshape(my, mx, 1, 64), crq.reshape(my, mx, 1, 64)], axis=2).reshape(-1, 64)
    q = np.sign(quot) * np.floor(np.abs(quot) + c(0.5))                              # ties away from zero
    lo = np.full(64, -1023.0)
    lo[0] = -1024.0
    q = np.clip(q, lo, 1023.0).astype(np.int64)
    return q, quot


def tie_distance(quot):
    """Distance of every quotient to the nearest rounding tie (k + 0.5)."""
    a = np.abs(np.asarray(quot, dtype=np.float64))
    return np.abs(a - np.floor(a) - 0.5)


def header(H, W, quality, subsampling, restart_mcus):
    """SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS (T.81 annex B, JFIF 1.02)."""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload

    out = b"\xff\xd8"
    out += seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, table in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(int(v) for v in table[ZIGZAG]))
    sampling = 0x22 if subsampling == 420 else 0x11
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, sampling, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += seg(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, restart_mcus.to_bytes(2, "big"))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        if self.n >= 512:
            rest = self.n & 7
            self.out += (self.acc >> rest).to_bytes((self.n - rest) // 8, "big")
            self.acc &= (1 << rest) - 1
            self.n = rest

    def finish(self):
        fill = -self.n % 8
        self.put((1 << fill) - 1, fill)                            # the last byte is filled with 1-bits
        if self.n:
            self.out += self.acc.to_bytes(self.n // 8, "big")
        return bytes(self.out)


def _size_and_bits(v):
    if v == 0:
        return 0, 0
    size = abs(v).bit_length()
    return size, (v if v > 0 else v - 1) & ((1 << size) - 1)


def entropy(q, subsampling, restart_mcus, stats=None):
    """Step 6 over q [blocks, 64] (scan order): the scan with its restart markers and EOI.  ``stats`` (a dict) collects what the
    stream exercises: stuffed bytes, ZRL symbols, blocks without EOB, DC and AC categories."""
    bpm = blocks_per_mcu(subsampling)
    q = np.asarray(q)
    mcus = q.shape[0] // bpm
    assert q.shape == (mcus * bpm, 64)
    st = stats if stats is not None else {}
    st.update(stuffed=0, zrl=0, no_eob=0, dc_categories=set(), ac_categories=set())
    comp_of = [0, 0, 0, 0, 1, 2] if bpm == 6 else [0, 1, 2]
    out = bytearray()
    intervals = -(-mcus // restart_mcus)
    rows = q.tolist()
    for it in range(intervals):
        bits = _Bits()
        pred = [0, 0, 0]
        for blk in range(it * restart_mcus * bpm, min((it + 1) * restart_mcus, mcus) * bpm):
            comp = comp_of[blk % bpm]
            tab = 0 if comp == 0 else 1
            row = rows[blk]
            size, extra = _size_and_bits(row[0] - pred[comp])
            pred[comp] = row[0]
            st["dc_categories"].add(size)
            code, length = DC_CODES[tab][size]
            bits.put((code << size) | extra, length + size)
            run = 0
            for k in range(1, 64):
                v = row[k]
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    bits.put(*AC_CODES[tab][0xF0])
                    st["zrl"] += 1
                    run -= 16
                size, extra = _size_and_bits(v)
                st["ac_categories"].add(size)
                code, length = AC_CODES[tab][(run << 4) | size]
                bits.put((code << size) | extra, length + size)
                run = 0
            if run:
                bits.put(*AC_CODES[tab][0x00])
            else:
                st["no_eob"] += 1
        data = bits.finish()
        st["stuffed"] += data.count(b"\xff")
        out += data.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD9 if it == intervals - 1 else 0xD0 + it % 8])
    return bytes(out)


def stream_from_coefficients(q, H, W, quality, subsampling, restart_mcus, stats=None):
    return header(H, W, quality, subsampling, restart_mcus) + entropy(q, subsampling, restart_mcus, stats)


def encode(x, quality, subsampling, restart_mcus, dtype=np.float64, stats=None):
    q, _ = coefficients(x, quality, subsampling, dtype)
    return stream_from_coefficients(q, x.shape[1], x.shape[2], quality, subsampling, restart_mcus, stats)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def synth(seed, h, w):
    """Seeded noise over smooth content, [3,h,w] fp32 (conftest.synth_image)."""
    from conftest import synth_image
    return synth_image(seed, 3, h, w).numpy().astype(np.float32)


def crafted(name, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "constant":
        p = np.full((h, w), 0.5)
    elif name == "noise":                                         # with quality 100: long codes, stuffed 0xFF bytes
        return np.random.default_rng(5).random((3, h, w), dtype=np.float32)
    elif name == "blocks":                                        # 8 x 8 black / white: DC differences of +-2040
        p = ((yy // 8 + xx // 8) % 2).astype(np.float64)
    elif name == "pixels":                                        # one-pixel checker: the highest frequencies
        p = ((yy + xx) % 2).astype(np.float64)
    elif name == "clamp":                                         # values outside [0, 1]
        return synth(11, h, w) * np.float32(1.6) - np.float32(0.3)
    else:
        raise KeyError(name)
    return np.broadcast_to(p.astype(np.float32), (3, h, w)).copy()


def whole_row(W, subsampling):
    return -(-W // mcu_size(subsampling))


# ---- PIL / libjpeg as the yardstick ----------------------------------------------------------------------------------------------
def pil_subsampling(subsampling):
    return {444: 0, 420: 2}[subsampling]


def pil_encode(u8_hwc, quality, subsampling, restart_mcus):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(u8_hwc).save(bio, "JPEG", quality=quality, subsampling=pil_subsampling(subsampling),
                                 restart_marker_blocks=restart_mcus)
    return bio.getvalue()


def pil_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def psnr_u8(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 10.0 * np.log10(255.0 ** 2 / max(mse, 1e-9))


def u8_image(x):
    return to_uint8_values(x).astype(np.uint8).transpose(1, 2, 0).copy()


def yardstick(x, quality, subsampling, restart_mcus):
    """PSNR to the uint8 input and stream size of libjpeg (through PIL) and of this restatement, both decoded by PIL."""
    u8 = u8_image(x)
    lib = pil_encode(u8, quality, subsampling, restart_mcus)
    ref = encode(x, quality, subsampling, restart_mcus)
    return {"u8": u8, "psnr_lib": psnr_u8(np.asarray(pil_decode(lib)), u8), "size_lib": len(lib),
            "psnr_ref": psnr_u8(np.asarray(pil_decode(ref)), u8), "size_ref": len(ref), "ref": ref}


# ---- the device's coefficients against the float64 statement ------------------------------------------------------------------
BAND_MARGIN = 4.0                    # for the kernel's summation order, which differs from the fp32 restatement's
# fp32 reasoning for a ceiling of the band: |c| < 2^11, so one rounding is at most 2^-13; the colour conversion, the chroma mean,
# the level shift, two 8-term sums and the division are fewer than 24 roundings on a path: 24 * 2^-13 * BAND_MARGIN
BAND_CEILING = 24 * 2.0 ** -13 * BAND_MARGIN


def coefficient_agreement(coef_dev, x, quality, subsampling):
    """Compare coefficients [blocks, 64] with the float64 statement on frame x.  The tie band is the fp32 restatement's largest
    deviation of c / Q from float64 on this input times BAND_MARGIN.  Returns the figures; ``bad`` counts coefficients that differ
    outside the band or by more than 1."""
    q64, quot64 = coefficients(x, quality, subsampling, np.float64)
    _, quot32 = coefficients(x, quality, subsampling, np.float32)
    dev32 = float(np.abs(quot32.astype(np.float64) - quot64).max())
    band = BAND_MARGIN * dev32
    coef_dev = np.asarray(coef_dev, dtype=np.int64)
    assert coef_dev.shape == q64.shape, (coef_dev.shape, q64.shape)
    differ = coef_dev != q64
    in_band = tie_distance(quot64) <= band
    bad = differ & (~in_band | (np.abs(coef_dev - q64) != 1))
    return {"band": band, "fp32_deviation": dev32, "margin": BAND_MARGIN, "coefficients": int(q64.size),
            "in_band": int(in_band.sum()), "mismatches": int(differ.sum()), "bad": int(bad.sum())}
