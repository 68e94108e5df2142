"""A restatement of the PNG frame encoder of nunif_amd/csrc/png.hip in plain Python / numpy, written from the PNG specification
(filter types, chunk layout), RFC 1950 (zlib wrapper, Adler-32) and RFC 1951 (dynamic Huffman blocks), and from the layout that
DESIGN.md ("PNG frame encoder") fixes: stripes, the row filter heuristic, greedy matches at the pixel distance, the tie orders of
the three codes.  It shares no code with the kernel: the tokens come from a sequential greedy loop, the code lengths from an
explicit two-queue Huffman tree.  The device's stream has to equal this one byte for byte.
"""
import struct
import zlib
from collections import deque

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
RGB8_F32, RGB8_U8, GRAY16_F32 = 0, 1, 2
BPP = {RGB8_F32: 3, RGB8_U8: 3, GRAY16_F32: 2}
MAX_DIM, MAX_BATCH = 8192, 16
MAX_MATCH, MIN_MATCH = 258, 3

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
N_LIT, N_DIST, N_CL = 286, 30, 19


# ---- pixels -------------------------------------------------------------------------------------------------------------------------
def quantise(frame, form):
    """One frame -> its raw PNG rows, uint8 [H, W * bpp].  RGB from f32 [3,H,W]: clamp, x 255, round half even; RGB from u8
    [H,W,3]: as it is; grey 16 from f32 [1,H,W]: clamp, fp32 0xffff * d, truncation, big-endian."""
    x = np.asarray(frame)
    if form == RGB8_F32:
        q = np.rint(np.clip(x.astype(np.float32), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
        return np.ascontiguousarray(q.transpose(1, 2, 0)).reshape(q.shape[1], -1)
    if form == RGB8_U8:
        assert x.dtype == np.uint8
        return np.ascontiguousarray(x).reshape(x.shape[0], -1)
    d = (np.float32(0xffff) * np.clip(x.astype(np.float32), np.float32(0), np.float32(1))).astype(np.uint16)[0]
    return np.ascontiguousarray(d.astype(">u2")).view(np.uint8).reshape(d.shape[0], -1)


def pixels(frame, form):
    """What a decoder has to give back: uint8 [H,W,3] or uint16 [H,W]."""
    raw = quantise(frame, form)
    if form == GRAY16_F32:
        return raw.view(">u2").astype(np.uint16)
    return raw.reshape(raw.shape[0], -1, 3)


# ---- row filter ---------------------------------------------------------------------------------------------------------------------
def filter_rows(raw, bpp):
    """PNG filter types 0..4 over the whole image; per row the type with the smallest sum of |filtered byte as signed|, the
    lowest type on a tie.  Returns uint8 [H, 1 + W * bpp], the type in column 0."""
    H, R = raw.shape
    x = raw.astype(np.int32)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if R > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, bpp:] = b[:, :-bpp] if R > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)             # [5, H]
    ftype = np.argmin(cost, axis=0)                                       # the first minimum
    out = np.empty((H, 1 + R), np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = cand[ftype, np.arange(H)]
    return out


# ---- tokens -------------------------------------------------------------------------------------------------------------------------
def tokens(d, bpp):
    """Greedy, left to right over the stripe's bytes: a match at distance bpp of the longest length 3..258, else a literal.
    A match never reaches back past the start of the stripe.  Returns a list of (literal,) and (length, distance)."""
    d = np.asarray(d, np.uint8)
    n = len(d)
    eq = np.zeros(n + 1, bool)
    eq[bpp:n] = d[bpp:] == d[:-bpp]
    # ahead[i]: how many positions from i on repeat the byte bpp before them
    idx = np.arange(n + 1)
    stop = np.where(~eq, idx, n + 1)
    nxt = np.minimum.accumulate(stop[::-1])[::-1]
    ahead = (nxt - idx)[:n]
    out, i = [], 0
    dl = d.tolist()
    al = ahead.tolist()
    while i < n:
        length = min(al[i], MAX_MATCH)
        if length >= MIN_MATCH:
            out.append((length, bpp))
            i += length
        else:
            out.append((dl[i],))
            i += 1
    return out


def length_symbol(length):
    for k in range(28, -1, -1):
        if length >= LEN_BASE[k]:
            return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def distance_symbol(dist):
    assert 1 <= dist <= 4                                                 # codes 0..3 carry no extra bits
    return dist - 1


def histograms(toks):
    lit, dist = [0] * N_LIT, [0] * N_DIST
    for t in toks:
        if len(t) == 1:
            lit[t[0]] += 1
        else:
            lit[length_symbol(t[0])[0]] += 1
            dist[distance_symbol(t[1])] += 1
    lit[256] += 1
    return lit, dist


# ---- codes --------------------------------------------------------------------------------------------------------------------------
def unlimited_depths(hist):
    """Huffman's algorithm with two queues.  The leaves are ordered by (count, symbol) ascending; the internal nodes by creation;
    of a leaf and an internal node of equal weight the leaf goes first.  Returns {symbol: depth}."""
    leaves = deque(sorted((c, s) for s, c in enumerate(hist) if c))
    depth = {s: 0 for _, s in leaves}
    if len(leaves) == 1:
        return {leaves[0][1]: 1}
    inner = deque()

    def take():
        if inner and (not leaves or inner[0][0] < leaves[0][0]):
            return inner.popleft()
        c, s = leaves.popleft()
        return c, [s]

    while len(leaves) + len(inner) > 1:
        (w1, m1), (w2, m2) = take(), take()
        for s in m1 + m2:
            depth[s] += 1
        inner.append((w1 + w2, m1 + m2))
    return depth


def code_lengths(hist, limit):
    """Code lengths of a prefix code limited to `limit` bits.  The depths of the unlimited tree are counted per length; lengths
    above the limit are folded into it; while the Kraft sum is too large, one code of the limit is dropped and the deepest
    shorter length that has a code gives one up for two of the next length.  The symbols, ordered by (count, symbol) ascending,
    then take the lengths from the longest to the shortest."""
    lens = [0] * len(hist)
    depth = unlimited_depths(hist)
    if not depth:
        return lens
    count = [0] * (limit + 1)
    for dep in depth.values():
        count[min(dep, limit)] += 1
    total = sum(count[i] << (limit - i) for i in range(1, limit + 1))
    while total > (1 << limit):
        count[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if count[i]:
                count[i] -= 1
                count[i + 1] += 2
                break
        total -= 1
    order = sorted((c, s) for s, c in enumerate(hist) if c)
    k = 0
    for i in range(limit, 0, -1):
        for _ in range(count[i]):
            lens[order[k][1]] = i
            k += 1
    assert k == len(order)
    return lens


def canonical_codes(lens):
    """RFC 1951 section 3.2.2."""
    top = max(lens) if lens else 0
    bl = [0] * (top + 2)
    for n in lens:
        if n:
            bl[n] += 1
    nxt, code = [0] * (top + 2), 0
    for bits in range(1, top + 1):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lens)
    for s, n in enumerate(lens):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


def run_length_lengths(seq):
    """The code lengths as symbols of the code-length alphabet: runs of zeros as 18 (11..138) and 17 (3..10), the longest first;
    everything else, shorter runs of zeros included, as it is.  Symbol 16 is not used.  Returns (symbol, extra bits, value)."""
    out, i = [], 0
    while i < len(seq):
        if seq[i] == 0:
            z = 1
            while i + z < len(seq) and seq[i + z] == 0 and z < 138:
                z += 1
            if z >= 11:
                out.append((18, 7, z - 11))
            elif z >= 3:
                out.append((17, 3, z - 3))
            else:
                z = 1
                out.append((0, 0, 0))
            i += z
        else:
            out.append((seq[i], 0, 0))
            i += 1
    return out


class StripeCodes():
    def __init__(self, toks):
        self.lit_hist, self.dist_hist = histograms(toks)
        self.lit_len = code_lengths(self.lit_hist, 15)
        self.dist_len = code_lengths(self.dist_hist, 15)
        self.hlit = max(257, max(s for s in range(N_LIT) if self.lit_len[s]) + 1)
        self.hdist = max([1] + [s + 1 for s in range(N_DIST) if self.dist_len[s]])
        self.cl_syms = run_length_lengths(self.lit_len[:self.hlit] + self.dist_len[:self.hdist])
        self.cl_hist = [0] * N_CL
        for s, _, _ in self.cl_syms:
            self.cl_hist[s] += 1
        self.cl_len = code_lengths(self.cl_hist, 7)
        self.hclen = max(4, max(k + 1 for k in range(N_CL) if self.cl_len[CL_ORDER[k]]))

    def hist(self):
        return self.lit_hist + self.dist_hist + self.cl_hist

    def lengths(self):
        return self.lit_len + self.dist_len + self.cl_len


class BitSink():
    """RFC 1951 section 3.1.1: data elements from the least significant bit of a byte on, Huffman codes from their most significant bit on."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, count):
        self.bits(int(format(code, "0%db" % count)[::-1], 2) if count else 0, count)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def deflate_stripe(d, bpp, last):
    """One dynamic-Huffman block (BFINAL 0) and an empty stored block, which carries BFINAL in the last stripe."""
    toks = tokens(d, bpp)
    sc = StripeCodes(toks)
    lit_code, dist_code, cl_code = (canonical_codes(x) for x in (sc.lit_len, sc.dist_len, sc.cl_len))
    s = BitSink()
    s.bits(0, 1)
    s.bits(2, 2)
    s.bits(sc.hlit - 257, 5)
    s.bits(sc.hdist - 1, 5)
    s.bits(sc.hclen - 4, 4)
    for k in range(sc.hclen):
        s.bits(sc.cl_len[CL_ORDER[k]], 3)
    for sym, nb, val in sc.cl_syms:
        s.code(cl_code[sym], sc.cl_len[sym])
        s.bits(val, nb)
    for t in toks:
        if len(t) == 1:
            s.code(lit_code[t[0]], sc.lit_len[t[0]])
        else:
            sym, nb, val = length_symbol(t[0])
            s.code(lit_code[sym], sc.lit_len[sym])
            s.bits(val, nb)
            ds = distance_symbol(t[1])
            s.code(dist_code[ds], sc.dist_len[ds])
    s.code(lit_code[256], sc.lit_len[256])
    s.bits(1 if last else 0, 1)
    s.bits(0, 2)
    s.align()
    s.out += b"\x00\x00\xff\xff"
    return bytes(s.out)


# ---- checksums ----------------------------------------------------------------------------------------------------------------------
def crc_table():
    t = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0xEDB88320 if c & 1 else c >> 1
        t.append(c)
    return t


_CRC = crc_table()


def crc32(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32(data):
    a, b = 1, 0
    for v in bytes(data):
        a = (a + v) % 65521
        b = (b + a) % 65521
    return (b << 16) | a


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc32(kind + data))


# ---- the file -----------------------------------------------------------------------------------------------------------------------
def header(H, W, form, text=None):
    """Signature, IHDR and one tEXt chunk per entry of `text` (Latin-1 keyword, a zero byte, Latin-1 text)."""
    ihdr = struct.pack(">IIBBBBB", W, H, 16 if form == GRAY16_F32 else 8, 0 if form == GRAY16_F32 else 2, 0, 0, 0)
    out = SIGNATURE + chunk(b"IHDR", ihdr)
    for k, v in (text or {}).items():
        out += chunk(b"tEXt", str(k).encode("latin-1") + b"\0" + str(v).encode("latin-1"))
    return out


def stripes(filtered, stripe_rows):
    H = filtered.shape[0]
    return [filtered[r:r + stripe_rows].reshape(-1) for r in range(0, H, stripe_rows)]


def body(frame, form, stripe_rows):
    """The IDAT chunks, one per stripe, and IEND."""
    bpp = BPP[form]
    filtered = filter_rows(quantise(frame, form), bpp)
    parts = stripes(filtered, stripe_rows)
    out = b""
    for k, d in enumerate(parts):
        last = k == len(parts) - 1
        data = (b"\x78\x01" if k == 0 else b"") + deflate_stripe(d, bpp, last)
        if last:
            data += struct.pack(">I", adler32(filtered.tobytes()))
        out += chunk(b"IDAT", data)
    return out + chunk(b"IEND", b"")


def encode(frame, form, stripe_rows, text=None):
    raw = quantise(frame, form)
    return header(raw.shape[0], raw.shape[1] // BPP[form], form, text) + body(frame, form, stripe_rows)


def stripe_codes(frame, form, stripe_rows):
    bpp = BPP[form]
    filtered = filter_rows(quantise(frame, form), bpp)
    return [StripeCodes(tokens(d, bpp)) for d in stripes(filtered, stripe_rows)]


def max_bytes(H, W, form, stripe_rows):
    """The bound of DESIGN.md, restated: per stripe of n filtered bytes 3 + 14 + 19 x 3 + 316 x 7 header bits, 15 bits per byte,
    15 for the end of block, 3 for the stored block's header, rounded up to a byte, its 4 length bytes and 12 bytes of chunk;
    2 bytes of zlib header, 4 of Adler-32, 12 of IEND."""
    if form not in BPP or not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM and 1 <= stripe_rows <= H):
        return -1
    row = 1 + W * BPP[form]
    total = 2 + 4 + 12
    for r in range(0, H, stripe_rows):
        n = min(stripe_rows, H - r) * row
        total += (3 + 14 + 57 + 316 * 7 + 15 * n + 15 + 3 + 7) // 8 + 4 + 12
    return total


def split_chunks(stream):
    """[(type, data, crc)] of a chunk sequence."""
    out, o = [], 0
    while o < len(stream):
        n, = struct.unpack(">I", stream[o:o + 4])
        out.append((stream[o + 4:o + 8], stream[o + 8:o + 8 + n], struct.unpack(">I", stream[o + 8 + n:o + 12 + n])[0]))
        o += 12 + n
    return out


# ---- crafted inputs ------------------------------------------------------------------------------------------------------------------
def fibonacci_frame():
    """uint8 [8,W,3]: one stripe of 8 rows whose byte counts grow like Fibonacci numbers over 24 values close to 0 (as signed bytes), so that
    whichever filter a row takes the unlimited Huffman tree of the stripe is deeper than 15.  Encode with stripe_rows = 8."""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    values = [0] + [v for k in range(1, 13) for v in (k, 256 - k)][:23]
    data = np.concatenate([np.full(c, v, np.uint8) for c, v in zip(fib, values)])
    data = np.concatenate([data, np.zeros((-len(data)) % 3, np.uint8)])
    np.random.default_rng(7).shuffle(data)
    return data.reshape(8, -1, 3)


def run_frames():
    """[(frame f32 [1,H,W] for the 16-bit grey form, stripe_rows, run)]: all-zero stripes, so two literals and then a run of
    258 + 1, 258 + 2 and 258 + 3 repeating bytes."""
    return [(np.zeros((1, 1, 130), np.float32), 1, 259), (np.zeros((1, 2, 65), np.float32), 2, 260),
            (np.zeros((1, 1, 131), np.float32), 1, 261)]
