// Host-only part of the PNG frame encoder (png.hip): the forms and limits, the deflate constants, the CRC-32 table and the powers
// of x that combine piecewise CRCs, the writer of signature + IHDR + tEXt, and the arithmetic of the stream bound and of the
// workspace.  No HIP type or call: tests/cpp/png_host_check.cpp compiles this header on its own with the host sanitizers.
#pragma once
#include <cstdint>
#include <cstring>

namespace nunif {
namespace png {

constexpr int kMaxDim = 8192;            // H and W
constexpr int kMaxBatch = 16;
// 3 is refused (it never named a form); 4..6 take planar fp32 colour and, where the form has one, a separate fp32 alpha plane
enum Form { kRgb8F32 = 0, kRgb8U8 = 1, kGray16F32 = 2, kRgba8F32 = 4, kGray8F32 = 5, kGrayA8F32 = 6 };

constexpr int kNumLit = 286, kNumDist = 30, kNumCl = 19;
constexpr int kSymbols = kNumLit + kNumDist + kNumCl;        // 335: one stripe's histogram or code lengths, in this order
constexpr int kSymbolStride = 336;
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr int kHeaderWords = 160;        // the block header of one stripe, bit-packed: at most 74 + 316 x 14 = 4 498 bits
constexpr int kCodeWords = 288;          // 286 literal / length codes, then the distance code

// RFC 1951 section 3.2.5: length symbols 257..285
constexpr uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
// RFC 1951 section 3.2.7: the order in which the code lengths of the code-length alphabet are sent
constexpr uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

inline bool valid_form(int form) {
    return form == kRgb8F32 || form == kRgb8U8 || form == kGray16F32 || form == kRgba8F32 || form == kGray8F32 || form == kGrayA8F32;
}
inline bool planes_form(int form) { return form == kRgba8F32 || form == kGray8F32 || form == kGrayA8F32; }
inline bool has_alpha(int form) { return form == kRgba8F32 || form == kGrayA8F32; }
inline int bytes_per_pixel(int form) {
    return form == kRgba8F32 ? 4 : form == kGray8F32 ? 1 : (form == kGray16F32 || form == kGrayA8F32) ? 2 : 3;
}
// IHDR: bit depth and colour type (0 grey, 2 RGB, 4 grey + alpha, 6 RGB + alpha)
inline int bit_depth(int form) { return form == kGray16F32 ? 16 : 8; }
inline int colour_type(int form) {
    return form == kRgba8F32 ? 6 : form == kGrayA8F32 ? 4 : (form == kGray16F32 || form == kGray8F32) ? 0 : 2;
}
inline bool valid_frame(int64_t B, int64_t H, int64_t W, int form, int64_t stripe_rows) {
    return B >= 1 && B <= kMaxBatch && H >= 1 && H <= kMaxDim && W >= 1 && W <= kMaxDim && valid_form(form) &&
           stripe_rows >= 1 && stripe_rows <= H;
}

// ---- CRC-32 (PNG annex D; reflected polynomial 0xEDB88320) ---------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
struct CrcTable {
    uint32_t e[256];
};
constexpr CrcTable crc_table() {
    CrcTable t{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        t.e[n] = c;
    }
    return t;
}
// a x b mod P for reflected polynomials: bit 31 is x^0
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// Appending n zero bytes to a message multiplies its raw CRC (start 0, no final complement) by x^(8n); so for raw CRCs
// crc(A || B) = crc(A) x^(8 |B|) + crc(B).  kPow16[k] = x^(128 k), pieces of 16 bytes; kPow1[r] = x^(8 r), the last piece.
constexpr int kCrcPieces = 640;
struct CrcPowers {
    uint32_t pow16[kCrcPieces + 1];
    uint32_t pow1[16];
};
constexpr CrcPowers crc_powers() {
    CrcPowers t{};
    const uint32_t x8 = 0x00800000u;                          // x^8
    t.pow1[0] = 0x80000000u;
    for (int r = 1; r < 16; ++r) t.pow1[r] = crc_mul(t.pow1[r - 1], x8);
    const uint32_t x128 = crc_mul(t.pow1[15], x8);
    t.pow16[0] = 0x80000000u;
    for (int k = 1; k <= kCrcPieces; ++k) t.pow16[k] = crc_mul(t.pow16[k - 1], x128);
    return t;
}
inline uint32_t crc32(const uint8_t *p, int64_t n) {
    static const CrcTable t = crc_table();
    uint32_t c = 0xFFFFFFFFu;
    for (int64_t i = 0; i < n; ++i) c = t.e[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// ---- the bound ---------------------------------------------------------------------------------------------------------------------
struct Geometry {
    int bpp, stripes, stripe_rows;
    int64_t row;                         // filtered bytes of a row: the filter type and W x bpp
    int64_t stripe_bytes;                // of a full stripe
};
inline Geometry geometry(int H, int W, int form, int stripe_rows) {
    Geometry g;
    g.bpp = bytes_per_pixel(form);
    g.stripe_rows = stripe_rows;
    g.stripes = (H + stripe_rows - 1) / stripe_rows;
    g.row = 1 + (int64_t)W * g.bpp;
    g.stripe_bytes = g.row * stripe_rows;
    return g;
}

// Upper bound of the deflate data of a stripe of n filtered bytes.  Bits: BFINAL + BTYPE 3, HLIT + HDIST + HCLEN 14, the code
// lengths of the code-length code 19 x 3, at most 316 code lengths of at most 7 bits each (a run symbol with its extra bits costs
// at most 14 bits and stands for at least 3 of them), at most 15 bits per filtered byte (a literal is one byte and at most 15
// bits; a match is at least 3 bytes and at most 15 + 5 + 15 bits), the end of block 15, the stored block's header 3; the fill
// to a byte boundary; the 4 bytes LEN / NLEN.
inline int64_t stripe_data_bound(int64_t n) { return (3 + 14 + 57 + 316 * 7 + 15 * n + 15 + 3 + 7) / 8 + 4; }

// Upper bound of the body (the IDAT chunks and IEND); -1 for a frame the encoder refuses.
inline int64_t max_bytes(int H, int W, int form, int stripe_rows) {
    if (!valid_frame(1, H, W, form, stripe_rows)) return -1;
    const Geometry g = geometry(H, W, form, stripe_rows);
    const int64_t tail_rows = H - (int64_t)(g.stripes - 1) * stripe_rows;
    return (int64_t)(g.stripes - 1) * (12 + stripe_data_bound(g.stripe_bytes)) + 12 + stripe_data_bound(tail_rows * g.row) + 2 + 4 +
           12;
}

// ---- the workspace -----------------------------------------------------------------------------------------------------------------
// filtered: [B][stripes] slots of stripe_stride bytes (a stripe starts on a multiple of 16); rowsum: [B][H][2] u32, the Adler
// sums of a row; hist and lens: [B][stripes][336] i32; codes: [B][stripes][288] u32; header: [B][stripes][160] u32;
// meta: [B][stripes][4] i32 (header bits, data bytes, offset of the chunk in the body, spare); frame: [B][4] u32 (Adler-32).
struct Workspace {
    int64_t filtered, rowsum, hist, lens, codes, header, meta, frame, total;
    int64_t stripe_stride;
};
inline int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }
inline Workspace workspace(int B, int H, int W, int form, int stripe_rows) {
    const Geometry g = geometry(H, W, form, stripe_rows);
    const int64_t ns = (int64_t)B * g.stripes;
    Workspace w;
    w.stripe_stride = (g.stripe_bytes + 15) & ~(int64_t)15;
    w.filtered = 0;
    w.rowsum = align256(w.filtered + ns * w.stripe_stride);
    w.hist = align256(w.rowsum + (int64_t)B * H * 8);
    w.lens = align256(w.hist + ns * kSymbolStride * 4);
    w.codes = align256(w.lens + ns * kSymbolStride * 4);
    w.header = align256(w.codes + ns * kCodeWords * 4);
    w.meta = align256(w.header + ns * kHeaderWords * 4);
    w.frame = align256(w.meta + ns * 16);
    w.total = align256(w.frame + (int64_t)B * 16);
    return w;
}
inline int64_t workspace_bytes(int B, int H, int W, int form, int stripe_rows) {
    if (!valid_frame(B, H, W, form, stripe_rows)) return -1;
    return workspace(B, H, W, form, stripe_rows).total;
}

// ---- signature, IHDR, tEXt ---------------------------------------------------------------------------------------------------------
struct ByteSink {
    uint8_t *p;
    int64_t n, cap;
    bool ok;
    void u8(int v) {
        if (n < cap) p[n] = (uint8_t)v; else ok = false;
        ++n;
    }
    void u32(uint32_t v) { u8(v >> 24); u8((v >> 16) & 255); u8((v >> 8) & 255); u8(v & 255); }
    void bytes(const void *s, int64_t k) { for (int64_t i = 0; i < k; ++i) u8(static_cast<const uint8_t *>(s)[i]); }
    // the CRC of a chunk covers its type and its data: the bytes from `from` on
    void crc_since(int64_t from) { const uint32_t c = ok ? crc32(p + from, n - from) : 0u; u32(c); }
};

// The PNG signature, IHDR (bit depth and colour type of the form, deflate, adaptive filtering, no interlace) and one tEXt chunk per entry
// (keyword 1..79 bytes, a zero byte, the text) into out[capacity]; returns the length, -1 for arguments the encoder refuses,
// -2 where the capacity is too small.
inline int64_t header(int H, int W, int form, const char *const *keys, const char *const *values, int n_text, uint8_t *out,
                      int64_t capacity) {
    if (!valid_frame(1, H, W, form, 1) || n_text < 0 || (n_text > 0 && (!keys || !values)) || !out || capacity < 0) return -1;
    for (int i = 0; i < n_text; ++i) {
        if (!keys[i] || !values[i]) return -1;
        const size_t k = std::strlen(keys[i]);
        if (k < 1 || k > 79) return -1;
    }
    ByteSink s{out, 0, capacity, true};
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    s.bytes(sig, 8);
    s.u32(13);
    int64_t from = s.n;
    s.bytes("IHDR", 4);
    s.u32((uint32_t)W); s.u32((uint32_t)H);
    s.u8(bit_depth(form)); s.u8(colour_type(form)); s.u8(0); s.u8(0); s.u8(0);
    s.crc_since(from);
    for (int i = 0; i < n_text; ++i) {
        const int64_t k = (int64_t)std::strlen(keys[i]), v = (int64_t)std::strlen(values[i]);
        s.u32((uint32_t)(k + 1 + v));
        from = s.n;
        s.bytes("tEXt", 4);
        s.bytes(keys[i], k); s.u8(0); s.bytes(values[i], v);
        s.crc_since(from);
    }
    return s.ok ? s.n : -2;
}

}  // namespace png
}  // namespace nunif
