// Host-only part of the baseline JPEG encoder (jpeg.hip): the ITU T.81 Annex K tables, the IJG quality scaling, the JFIF header
// writer and the arithmetic of the stream bound and of the workspace.  No HIP type or call: tests/cpp/jpeg_host_check.cpp compiles
// this header on its own with the host sanitizers.
#pragma once
#include <cstdint>

namespace nunif {
namespace jpeg {

constexpr int kMaxDim = 8192;            // H and W
constexpr int kMaxBatch = 16;
constexpr int kMaxRestart = 65535;       // DRI holds 16 bits
constexpr int kHeaderBytes = 629;        // SOI 2, APP0 18, 2 x DQT 69, SOF0 19, DHT 2 x (33 + 183), DRI 6, SOS 14

// Worst case of one block in bits.  DC: the longest code (11 bits, chroma category 11) and 11 value bits.  AC: every symbol
// covers at least one coefficient and costs at most a 16-bit code and 10 value bits (AC is clamped to +-1023); ZRL covers 16
// coefficients with at most 16 bits and EOB at least one with at most 4: 26 bits per coefficient bounds them all.
constexpr int kMaxBlockBits = 22 + 63 * 26;

// zigzag position -> natural (row-major) index, T.81 figure A.6
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 tables K.1 and K.2, natural order
constexpr uint8_t kLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                  99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// T.81 tables K.3 - K.6: BITS (codes per length 1..16) and HUFFVAL
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

constexpr int bits_total(const uint8_t *bits) {
    int n = 0;
    for (int i = 0; i < 16; ++i) n += bits[i];
    return n;
}
static_assert(bits_total(kDcLumaBits) == 12 && bits_total(kDcChromaBits) == 12, "DC tables: 12 categories");
static_assert(bits_total(kAcLumaBits) == 162 && bits_total(kAcChromaBits) == 162, "AC tables: 162 symbols");

// The code of every symbol of one table (T.81 annex C): length << 16 | code, 0 for a symbol the table does not hold.
struct HuffTable {
    uint32_t e[256];
};
constexpr HuffTable huff_table(const uint8_t *bits, const uint8_t *vals) {
    HuffTable t{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) t.e[vals[k++]] = ((unsigned)len << 16) | code++;
        code <<= 1;
    }
    return t;
}

inline bool valid_subsampling(int ss) { return ss == 420 || ss == 444; }
inline int mcu_size(int ss) { return ss == 420 ? 16 : 8; }            // pixels per MCU side
inline int blocks_per_mcu(int ss) { return ss == 420 ? 6 : 3; }

inline bool valid_frame(int64_t B, int64_t H, int64_t W, int ss, int64_t restart_mcus) {
    return B >= 1 && B <= kMaxBatch && H >= 1 && H <= kMaxDim && W >= 1 && W <= kMaxDim && valid_subsampling(ss) &&
           restart_mcus >= 1 && restart_mcus <= kMaxRestart;
}

// The IJG scaling of the Annex K tables, baseline-clamped (jpeg_set_quality(q, TRUE)); natural order.
inline bool quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
    if (quality < 1 || quality > 100) return false;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        int l = (kLumaQ[i] * scale + 50) / 100, c = (kChromaQ[i] * scale + 50) / 100;
        luma[i] = (uint8_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma[i] = (uint8_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
    return true;
}

struct Geometry {
    int mcus_x, mcus_y, bpm;
    int64_t mcus, blocks, intervals;
};
inline Geometry geometry(int H, int W, int ss, int restart_mcus) {
    const int m = mcu_size(ss);
    Geometry g;
    g.mcus_x = (W + m - 1) / m;
    g.mcus_y = (H + m - 1) / m;
    g.bpm = blocks_per_mcu(ss);
    g.mcus = (int64_t)g.mcus_x * g.mcus_y;
    g.blocks = g.mcus * g.bpm;
    g.intervals = (g.mcus + restart_mcus - 1) / restart_mcus;
    return g;
}

// Upper bound of one restart interval of `mcus` MCUs in bytes, its RSTn or EOI marker included: every bit of every block, the
// last byte filled up, every byte a stuffed 0xFF.
inline int64_t interval_bound(int64_t mcus, int bpm) { return 2 * ((mcus * bpm * kMaxBlockBits + 7) / 8) + 2; }

// Upper bound of the whole stream; -1 for a frame the encoder refuses.
inline int64_t max_bytes(int H, int W, int ss, int restart_mcus) {
    if (!valid_frame(1, H, W, ss, restart_mcus)) return -1;
    const Geometry g = geometry(H, W, ss, restart_mcus);
    const int64_t full = g.mcus / restart_mcus, tail = g.mcus % restart_mcus;
    return kHeaderBytes + full * interval_bound(restart_mcus, g.bpm) + (tail ? interval_bound(tail, g.bpm) : 0);
}

// The workspace: the quantised coefficients [B][blocks][64] i16, per interval its byte count and its offset in the scan (i32
// each), and a staging slot of interval_bound(restart_mcus) bytes per interval.  Every part starts on a multiple of 256 bytes.
struct Workspace {
    int64_t coef, count, offset, stage, slot, total;
};
inline int64_t align256(int64_t n) { return (n + 255) & ~(int64_t)255; }
inline Workspace workspace(int B, int H, int W, int ss, int restart_mcus) {
    const Geometry g = geometry(H, W, ss, restart_mcus);
    Workspace w;
    w.coef = 0;
    w.count = align256(w.coef + (int64_t)B * g.blocks * 128);
    w.offset = align256(w.count + (int64_t)B * g.intervals * 4);
    w.stage = align256(w.offset + (int64_t)B * g.intervals * 4);
    w.slot = interval_bound(g.mcus < restart_mcus ? g.mcus : restart_mcus, g.bpm);
    w.total = align256(w.stage + (int64_t)B * g.intervals * w.slot);
    return w;
}
inline int64_t workspace_bytes(int B, int H, int W, int ss, int restart_mcus) {
    if (!valid_frame(B, H, W, ss, restart_mcus)) return -1;
    return workspace(B, H, W, ss, restart_mcus).total;
}

struct ByteSink {
    uint8_t *p;
    int n;
    void u8(int v) { p[n++] = (uint8_t)v; }
    void u16(int v) { u8(v >> 8); u8(v & 255); }
    void bytes(const uint8_t *s, int k) { for (int i = 0; i < k; ++i) u8(s[i]); }
};

// SOI, APP0 (JFIF 1.01, no units, 1:1), DQT x 2 (8 bit, zigzag), SOF0, DHT x 4 (Annex K), DRI, SOS into out[kHeaderBytes];
// returns the length, or -1 for arguments the encoder refuses.
inline int header(int H, int W, int quality, int ss, int restart_mcus, uint8_t *out) {
    uint8_t q[2][64];
    if (!valid_frame(1, H, W, ss, restart_mcus) || !quant_tables(quality, q[0], q[1])) return -1;
    ByteSink s{out, 0};
    s.u16(0xFFD8);
    s.u16(0xFFE0); s.u16(16);
    const uint8_t jfif[5] = {'J', 'F', 'I', 'F', 0};
    s.bytes(jfif, 5);
    s.u16(0x0101); s.u8(0); s.u16(1); s.u16(1); s.u8(0); s.u8(0);
    for (int t = 0; t < 2; ++t) {
        s.u16(0xFFDB); s.u16(67); s.u8(t);
        for (int i = 0; i < 64; ++i) s.u8(q[t][kZigzag[i]]);
    }
    s.u16(0xFFC0); s.u16(17); s.u8(8); s.u16(H); s.u16(W); s.u8(3);
    s.u8(1); s.u8(ss == 420 ? 0x22 : 0x11); s.u8(0);
    s.u8(2); s.u8(0x11); s.u8(1);
    s.u8(3); s.u8(0x11); s.u8(1);
    const struct { int id; const uint8_t *bits, *vals; int n; } dht[4] = {
        {0x00, kDcLumaBits, kDcVals, 12}, {0x10, kAcLumaBits, kAcLumaVals, 162},
        {0x01, kDcChromaBits, kDcVals, 12}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
    for (const auto &d : dht) {
        s.u16(0xFFC4); s.u16(2 + 1 + 16 + d.n); s.u8(d.id);
        s.bytes(d.bits, 16);
        s.bytes(d.vals, d.n);
    }
    s.u16(0xFFDD); s.u16(4); s.u16(restart_mcus);
    s.u16(0xFFDA); s.u16(12); s.u8(3);
    s.u8(1); s.u8(0x00); s.u8(2); s.u8(0x11); s.u8(3); s.u8(0x11);
    s.u8(0); s.u8(63); s.u8(0);
    return s.n;
}

}  // namespace jpeg
}  // namespace nunif
