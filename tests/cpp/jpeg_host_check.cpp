// Stand-alone check of nunif_amd/csrc/jpeg_host.h, built with the host sanitizers by tests/test_jpeg_host.py: the quantisation
// tables for every quality, the header for both subsamplings, the Huffman code construction, and the arithmetic of the stream
// bound and of the workspace at the corners of the accepted range.  No HIP call; nothing here runs on a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nunif_amd/csrc/jpeg_host.h"

using namespace nunif::jpeg;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main() {
    // tables: 1..255, monotone in the quality, Annex K itself at quality 50, all ones at 100
    std::vector<uint8_t> prev_l(64, 255), prev_c(64, 255);
    for (int q = 1; q <= 100; ++q) {
        std::vector<uint8_t> l(64), c(64);
        CHECK(quant_tables(q, l.data(), c.data()));
        for (int i = 0; i < 64; ++i) {
            CHECK(l[i] >= 1 && c[i] >= 1 && l[i] <= prev_l[i] && c[i] <= prev_c[i]);
            if (q == 50) CHECK(l[i] == kLumaQ[i] && c[i] == kChromaQ[i]);
            if (q == 100) CHECK(l[i] == 1 && c[i] == 1);
        }
        prev_l = l;
        prev_c = c;
    }
    {
        std::vector<uint8_t> l(64), c(64);
        CHECK(!quant_tables(0, l.data(), c.data()) && !quant_tables(101, l.data(), c.data()));
    }
    // zigzag is a permutation
    {
        int seen[64] = {0};
        for (int i = 0; i < 64; ++i) seen[kZigzag[i]]++;
        for (int i = 0; i < 64; ++i) CHECK(seen[i] == 1);
    }
    // Huffman codes: prefix-free by construction; lengths 2..16, every AC symbol of the table present, the all-ones code unused
    {
        const HuffTable t[4] = {huff_table(kDcLumaBits, kDcVals), huff_table(kDcChromaBits, kDcVals),
                                huff_table(kAcLumaBits, kAcLumaVals), huff_table(kAcChromaBits, kAcChromaVals)};
        for (int k = 0; k < 4; ++k) {
            int n = 0;
            for (int s = 0; s < 256; ++s) {
                if (!t[k].e[s]) continue;
                ++n;
                const unsigned len = t[k].e[s] >> 16, code = t[k].e[s] & 0xffffu;
                CHECK(len >= 2 && len <= 16 && code < (1u << len) - 1u);
                for (int o = 0; o < 256; ++o) {
                    if (o == s || !t[k].e[o]) continue;
                    const unsigned lo = t[k].e[o] >> 16, co = t[k].e[o] & 0xffffu;
                    if (lo >= len) CHECK((co >> (lo - len)) != code);
                }
            }
            CHECK(n == (k < 2 ? 12 : 162));
        }
        CHECK((t[0].e[11] >> 16) == 9 && (t[1].e[11] >> 16) == 11);           // the DC part of kMaxBlockBits
        CHECK((t[2].e[0xF0] >> 16) == 11 && (t[3].e[0xF0] >> 16) == 10 && (t[2].e[0] >> 16) == 4 && (t[3].e[0] >> 16) == 2);
    }
    // header: exactly kHeaderBytes into a buffer of exactly that size, for both subsamplings and the corner sizes
    const int dims[4] = {1, 8, 17, 8192};
    for (int ss : {420, 444})
        for (int H : dims)
            for (int W : dims) {
                std::vector<uint8_t> h(kHeaderBytes);
                CHECK(header(H, W, 75, ss, 16, h.data()) == kHeaderBytes);
                CHECK(h[0] == 0xFF && h[1] == 0xD8 && h[kHeaderBytes - 14] == 0xFF && h[kHeaderBytes - 13] == 0xDA);
                CHECK(h[163] == (H >> 8) && h[164] == (H & 255) && h[165] == (W >> 8) && h[166] == (W & 255));
                CHECK(h[169] == (ss == 420 ? 0x22 : 0x11));
            }
    {
        std::vector<uint8_t> h(kHeaderBytes);
        CHECK(header(0, 8, 75, 420, 1, h.data()) == -1 && header(8, 8193, 75, 420, 1, h.data()) == -1);
        CHECK(header(8, 8, 75, 422, 1, h.data()) == -1 && header(8, 8, 75, 420, 0, h.data()) == -1);
        CHECK(header(8, 8, 0, 420, 1, h.data()) == -1 && header(8, 8, 75, 420, 65536, h.data()) == -1);
    }
    // bound and workspace arithmetic
    for (int ss : {420, 444})
        for (int H : dims)
            for (int W : dims)
                for (int R : {1, 3, 8, 512, 65535}) {
                    const Geometry g = geometry(H, W, ss, R);
                    const int m = mcu_size(ss);
                    CHECK(g.mcus_x * m >= W && (g.mcus_x - 1) * m < W && g.mcus_y * m >= H && (g.mcus_y - 1) * m < H);
                    CHECK(g.intervals * R >= g.mcus && (g.intervals - 1) * R < g.mcus);
                    const int64_t mb = max_bytes(H, W, ss, R);
                    // every block's worst case, twice (stuffing), plus marker and fill per interval
                    const int64_t blocks_bytes = 2 * ((g.blocks * kMaxBlockBits + 7) / 8);
                    CHECK(mb >= kHeaderBytes + blocks_bytes + 2 * g.intervals);
                    CHECK(mb <= kHeaderBytes + blocks_bytes + 4 * g.intervals);
                    CHECK(mb < (int64_t)1 << 31);                              // out_len and the offsets are 32 bits
                    for (int B : {1, 16}) {
                        const Workspace w = workspace(B, H, W, ss, R);
                        CHECK(w.count >= w.coef + B * g.blocks * 128 && w.offset >= w.count + B * g.intervals * 4);
                        CHECK(w.stage >= w.offset + B * g.intervals * 4 && w.total >= w.stage + B * g.intervals * w.slot);
                        CHECK(w.count % 256 == 0 && w.offset % 256 == 0 && w.stage % 256 == 0);
                        CHECK(w.slot >= interval_bound(g.mcus < R ? g.mcus : R, g.bpm));
                        CHECK(workspace_bytes(B, H, W, ss, R) == w.total);
                        CHECK(kHeaderBytes + g.intervals * w.slot >= mb);      // the staging area holds the bound
                    }
                }
    CHECK(max_bytes(8193, 8, 420, 1) == -1 && workspace_bytes(17, 8, 8, 420, 1) == -1 && workspace_bytes(0, 8, 8, 420, 1) == -1);
    std::printf("jpeg_host: ok\n");
    return 0;
}
