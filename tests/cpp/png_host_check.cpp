// Stand-alone check of nunif_amd/csrc/png_host.h, built with the host sanitizers by tests/test_png_host.py: the header writer, the
// CRC table and the powers of x against known vectors, and the arithmetic of the bound and of the workspace at the corners of the
// accepted range.  No HIP call; nothing here runs on a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nunif_amd/csrc/png_host.h"

using namespace nunif::png;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                       \
        }                                                                   \
    } while (0)

// raw CRC: start 0, no final complement
static uint32_t raw_crc(const CrcTable &t, const uint8_t *p, size_t n) {
    uint32_t c = 0;
    for (size_t i = 0; i < n; ++i) c = t.e[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c;
}

int main() {
    // CRC-32: the check value of "123456789", the CRC of IEND that every PNG file ends with, the table's corner entries
    const CrcTable t = crc_table();
    CHECK(t.e[0] == 0u && t.e[1] == 0x77073096u && t.e[255] == 0x2D02EF8Du);
    CHECK(crc32(reinterpret_cast<const uint8_t *>("123456789"), 9) == 0xCBF43926u);
    CHECK(crc32(reinterpret_cast<const uint8_t *>("IEND"), 4) == 0xAE426082u);
    // the powers of x: appending zeros, and crc(A || B) = crc(A) x^(8 |B|) + crc(B) for pieces of 16 bytes and a shorter tail
    const CrcPowers pw = crc_powers();
    CHECK(pw.pow1[0] == 0x80000000u && pw.pow16[0] == 0x80000000u && crc_mul(pw.pow1[1], 0x80000000u) == pw.pow1[1]);
    std::vector<uint8_t> msg(16 * kCrcPieces + 15);
    uint32_t seed = 12345u;
    for (auto &b : msg) { seed = seed * 1664525u + 1013904223u; b = (uint8_t)(seed >> 24); }
    for (int pieces : {1, 2, 3, 255, 256, kCrcPieces})
        for (int rest : {0, 1, 7, 15}) {
            uint32_t acc = 0;
            for (int k = 0; k < pieces; ++k) acc ^= crc_mul(raw_crc(t, msg.data() + 16 * k, 16), pw.pow16[pieces - 1 - k]);
            CHECK(acc == raw_crc(t, msg.data(), 16 * (size_t)pieces));
            // a state carried in, as the emit kernel does from flush to flush
            const uint32_t carried = crc_mul(0xDEADBEEFu, pw.pow16[pieces]) ^ acc;
            std::vector<uint8_t> zeros(16 * (size_t)pieces, 0);
            uint32_t c = 0xDEADBEEFu;
            for (size_t i = 0; i < zeros.size(); ++i) c = t.e[c & 255u] ^ (c >> 8);
            CHECK(carried == (c ^ acc));
            if (rest) {
                const uint32_t whole = crc_mul(acc, pw.pow1[rest]) ^ raw_crc(t, msg.data() + 16 * pieces, rest);
                CHECK(whole == raw_crc(t, msg.data(), 16 * (size_t)pieces + rest));
            }
        }
    // the start value 0xFFFFFFFF complements the first four bytes of a message
    {
        uint8_t m[12] = {'I', 'D', 'A', 'T', 1, 2, 3, 4, 5, 6, 7, 8};
        const uint32_t want = crc32(m, 12);
        for (int i = 0; i < 4; ++i) m[i] ^= 255;
        CHECK((raw_crc(t, m, 12) ^ 0xFFFFFFFFu) == want);
    }
    // deflate constants
    for (int k = 0; k + 1 < 29; ++k) CHECK(k == 27 || kLenBase[k] + (1 << kLenExtra[k]) == kLenBase[k + 1]);
    CHECK(kLenBase[0] == kMinMatch && kLenBase[28] == kMaxMatch && kLenBase[27] + 31 == 258);
    {
        int seen[19] = {0};
        for (int i = 0; i < 19; ++i) seen[kClOrder[i]]++;
        for (int i = 0; i < 19; ++i) CHECK(seen[i] == 1);
    }
    // the header writer: exact size, the size it reports, a capacity one byte short, refused arguments
    const int dims[4] = {1, 2, 17, 8192};
    const char *keys[2] = {"iw3_min_depth_value", "k"};
    const char *vals[2] = {"0.5", ""};
    for (int form : {0, 1, 2})
        for (int H : dims)
            for (int W : dims)
                for (int n_text : {0, 1, 2}) {
                    int64_t want = 8 + 25;
                    for (int i = 0; i < n_text; ++i) want += 12 + (int64_t)std::strlen(keys[i]) + 1 + (int64_t)std::strlen(vals[i]);
                    std::vector<uint8_t> h((size_t)want);
                    CHECK(header(H, W, form, keys, vals, n_text, h.data(), want) == want);
                    CHECK(h[0] == 0x89 && h[1] == 'P' && h[12] == 'I' && h[15] == 'R');
                    CHECK(h[16] == 0 && h[17] == 0 && h[18] == (W >> 8) && h[19] == (W & 255) && h[22] == (H >> 8) && h[23] == (H & 255));
                    CHECK(h[24] == (form == 2 ? 16 : 8) && h[25] == (form == 2 ? 0 : 2) && h[26] == 0 && h[27] == 0 && h[28] == 0);
                    const uint32_t crc = crc32(h.data() + 12, 17);
                    CHECK(h[29] == (crc >> 24) && h[32] == (crc & 255u));
                    if (n_text) CHECK(std::memcmp(h.data() + 37, "tEXt", 4) == 0 && h[41] == 'i');
                    std::vector<uint8_t> small((size_t)want - 1);
                    CHECK(header(H, W, form, keys, vals, n_text, small.data(), want - 1) == -2);
                }
    {
        std::vector<uint8_t> h(256);
        const char *long_key[1] = {"0123456789012345678901234567890123456789012345678901234567890123456789012345678901234567890"};
        const char *empty_key[1] = {""};
        CHECK(header(0, 8, 0, nullptr, nullptr, 0, h.data(), 256) == -1 && header(8, 8193, 0, nullptr, nullptr, 0, h.data(), 256) == -1);
        CHECK(header(8, 8, 3, nullptr, nullptr, 0, h.data(), 256) == -1 && header(8, 8, 0, nullptr, nullptr, 1, h.data(), 256) == -1);
        CHECK(header(8, 8, 0, long_key, vals, 1, h.data(), 256) == -1 && header(8, 8, 0, empty_key, vals, 1, h.data(), 256) == -1);
    }
    // bound and workspace arithmetic
    for (int form : {0, 1, 2})
        for (int H : dims)
            for (int W : dims)
                for (int S : {1, 16, H}) {
                    if (S > H) continue;
                    const Geometry g = geometry(H, W, form, S);
                    CHECK(g.row == 1 + (int64_t)W * (form == 2 ? 2 : 3));
                    CHECK((int64_t)g.stripes * S >= H && (int64_t)(g.stripes - 1) * S < H);
                    const int64_t mb = max_bytes(H, W, form, S);
                    const int64_t n = (int64_t)H * g.row;
                    // 15 bits per filtered byte, and per stripe between 293 and 294 bytes of header, end and chunk
                    CHECK(mb >= 15 * n / 8 + (int64_t)g.stripes * (12 + 4 + 288) + 18);
                    CHECK(mb <= 15 * n / 8 + (int64_t)g.stripes * (12 + 4 + 290) + 18);
                    CHECK(mb < (int64_t)1 << 31);                              // out_len and the offsets are 32 bits
                    for (int B : {1, 16}) {
                        const Workspace w = workspace(B, H, W, form, S);
                        const int64_t ns = (int64_t)B * g.stripes;
                        CHECK(w.stripe_stride % 16 == 0 && w.stripe_stride >= g.stripe_bytes && w.stripe_stride < g.stripe_bytes + 16);
                        const int64_t start[9] = {w.filtered, w.rowsum, w.hist, w.lens, w.codes, w.header, w.meta, w.frame, w.total};
                        const int64_t size[8] = {ns * w.stripe_stride, (int64_t)B * H * 8, ns * kSymbolStride * 4, ns * kSymbolStride * 4,
                                                 ns * kCodeWords * 4, ns * kHeaderWords * 4, ns * 16, (int64_t)B * 16};
                        for (int k = 0; k < 8; ++k) {
                            CHECK(start[k] % 256 == 0 && size[k] > 0);
                            CHECK(start[k] + size[k] <= start[k + 1]);          // aligned and disjoint
                        }
                        CHECK(workspace_bytes(B, H, W, form, S) == w.total);
                    }
                }
    CHECK(kSymbols == 335 && kSymbolStride >= kSymbols && kCodeWords > kNumLit && kHeaderWords * 32 >= 74 + 316 * 14);
    CHECK(stripe_data_bound(1) == (2304 + 15 + 7) / 8 + 4);
    CHECK(max_bytes(8193, 8, 0, 1) == -1 && max_bytes(8, 8, 0, 9) == -1 && max_bytes(8, 8, 0, 0) == -1);
    CHECK(workspace_bytes(17, 8, 8, 0, 1) == -1 && workspace_bytes(0, 8, 8, 0, 1) == -1 && workspace_bytes(1, 8, 8, 3, 1) == -1);
    std::printf("png_host: ok\n");
    return 0;
}
