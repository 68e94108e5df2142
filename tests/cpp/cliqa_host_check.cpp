// CPU check of nunif_amd/csrc/cliqa_host.h (tests/test_cliqa_host.py builds this with the host sanitizers and runs it).
//
// Groups and workspace: for corner shapes of the accepted range the group size stays inside its bounds, the groups cover the
// batch, the seven regions are 256-byte aligned, disjoint, each as large as the kernels' own extent of it (restated here from the
// kernels' index expressions), and add up to the total that nunif_hip_cliqa_workspace_bytes reports for the same arguments.
// Weights: both streams are checked by the INVERSE of the fragment layout against a direct [n][k] matrix, every half no element
// maps to (the padded taps and channel slots, the ring padding behind the last k-step) must be zero, and the stream is long
// enough for the furthest chunk tile_conv requests.  No HIP call is made.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../nunif_amd/csrc/cliqa_host.h"

static std::string g_error;
namespace nunif {
void set_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace nunif

using namespace nunif;
namespace C = nunif::cliqa_host;

static int g_failed = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (++g_failed <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                 \
    } while (0)

static uint16_t bits_of(f16 h) { uint16_t b; memcpy(&b, &h, 2); return b; }
static float value(long index) {               // a distinct, non-zero fp16 per index below 2^15 - 0x0400, exact in float
    const uint16_t bits = (uint16_t)(0x0400 + index);
    f16 h;
    memcpy(&h, &bits, 2);
    return (float)h;
}

// where row n, column k of an [N][K] matrix lies in a [k-step][n-tile] stream (host_weights.h, the kernels' reading order)
static size_t place(int N, int n, int k) {
    const size_t frag = (size_t)(k / 32) * (N / 16) + n / 16;
    return (frag * 64 + ((k % 32) / 8) * 16 + n % 16) * 8 + k % 8;
}

static void check_geometry(int heads, int B, int H, int W, int group) {
    const int G = C::group_size(B, H, W, group);
    const long cap = std::max<long>(1, C::kGroupPixels / ((long)H * W));
    CHECK(G >= 1 && G <= B && G <= C::kMaxGroup && G <= cap && (group <= 0 || G <= group), "group_size(%d, %d, %d, %d) = %d", B, H, W,
          group, G);
    CHECK(G == std::min<long>(std::min<long>(group > 0 ? std::min<long>(cap, group) : cap, B), C::kMaxGroup), "group_size not maximal");
    long covered = 0;
    int passes = 0;
    for (int b0 = 0; b0 < B; b0 += G, ++passes) {
        const int n = std::min(G, B - b0);
        CHECK(n >= 1 && n <= G, "pass of %d images", n);
        covered += n;
    }
    CHECK(covered == B && passes == (B + G - 1) / G, "groups cover %ld of %d images", covered, B);
    const C::Geometry q = C::geometry(heads, G, H, W);
    CHECK(q.H1 == H / 2 && q.H2 == H / 4 && q.H3 == H / 8 && q.W1 == W / 2 && q.W2 == W / 4 && q.W3 == W / 8 && q.H3 >= 1 && q.W3 >= 1,
          "pooled sizes of %d x %d", H, W);
    // the furthest byte each launch touches, from the kernels' index expressions: pixel (G - 1, h - 1, w - 1), last channel
    const long need[7] = {((((long)G - 1) * H + H - 1) * W + W - 1) * 64 * 2 + 128,
                          ((((long)G - 1) * q.H1 + q.H1 - 1) * q.W1 + q.W1 - 1) * 128 * 2 + 256, 0,
                          ((((long)G - 1) * q.H2 + q.H2 - 1) * q.W2 + q.W2 - 1) * 128 * 2 + 256, 0,
                          ((((long)G - 1) * q.H3 + q.H3 - 1) * q.W3 + q.W3 - 1) * 128 * 2 + 256,
                          (((((long)G - 1) * heads + heads - 1) * q.tiles3 + q.tiles3 - 1) * 256 + 255) * 4 + 4};
    const int tiles = ((q.H3 + 7) / 8) * ((q.W3 + 15) / 16);
    CHECK(q.tiles3 == tiles && tiles >= 1, "tiles3 %d", q.tiles3);
    long sum = 0;
    for (int i = 0; i < 7; ++i) {
        const long o = q.offset(i), want = i == 2 ? need[1] : i == 4 ? need[3] : need[i];
        CHECK(o % 256 == 0 && o >= 0, "region %d at %ld is not aligned", i, o);
        CHECK(q.size[i] == want, "region %d holds %ld bytes, the kernels reach %ld", i, q.size[i], want);
        CHECK(o == sum, "region %d at %ld, the regions before it end at %ld", i, o, sum);             // packed in order: disjoint
        CHECK(o + q.size[i] <= q.total, "region %d ends behind the total", i);
        sum += C::align256(q.size[i]);
    }
    CHECK(q.total == sum && q.total > 0, "total %ld, regions add up to %ld", q.total, sum);
    CHECK(C::workspace_bytes(heads, B, H, W, group) == q.total, "workspace_bytes differs from forward's geometry");
}

static void check_conv_stream(int cout, int cin, int n0) {
    std::vector<float> w((size_t)cout * cin * 9);
    // values cycle below 2^15 - 0x0400 indices; the cycle length 30011 is prime, so neighbours in any direction differ
    for (size_t i = 0; i < w.size(); ++i) w[i] = value((long)(i % 30011));
    const int K = 9 * cin, KS = K / 32;
    const std::vector<f16> s = C::conv_stream(w.data(), cin, n0);
    CHECK(s.size() == (size_t)128 * K + kRingPadHalfs, "conv_stream: %zu halfs", s.size());
    // tile_conv requests chunks 0 .. KS (512 x 16 bytes each): the last one is padding and must exist and be zero
    CHECK(s.size() * sizeof(f16) >= (size_t)(KS + 1) * 512 * 16, "conv_stream: no room for chunk %d", KS);
    std::vector<char> seen(s.size(), 0);
    for (int n = 0; n < 128; ++n)
        for (int k = 0; k < K; ++k) {
            const int tap = k / cin, ci = k % cin;
            const size_t direct = ((size_t)(n0 + n) * cin + ci) * 9 + tap;      // w[n0 + n][ci][tap / 3][tap % 3]
            CHECK((long)direct == C::conv_weight_index(n0 + n, k, cin), "conv_weight_index(%d, %d)", n0 + n, k);
            const size_t at = place(128, n, k);
            CHECK(at < (size_t)128 * K && !seen[at], "conv_stream: (%d, %d) maps to %zu", n, k, at);
            if (at >= (size_t)128 * K) continue;
            seen[at] = 1;
            CHECK(bits_of(s[at]) == bits_of((f16)w[direct]), "conv_stream cin %d n0 %d: (%d, %d)", cin, n0, n, k);
        }
    for (size_t i = 0; i < s.size(); ++i)
        if (!seen[i]) CHECK(bits_of(s[i]) == 0, "conv_stream: half %zu is not zero", i);
}

static void check_entry_stream(int cin) {
    std::vector<float> w((size_t)64 * cin * 9);
    for (size_t i = 0; i < w.size(); ++i) w[i] = value((long)i);
    const std::vector<f16> s = C::entry_stream(w.data(), cin);
    CHECK(s.size() == (size_t)64 * C::kEntryK + kRingPadHalfs, "entry_stream: %zu halfs", s.size());
    CHECK(s.size() >= (size_t)3 * 4 * kFragHalfs, "entry_stream: 12 fragments");
    std::vector<char> seen(s.size(), 0);
    for (int n = 0; n < 64; ++n)
        for (int k = 0; k < C::kEntryK; ++k) {
            // the kernel: k-step ks, lane group g, slot j read tap 4 ks + g, channel j
            const int ks = k / 32, g = (k % 32) / 8, tap = 4 * ks + g, c = k % 8;
            const bool real = tap < 9 && c < cin;
            const size_t at = place(64, n, k);
            CHECK(at < (size_t)64 * C::kEntryK && !seen[at], "entry_stream: (%d, %d) maps to %zu", n, k, at);
            if (at >= (size_t)64 * C::kEntryK) continue;
            seen[at] = 1;
            const uint16_t want = real ? bits_of((f16)w[((size_t)n * cin + c) * 9 + tap]) : 0;
            CHECK(bits_of(s[at]) == want, "entry_stream cin %d: (%d, tap %d, channel %d)", cin, n, tap, c);
            CHECK((C::entry_weight_index(n, k, cin) >= 0) == real, "entry_weight_index(%d, %d)", n, k);
        }
    for (size_t i = 0; i < s.size(); ++i)
        if (!seen[i]) CHECK(bits_of(s[i]) == 0, "entry_stream: half %zu is not zero", i);
}

int main() {
    CHECK(!C::shape_ok(0, 8, 8) && !C::shape_ok(1, 7, 8) && !C::shape_ok(1, 8, 7) && C::shape_ok(1, 8, 8), "shape_ok: lower corners");
    CHECK(C::shape_ok(1, 8192, 8192) && !C::shape_ok(1, 8192, 8193) && C::shape_ok(1, 8, 1 << 23) && !C::shape_ok(1, 65536, 65536),
          "shape_ok: H W = 2^26");
    CHECK(C::workspace_bytes(1, 1, 7, 8, 0) == 0 && C::workspace_bytes(3, 1, 8, 8, 0) == 0 && C::workspace_bytes(0, 1, 8, 8, 0) == 0 &&
          C::workspace_bytes(1, 1, 8192, 8193, 0) == 0, "workspace_bytes: refused shapes");
    const int shapes[][2] = {{8, 8}, {9, 15}, {16, 24}, {21, 30}, {40, 56}, {128, 128}, {135, 241}, {1080, 1920}, {2896, 2896},
                             {8192, 8192}, {8, 1 << 23}, {1 << 23, 8}};
    const int batches[] = {1, 2, 8, 9, 511, 512, 513, 32768, 32769, 100000};
    const int groups[] = {0, -1, 1, 2, 8, 100, 32768, 40000, 1 << 30};
    for (const auto &hw : shapes)
        for (int B : batches)
            for (int group : groups)
                for (int heads = 1; heads <= 2; ++heads) check_geometry(heads, B, hw[0], hw[1], group);
    CHECK(C::group_size(100000, 8, 8, 0) == 32768 && C::group_size(100000, 8, 8, 40000) == 32768, "G = 32768");
    CHECK(C::group_size(600, 128, 128, 0) == 512 && C::group_size(600, 128, 128, 1000) == 512 && C::group_size(5, 128, 128, 9) == 5,
          "512 patches of 128 x 128 per group; group > B");
    CHECK(C::group_size(4, 8192, 8192, 0) == 1 && C::group_size(4, 8192, 8192, 4) == 1, "one image beyond the group's pixels");
    CHECK(C::geometry(2, 512, 128, 128).total < (1L << 32), "512 patches need less than 4 GiB");
    check_conv_stream(128, 64, 0);
    check_conv_stream(128, 128, 0);
    check_conv_stream(256, 128, 0);
    check_conv_stream(256, 128, 128);
    check_entry_stream(3);
    check_entry_stream(6);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("cliqa_host: ok\n");
    return 0;
}
