// CPU check of nunif_amd/csrc/packed_layers.h (tests/test_packed_layers_host.py builds this with the host sanitizers and runs it).
//
// As in host_weights_check.cpp the packers are not restated: each packing is checked by its INVERSE.  For every element of a
// matrix or conv weight the fragment, lane and slot where the kernels will look for it is computed and the half found there is
// compared; every half not reached that way (the padding of N, K and Cin, the ring pad behind the last fragment) must be zero.
// Test values are the fp16 numbers with bit pattern 0x3C00 + index: distinct, exact in float, never zero.  The argument builders
// are compared field by field against a value-initialised struct with the documented fields set.  No HIP call is made and nothing
// is launched.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>

#include "../../nunif_amd/csrc/packed_layers.h"

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

static int g_failed = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (++g_failed <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                 \
    } while (0)

static float value(int index) {               // the fp16 with bits 0x3C00 + index (index < 16 383: finite), as a float
    const uint16_t bits = (uint16_t)(0x3C00 + index);
    f16 h;
    memcpy(&h, &bits, 2);
    return (float)h;
}
static uint16_t bits_of(f16 h) { uint16_t b; memcpy(&b, &h, 2); return b; }

// the half of element (n, kk) inside fragment `frag` (kk = the element's index inside the fragment's 32 k-slots)
static size_t in_frag(size_t frag, bool chained, int n, int kk) {
    if (!chained) return (frag * 64 + (kk / 8) * 16 + n % 16) * 8 + kk % 8;
    return (frag * 64 + ((kk % 16) / 4) * 16 + n % 16) * 8 + kk % 4 + 4 * (kk / 16);
}

// `frags` fragments + the ring pad; expect(at) = index whose value must sit at half `at`, filled by the caller through put()
struct Inverse {
    const char *what;
    const std::vector<f16> &packed;
    size_t halfs;
    std::vector<char> seen;
    Inverse(const char *w, const std::vector<f16> &p, size_t frags) : what(w), packed(p), halfs(frags * kFragHalfs) {
        CHECK(packed.size() == halfs + kRingPadHalfs, "%s: %zu halfs, expected %zu", what, packed.size(), halfs + kRingPadHalfs);
        seen.assign(packed.size(), 0);
    }
    void put(size_t at, int index, int n, int k) {             // index < 0: zero
        CHECK(at < halfs && at < packed.size() && !seen[at], "%s: (%d, %d) maps to %zu (outside or twice)", what, n, k, at);
        if (at >= halfs || at >= packed.size()) return;
        seen[at] = 1;
        const uint16_t want = index < 0 ? 0 : (uint16_t)(0x3C00 + index);
        CHECK(bits_of(packed[at]) == want, "%s: (%d, %d) at %zu holds 0x%04x, expected 0x%04x", what, n, k, at, bits_of(packed[at]), want);
    }
    void rest_is_zero() {
        for (size_t i = 0; i < packed.size(); ++i)
            if (!seen[i]) CHECK(bits_of(packed[i]) == 0, "%s: half %zu (no element's place) is 0x%04x", what, i, bits_of(packed[i]));
    }
};

// pack_linear of rows n < n_real, columns k0 .. k0 + K_real of a [n_real][Kt] matrix
static void linear_case(const char *what, int n_real, int granule, int N_want, int K_real, int K, int k0, int Kt, bool chained, bool with_bias) {
    int outside = 0;
    std::vector<float> bias(n_real);
    for (int n = 0; n < n_real; ++n) bias[n] = 0.5f + n;
    auto wt = [&](int n, int k) { if (n >= n_real || k >= K_real) ++outside; return value(n * Kt + k0 + k); };
    auto bs = [&](int n) { if (n >= n_real) ++outside; return with_bias ? bias[n] : 0.f; };
    const LinearHost L = with_bias ? pack_linear(n_real, granule, K_real, K, chained, wt, bs)
                                   : pack_linear(n_real, granule, K_real, K, chained, wt, bias_at(nullptr));
    CHECK(outside == 0, "%s: a functor was asked %d times outside the real range", what, outside);
    CHECK(L.N == N_want && L.n_real == n_real && L.K == K, "%s: N %d n_real %d K %d", what, L.N, L.n_real, L.K);
    CHECK((int)L.bias.size() == L.N, "%s: bias of %zu", what, L.bias.size());
    for (int n = 0; n < (int)L.bias.size(); ++n)
        CHECK(L.bias[n] == (with_bias && n < n_real ? bias[n] : 0.f), "%s: bias[%d] = %f", what, n, L.bias[n]);
    const int KS = K / 32;
    Inverse inv(what, L.w, (size_t)(L.N / 16) * KS);
    for (int n = 0; n < L.N; ++n)
        for (int k = 0; k < K; ++k)
            inv.put(in_frag((size_t)(n / 16) * KS + k / 32, chained, n, k % 32), n < n_real && k < K_real ? n * Kt + k0 + k : -1, n, k);
    inv.rest_is_zero();
}

// pack_conv of a [cout][cin_real][k][k] weight
static void conv_case(const char *what, int cout, int granule, int N_want, int cin_real, int cin, int k, int cmaj, bool with_bias) {
    int outside = 0;
    const int taps = k * k;
    auto index = [&](int n, int tap, int ci) { return (n * cin_real + ci) * taps + tap; };
    auto wt = [&](int n, int tap, int ci) { if (n >= cout || ci >= cin_real || tap >= taps) ++outside; return value(index(n, tap, ci)); };
    auto bs = [&](int n) { if (n >= cout) ++outside; return 0.25f + n; };
    const ConvHost C = with_bias ? pack_conv(cout, granule, cin_real, cin, k, cmaj, wt, bs)
                                 : pack_conv(cout, granule, cin_real, cin, k, cmaj, wt, bias_at(nullptr));
    CHECK(outside == 0, "%s: a functor was asked %d times outside the real range", what, outside);
    CHECK(C.N == N_want && C.n_real == cout && C.Cin == cin && C.k == k && C.cmaj == cmaj, "%s: N %d n_real %d Cin %d k %d cmaj %d", what,
          C.N, C.n_real, C.Cin, C.k, C.cmaj);
    CHECK((int)C.bias.size() == C.N, "%s: bias of %zu", what, C.bias.size());
    for (int n = 0; n < (int)C.bias.size(); ++n)
        CHECK(C.bias[n] == (with_bias && n < cout ? 0.25f + n : 0.f), "%s: bias[%d] = %f", what, n, C.bias[n]);
    const int NT = C.N / 16;
    Inverse inv(what, C.stream, (size_t)NT * taps * cin / 32);
    for (int n = 0; n < C.N; ++n)
        for (int tap = 0; tap < taps; ++tap)
            for (int ci = 0; ci < cin; ++ci) {
                // tap-major: k-step of k = tap * cin + ci; chunk-major: [chunk of cmaj channels][tap][32-channel part]
                const size_t step = cmaj ? ((size_t)(ci / cmaj) * taps + tap) * (cmaj / 32) + (ci % cmaj) / 32 : (size_t)(tap * cin + ci) / 32;
                inv.put(in_frag(step * NT + n / 16, false, n, ci % 32), n < cout && ci < cin_real ? index(n, tap, ci) : -1, n, tap * cin + ci);
            }
    inv.rest_is_zero();
}

// every field of the argument structs, so that a field a builder is NOT documented to set is seen to be zero / its default
#define EQ(f) CHECK(a.f == b.f, "%s: field " #f " differs", what)
static void same(const char *what, const GemmArgs &a, const GemmArgs &b) {
    EQ(a); EQ(B); EQ(Hi); EQ(Wi); EQ(Cin); EQ(Ho); EQ(Wo); EQ(stride); EQ(oy); EQ(ox); EQ(kw); EQ(K); EQ(w); EQ(bias); EQ(N); EQ(mode);
    EQ(act); EQ(slope); EQ(res); EQ(out); EQ(ldo); EQ(n_real); EQ(ps); EQ(oshift); EQ(OH); EQ(OW); EQ(no_clamp); EQ(lda); EQ(rev);
    EQ(nt_chunk); EQ(res_H); EQ(res_W); EQ(res_crop); EQ(in_scale);
}
static void same(const char *what, const GemmOsArgs &a, const GemmOsArgs &b) {
    EQ(a); EQ(M); EQ(lda); EQ(K); EQ(w); EQ(bias); EQ(N); EQ(act); EQ(res); EQ(out); EQ(ldo); EQ(stats_out); EQ(stats_in);
    EQ(stats_parts); EQ(wsum); EQ(ln_eps);
}
static void same(const char *what, const ConvArgs &a, const ConvArgs &b) {
    EQ(a); EQ(a2); EQ(H2); EQ(W2); EQ(crop2); EQ(B); EQ(Hi); EQ(Wi); EQ(Cin); EQ(Ho); EQ(Wo); EQ(stride); EQ(kh); EQ(kw); EQ(wstream);
    EQ(bias); EQ(N); EQ(n_real); EQ(act); EQ(slope); EQ(out); EQ(out32); EQ(add32); EQ(addH); EQ(addW); EQ(add_crop); EQ(clamp01);
    EQ(rpad); EQ(res); EQ(zpad); EQ(relu_in); EQ(res2); EQ(ldo); EQ(cmaj); EQ(part32);
}
#undef EQ
static_assert(sizeof(GemmArgs) == 168 && sizeof(GemmOsArgs) == 112 && sizeof(ConvArgs) == 184,
              "a field was added to an argument struct: add it to same() above, then update these sizes");

int main() {
    // ---- Linear: N padded to 16 and to 32 and given padded, K_real < K, a column window, chained, bias absent -------------------
    linear_case("27 -> 32 by 16", 27, 16, 32, 64, 64, 0, 64, false, true);
    linear_case("40 -> 64 by 32", 40, 32, 64, 64, 64, 0, 64, false, true);
    linear_case("48 given padded", 48, 16, 48, 96, 96, 0, 96, false, true);
    linear_case("K 40 of 64", 20, 16, 32, 40, 64, 0, 40, false, true);
    linear_case("window 33 .. 97 of 161", 40, 32, 64, 64, 64, 33, 161, false, true);
    linear_case("chained", 48, 16, 48, 64, 64, 0, 64, true, true);
    linear_case("chained, K 40 of 64, no bias", 27, 32, 32, 40, 64, 0, 40, true, false);
    linear_case("no bias", 16, 16, 16, 32, 32, 0, 32, false, false);
    // ---- conv: k = 1, 2, 3, cin_real < cin, chunk-major 32 and 64, bias absent; NT = 2 or 3 != the k-step count ---------------------
    conv_case("1x1", 40, 16, 48, 64, 64, 1, 0, true);
    conv_case("2x2", 24, 16, 32, 32, 32, 2, 0, true);
    conv_case("3x3 to 32", 40, 32, 64, 32, 32, 3, 0, true);
    conv_case("3x3 cin 3 of 32", 16, 16, 16, 3, 32, 3, 0, true);
    conv_case("3x3 cin 40 of 64, no bias", 20, 16, 32, 40, 64, 3, 0, false);
    conv_case("3x3 chunks of 32", 24, 16, 32, 40, 64, 3, 32, false);
    conv_case("3x3 chunks of 64", 24, 16, 32, 70, 128, 3, 64, true);
    conv_case("1x1 chunks of 32", 48, 16, 48, 96, 96, 1, 32, true);

    // ---- builders -------------------------------------------------------------------------------------------------------------
    f16 buf[256];
    float fb[256];
    const f16 *a = buf + 1;
    f16 *out = buf + 2;
    PackedLinear L;
    L.w = buf + 3; L.bias = fb + 1; L.N = 48; L.n_real = 40; L.K = 96;
    {
        GemmArgs e{};
        e.a = a; e.B = 1; e.Hi = 1; e.Wi = 777; e.Cin = 96; e.Ho = 1; e.Wo = 777; e.stride = 1; e.kw = 1; e.K = 96; e.w = L.w; e.bias = L.bias;
        e.N = 48; e.n_real = 40; e.out = out; e.ldo = 40; e.ps = 1;
        same("gemm_token_args", gemm_token_args(L, a, 777, out), e);
    }
    {
        GemmArgs e{};
        e.a = a; e.B = 3; e.Hi = 10; e.Wi = 12; e.Cin = 96; e.Ho = 10; e.Wo = 12; e.stride = 1; e.kw = 1; e.K = 96; e.w = L.w; e.bias = L.bias;
        e.N = 48; e.n_real = 40; e.out = out; e.ldo = 40; e.ps = 1;
        same("gemm_map_args 1x1", gemm_map_args(L, a, 3, 10, 12, 96, 10, 12, out), e);
        e.Cin = 24; e.Ho = 5; e.Wo = 6; e.stride = 2; e.kw = 2; e.oy = 1; e.ox = 3;
        same("gemm_map_args gather", gemm_map_args(L, a, 3, 10, 12, 24, 5, 6, out, 2, 2, 1, 3), e);
    }
    {
        GemmOsArgs e{};
        e.a = a; e.M = (1L << 33) + 5; e.lda = 96; e.K = 96; e.w = L.w; e.bias = L.bias; e.N = 48; e.out = out; e.ldo = 48;
        same("gemm_os_args", gemm_os_args(L, a, (1L << 33) + 5, out), e);
    }
    PackedConv C;
    C.stream = buf + 4; C.bias = fb + 2; C.N = 64; C.n_real = 48; C.Cin = 96; C.k = 3; C.cmaj = 32;
    {
        ConvArgs e{};
        e.a = a; e.B = 2; e.Hi = 21; e.Wi = 30; e.Cin = 96; e.stride = 1; e.kh = 3; e.kw = 3; e.wstream = C.stream; e.bias = C.bias; e.N = 64;
        e.n_real = 48; e.out = out; e.cmaj = 32;
        e.Ho = 19; e.Wo = 28;
        same("conv_args valid", conv_args(C, a, 2, 21, 30, out), e);
        e.Ho = 21; e.Wo = 30; e.zpad = 1;
        same("conv_args zpad", conv_args(C, a, 2, 21, 30, out, 1, 1), e);
        e.zpad = 0; e.rpad = 1;
        same("conv_args rpad", conv_args(C, a, 2, 21, 30, out, 1, 0, 1), e);
        e.rpad = 0; e.zpad = 1; e.stride = 2; e.Ho = (21 + 2 - 3) / 2 + 1; e.Wo = (30 + 2 - 3) / 2 + 1;
        same("conv_args zpad stride 2", conv_args(C, a, 2, 21, 30, out, 2, 1), e);
        PackedConv C2 = C;
        C2.k = 2; C2.cmaj = 0;
        e.zpad = 0; e.kh = e.kw = 2; e.cmaj = 0; e.Ho = (21 - 2) / 2 + 1; e.Wo = (30 - 2) / 2 + 1;
        same("conv_args 2x2 stride 2", conv_args(C2, a, 2, 21, 30, out, 2), e);
    }
    // ---- slices: 96 channels as 64 + 32; bias / out / res / res2 move by the slice's first channel, ldo = the whole width --------
    {
        PackedConv W;
        W.stream = buf; W.bias = fb; W.N = 96; W.n_real = 96; W.Cin = 32; W.k = 3;
        ConvArgs cv = conv_args(W, a, 2, 16, 16, out, 1, 0, 1);
        cv.act = 2; cv.slope = 0.2f; cv.relu_in = 1;
        const ConvSlice sl[2] = {{buf + 5, 4}, {buf + 6, 2}};
        int n0 = 0;
        for (int q = 0; q < 2; ++q) {
            ConvArgs e = cv;
            e.wstream = sl[q].stream; e.N = e.n_real = 16 * sl[q].nt; e.bias = fb + n0; e.out = out + n0; e.ldo = 96;
            same("slice without residual", conv_slice_args(cv, sl[q], n0), e);
            n0 += 16 * sl[q].nt;
        }
        CHECK(n0 == 96, "slices cover %d channels", n0);
        cv.res = buf + 1; cv.res2 = buf + 2; cv.ldo = 192;
        ConvArgs e = cv;
        e.wstream = sl[1].stream; e.N = e.n_real = 32; e.bias = fb + 64; e.out = out + 64; e.res = buf + 1 + 64; e.res2 = buf + 2 + 64; e.ldo = 192;
        same("slice with residuals into a wider map", conv_slice_args(cv, sl[1], 64), e);
    }
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("packed_layers: ok\n");
    return 0;
}
