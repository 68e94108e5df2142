// CPU check of nunif_amd/csrc/host_weights.h (tests/test_host_weights.py builds this with the host sanitizers and runs it).
//
// The packers are not restated here.  The layout is checked by its INVERSE: for every element (n, k) of a matrix the place
// where the kernels will look for it is computed, and the half found there is compared; every half not reached that way, the
// ring padding included, must be zero.  Test values are the fp16 numbers with bit pattern 0x3C00 + index: distinct, exact in
// float, never zero.  No HIP call is made.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>

#include "../../nunif_amd/csrc/host_weights.h"

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

static float value(int index) {               // the fp16 with bits 0x3C00 + index, as a float
    const uint16_t bits = (uint16_t)(0x3C00 + index);
    f16 h;
    memcpy(&h, &bits, 2);
    return (float)h;
}
static uint16_t bits_of(f16 h) { uint16_t b; memcpy(&b, &h, 2); return b; }

enum Order { NT_KS, KS_NT };

// where element (n, k) of an [N][K] matrix must be
static size_t place(Order order, bool chained, int N, int K, int n, int k) {
    const int NT = N / 16, KS = K / 32, nt = n / 16, ks = k / 32;
    const size_t frag = order == NT_KS ? (size_t)nt * KS + ks : (size_t)ks * NT + nt;
    if (!chained) return ((frag * 64 + ((k % 32) / 8) * 16 + n % 16) * 8 + k % 8);
    const int g = (k % 16) / 4, j = k % 4 + 4 * ((k % 32) / 16);
    return ((frag * 64 + g * 16 + n % 16) * 8 + j);
}

// expect(n, k): the index whose value must sit at (n, k), or -1 for zero
static void check_matrix(const char *what, const std::vector<f16> &packed, Order order, bool chained, int N, int K, size_t pad,
                         const std::function<int(int, int)> &expect) {
    CHECK(packed.size() == (size_t)N * K + pad, "%s: %zu halfs, expected %zu", what, packed.size(), (size_t)N * K + pad);
    if (packed.size() != (size_t)N * K + pad) return;
    std::vector<char> seen(packed.size(), 0);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            const size_t at = place(order, chained, N, K, n, k);
            CHECK(at < (size_t)N * K && !seen[at], "%s: (%d, %d) maps to %zu (outside or twice)", what, n, k, at);
            if (at >= (size_t)N * K) continue;
            seen[at] = 1;
            const int e = expect(n, k);
            const uint16_t want = e < 0 ? 0 : (uint16_t)(0x3C00 + e);
            CHECK(bits_of(packed[at]) == want, "%s: (%d, %d) at %zu holds 0x%04x, expected 0x%04x", what, n, k, at,
                  bits_of(packed[at]), want);
        }
    for (size_t i = 0; i < packed.size(); ++i)
        if (!seen[i]) CHECK(bits_of(packed[i]) == 0, "%s: half %zu (not an element's place) is 0x%04x", what, i, bits_of(packed[i]));
}

int main() {
    // rows beyond n_real are zero and the functor is never asked for them
    {
        const int n_real = 27, N = 32, K = 64;
        int outside = 0;
        auto p = pack_nt_ks(n_real, N, K, [&](int n, int k) { if (n >= n_real || k >= K) ++outside; return value(n * K + k); });
        CHECK(outside == 0, "functor called %d times outside n_real", outside);
        check_matrix("n_real 27", p, NT_KS, false, N, K, kRingPadHalfs, [&](int n, int k) { return n < n_real ? n * K + k : -1; });
    }
    // NT = 3 != KS = 2 tells the two fragment orders apart
    {
        const int N = 48, K = 64;
        auto wt = [&](int n, int k) { return value(n * K + k); };
        auto id = [&](int n, int k) { return n * K + k; };
        check_matrix("48x64 nt_ks", pack_nt_ks(N, N, K, wt), NT_KS, false, N, K, kRingPadHalfs, id);
        check_matrix("48x64 ks_nt", pack_ks_nt(N, N, K, wt), KS_NT, false, N, K, kRingPadHalfs, id);
        check_matrix("48x64 nt_ks no pad", pack_nt_ks(N, N, K, wt, false, 0), NT_KS, false, N, K, 0, id);
    }
    // one fragment, plain and chained; two k-steps and two tiles chained
    {
        auto one = [&](int N, int K, bool chained, const char *what) {
            auto wt = [&](int n, int k) { return value(n * K + k); };
            auto id = [&](int n, int k) { return n * K + k; };
            check_matrix(what, pack_nt_ks(N, N, K, wt, chained), NT_KS, chained, N, K, kRingPadHalfs, id);
        };
        one(16, 32, false, "16x32 plain");
        one(16, 32, true, "16x32 chained");
        one(32, 64, true, "32x64 chained");
        // put_frag on its own, into a fragment that is not the first
        std::vector<f16> two(2 * kFragHalfs, (f16)0.0f);
        put_frag(two, 1, 0, 0, true, [&](int n, int k) { return value(n * 32 + k); });
        std::vector<f16> second(two.begin() + kFragHalfs, two.end());
        check_matrix("put_frag second fragment", second, NT_KS, true, 16, 32, 0, [&](int n, int k) { return n * 32 + k; });
        for (size_t i = 0; i < kFragHalfs; ++i) CHECK(bits_of(two[i]) == 0, "put_frag touched fragment 0 at %zu", i);
    }
    // 3x3 conv, 3 real input channels padded to 32: k = tap * cin + ci
    {
        const int cout = 16, cin_real = 3, cin = 32, K = 9 * cin;
        auto p = pack_ks_nt(cout, cout, K, [&](int n, int k) {
            const int tap = k / cin, ci = k % cin;
            return ci < cin_real ? value((n * cin_real + ci) * 9 + tap) : 0.0f;
        });
        check_matrix("conv3 cin 3 -> 32", p, KS_NT, false, cout, K, kRingPadHalfs, [&](int n, int k) {
            const int tap = k / cin, ci = k % cin;
            return ci < cin_real ? (n * cin_real + ci) * 9 + tap : -1;
        });
    }
    // output-channel slices of a [ks][nt] stream
    {
        auto slices = [&](int NT, int first, const char *what) {
            const int N = NT * 16, K = 64, KS = K / 32;
            auto stream = pack_ks_nt(N, N, K, [&](int n, int k) { return value(n * K + k); });
            int nt0 = 0;
            for (int nts : {first, NT - first}) {
                auto part = stream_slice(stream, KS, NT, nt0, nts);
                check_matrix(what, part, KS_NT, false, nts * 16, K, kRingPadHalfs, [&](int n, int k) { return (nt0 * 16 + n) * K + k; });
                nt0 += nts;
            }
        };
        slices(6, 4, "slices 4 + 2 of 6");
        slices(12, 8, "slices 8 + 4 of 12");
    }
    // [ks][nt] -> [nt][ks] against the direct packing of the same matrix
    {
        const int N = 48, K = 64;
        auto wt = [&](int n, int k) { return value(n * K + k); };
        auto direct = pack_nt_ks(N, N, K, wt);
        auto turned = ks_nt_to_nt_ks(pack_ks_nt(N, N, K, wt), K / 32, N / 16);
        CHECK(direct.size() == turned.size() && !memcmp(direct.data(), turned.data(), direct.size() * sizeof(f16)),
              "ks_nt_to_nt_ks differs from pack_nt_ks");
        check_matrix("ks_nt_to_nt_ks", turned, NT_KS, false, N, K, kRingPadHalfs, [&](int n, int k) { return n * K + k; });
    }
    // the descriptor map
    {
        const float a[24] = {0}, b[5] = {0};
        nunif_tensor_desc d[2];
        memset(d, 0, sizeof(d));
        d[0].name = "conv.weight"; d[0].data = a; d[0].ndim = 4; d[0].shape[0] = 2; d[0].shape[1] = 3; d[0].shape[2] = 2; d[0].shape[3] = 2;
        d[1].name = "conv.bias"; d[1].data = b; d[1].ndim = 1; d[1].shape[0] = 5;
        const TensorMap m = tensor_map(d, 2);
        const HostTensor *t = nullptr;
        CHECK(m.size() == 2, "tensor_map: %zu entries", m.size());
        CHECK(find(m, "conv.weight", &t) == NUNIF_HIP_OK && t && t->data == a && t->numel == 24 && t->shape.size() == 4 &&
              t->shape[0] == 2 && t->shape[1] == 3 && t->shape[2] == 2 && t->shape[3] == 2, "tensor_map: conv.weight");
        CHECK(find(m, "conv.bias", &t) == NUNIF_HIP_OK && t->data == b && t->numel == 5 && t->shape.size() == 1 && t->shape[0] == 5,
              "tensor_map: conv.bias");
        g_error.clear();
        CHECK(find(m, "conv.gamma", &t) == NUNIF_HIP_EMISSING, "find: missing key");
        CHECK(g_error.find("conv.gamma") != std::string::npos, "find: error text '%s'", g_error.c_str());
    }
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("host_weights: ok\n");
    return 0;
}
