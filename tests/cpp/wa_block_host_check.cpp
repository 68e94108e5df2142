// Stand-alone check of nunif_amd/csrc/wa_block_host.h under the host sanitizers (tests/test_wa_block_host.py): the score-bias table and
// the packed arrays of a WABlock, built from a seeded state dict written here, for every shape the engines ask for — window 3 and 4
// with 64 channels (row_flow_v3, MLBW), window 4 with 128 (MLBW l4), window 8 with 32 channels in heads of 16 (DepthAA), and the
// N x N tables of windows 6 and 8 (swin_unet_v2).  Prints per case "table <case> <stride> <words as hex>" and "hash <case> <array>
// <FNV-1a 64 of its bytes>"; checks the padding rule of the stride-16 table, the sizes, and that bad shapes are refused.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <list>
#include <string>
#include <vector>

#include "../../nunif_amd/csrc/wa_block_host.h"

using namespace nunif;

static char last_error[512];
void nunif::set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// xorshift64*: the top 24 bits as a float in [-scale, scale)
struct Rng {
    uint64_t s;
    float next(float scale) {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        const uint64_t r = s * 0x2545F4914F6CDD1Dull;
        return ((float)(r >> 40) / 8388608.0f - 1.0f) * scale;
    }
};

struct State {
    std::list<std::vector<float>> store;      // a list: the tensors' addresses must not move
    TensorMap m;
    void add(const std::string &key, std::vector<int64_t> shape, float scale, Rng &rng) {
        int64_t n = 1;
        for (int64_t d : shape) n *= d;
        store.emplace_back((size_t)n);
        for (float &v : store.back()) v = rng.next(scale);
        m[key] = HostTensor{store.back().data(), shape, n};
    }
};

static void add_to_bias(State &st, const std::string &p, int window, Rng &rng) {
    const int hidden = 2 * window;            // WindowScoreBias: int(sqrt(window^2)) * 2
    st.add(p + "to_bias.0.weight", {hidden, 2}, 1.5f, rng);
    st.add(p + "to_bias.0.bias", {hidden}, 0.5f, rng);
    st.add(p + "to_bias.2.weight", {1, hidden}, 1.0f, rng);
    st.add(p + "to_bias.2.bias", {1}, 0.5f, rng);
}

static State block_state(const std::string &p, int window, int C, uint64_t seed) {
    State st;
    Rng rng{seed};
    st.add(p + "mha.mha.qkv_proj.weight", {3 * C, C}, 0.25f, rng);
    st.add(p + "mha.mha.qkv_proj.bias", {3 * C}, 0.5f, rng);
    st.add(p + "mha.mha.head_proj.weight", {C, C}, 0.25f, rng);
    st.add(p + "mha.mha.head_proj.bias", {C}, 0.5f, rng);
    st.add(p + "conv_mlp.0.weight", {C, C, 1, 1}, 0.25f, rng);
    st.add(p + "conv_mlp.0.bias", {C}, 0.5f, rng);
    st.add(p + "conv_mlp.3.weight", {C, C, 3, 3}, 0.1f, rng);
    st.add(p + "conv_mlp.3.bias", {C}, 0.5f, rng);
    add_to_bias(st, p + "bias.", window, rng);
    return st;
}

static uint64_t fnv1a(const void *data, size_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const unsigned char *)data)[i]) * 0x100000001b3ull;
    return h;
}

template <typename T>
static void print_hash(const char *name, const char *array, const std::vector<T> &v) {
    std::printf("hash %s %s %016llx\n", name, array, (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)));
}

static void print_table(const char *name, int stride, const std::vector<float> &tab) {
    std::printf("table %s %d ", name, stride);
    for (float v : tab) {
        uint32_t w;
        std::memcpy(&w, &v, 4);
        std::printf("%08x", w);
    }
    std::printf("\n");
}

static int table_of(const State &st, const std::string &p, int window, int stride, std::vector<float> *tab) {
    return wa_score_bias_table(&st.m.at(p + "to_bias.0.weight"), &st.m.at(p + "to_bias.0.bias"), &st.m.at(p + "to_bias.2.weight"),
                               &st.m.at(p + "to_bias.2.bias"), window, stride, p, tab);
}

static void block_case(const char *name, int window, int C, int hd, int stride, uint64_t seed) {
    const std::string p = "blocks.1.";
    const State st = block_state(p, window, C, seed);
    WaBlockHost b;
    CHECK(wa_block_pack(st.m, p, window, C, hd, stride, &b) == NUNIF_HIP_OK);
    const size_t NT = C / 16, KS = C / 32, N = (size_t)window * window;
    CHECK(b.wfrag.size() == 4 * NT * KS * kFragHalfs);
    CHECK(b.w1.size() == NT * KS * kFragHalfs + kRingPadHalfs && b.w3.size() == 9 * NT * KS * kFragHalfs + kRingPadHalfs);
    CHECK(b.bqkv.size() == (size_t)3 * C && b.bproj.size() == (size_t)C && b.b1.size() == (size_t)C && b.b3.size() == (size_t)C);
    CHECK(b.btab.size() == (size_t)stride * stride);
    // the padding rule: masked key columns in every row, zero rows for the padded queries, and the window's own entries are the ones
    // of the N x N table of the same MLP
    std::vector<float> dense;
    CHECK(table_of(st, p + "bias.", window, (int)N, &dense) == NUNIF_HIP_OK && dense.size() == N * N);
    for (size_t q = 0; q < (size_t)stride && b.btab.size() == (size_t)stride * stride && dense.size() == N * N; ++q)
        for (size_t k = 0; k < (size_t)stride; ++k) {
            const float v = b.btab[q * stride + k];
            if (k >= N) CHECK(v == -1.0e30f);
            else if (q >= N) CHECK(v == 0.f);
            else CHECK(std::memcmp(&v, &dense[q * N + k], 4) == 0 && std::isfinite(v) && std::fabs(v) < 100.f);
        }
    print_table(name, stride, b.btab);
    print_hash(name, "wfrag", b.wfrag);
    print_hash(name, "bqkv", b.bqkv);
    print_hash(name, "bproj", b.bproj);
    print_hash(name, "w1", b.w1);
    print_hash(name, "b1", b.b1);
    print_hash(name, "w3", b.w3);
    print_hash(name, "b3", b.b3);
}

static void table_case(const char *name, int window, uint64_t seed) {
    State st;
    Rng rng{seed};
    add_to_bias(st, "relative_bias.", window, rng);
    std::vector<float> tab;
    CHECK(table_of(st, "relative_bias.", window, window * window, &tab) == NUNIF_HIP_OK);
    CHECK(tab.size() == (size_t)window * window * window * window);
    for (float v : tab) CHECK(std::isfinite(v) && std::fabs(v) < 100.f);
    print_table(name, window * window, tab);
}

static void refused_shapes() {
    const std::string p = "blocks.1.";
    WaBlockHost b;
    {   // a qkv_proj of another channel count
        State st = block_state(p, 4, 64, 5);
        st.m[p + "mha.mha.qkv_proj.weight"].numel -= 64;
        last_error[0] = 0;
        CHECK(wa_block_pack(st.m, p, 4, 64, 32, 16, &b) == NUNIF_HIP_EINVAL && std::strstr(last_error, "expected 64 channels"));
        State st8 = block_state(p, 8, 64, 5);                          // DepthAA's shape asked of 64-channel weights
        CHECK(wa_block_pack(st8.m, p, 8, 32, 16, 64, &b) == NUNIF_HIP_EINVAL && std::strstr(last_error, "expected 32 channels"));
    }
    {   // to_bias: a first layer that does not take (dy, dx), a second one with two outputs
        State st = block_state(p, 4, 64, 6);
        st.m[p + "bias.to_bias.0.weight"].numel -= 1;
        last_error[0] = 0;
        CHECK(wa_block_pack(st.m, p, 4, 64, 32, 16, &b) == NUNIF_HIP_EINVAL && std::strstr(last_error, "score-bias MLP shape"));
        State st2 = block_state(p, 4, 64, 6);
        Rng rng{7};
        st2.add(p + "bias.to_bias.2.bias", {2}, 0.5f, rng);
        CHECK(wa_block_pack(st2.m, p, 4, 64, 32, 16, &b) == NUNIF_HIP_EINVAL);
    }
    {   // a missing tensor
        State st = block_state(p, 4, 64, 8);
        st.m.erase(p + "conv_mlp.3.bias");
        CHECK(wa_block_pack(st.m, p, 4, 64, 32, 16, &b) == NUNIF_HIP_EMISSING);
    }
}

int main() {
    block_case("w3c64", 3, 64, 32, 16, 11);
    block_case("w4c64", 4, 64, 32, 16, 12);
    block_case("w4c128", 4, 128, 32, 16, 13);
    block_case("w8c32", 8, 32, 16, 64, 14);
    table_case("t6", 6, 15);
    table_case("t8", 8, 16);
    refused_shapes();
    if (fails) { std::printf("wa_block_host: %d check(s) FAILED\n", fails); return 1; }
    std::printf("wa_block_host: ok\n");
    return 0;
}
