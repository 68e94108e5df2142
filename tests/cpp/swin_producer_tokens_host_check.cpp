// Stand-alone check of nunif_amd/csrc/swin_producer_tokens_host.h under the host sanitizers (tests/test_swin_producer_tokens_host.py):
// every producer's table for sides 48 .. 240, every window count per axis, with and without whole-tile stages, into exactly sized heap
// buffers; every entry must name a token (patch) of the map, ascending, and a table one entry short must be refused.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../nunif_amd/csrc/swin_producer_tokens_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const int32_t kStages[5] = {2, 2, 6, 2, 2};

static void run(const std::vector<nunif_swin_block_extent> &ext, int n_tiles, int S, const int32_t *listed, int f1_whole) {
    int32_t shifts[14];
    for (int st = 0, k = 0; st < 5; ++st)
        for (int i = 0; i < kStages[st]; ++i) shifts[k++] = i % 2 ? 3 : 0;
    for (int pr = NUNIF_SWIN_PRODUCER_STEM; pr <= NUNIF_SWIN_PRODUCER_UP1; ++pr) {
        const int side = pr == NUNIF_SWIN_PRODUCER_DOWN2 || pr == NUNIF_SWIN_PRODUCER_UP2 ? S / 4 : S / 2;
        const int64_t limit = pr == NUNIF_SWIN_PRODUCER_STEM ? (int64_t)n_tiles * ((S + 23) / 24) * ((S + 15) / 16) : (int64_t)n_tiles * side * side;
        int64_t n = -1, n2 = -1;
        CHECK(nunif::swin_producer_tokens_host(ext.data(), n_tiles, kStages, shifts, listed, S, f1_whole, pr, 24, 16, nullptr, 0, &n) == nullptr);
        CHECK(n > 0 && n <= limit);
        const int64_t cap = pr == NUNIF_SWIN_PRODUCER_STEM ? n : (n + 31) / 32 * 32;
        uint32_t *tab = (uint32_t *)std::malloc(sizeof(uint32_t) * (size_t)cap);
        CHECK(nunif::swin_producer_tokens_host(ext.data(), n_tiles, kStages, shifts, listed, S, f1_whole, pr, 24, 16, tab, cap, &n2) == nullptr);
        CHECK(n2 == n);
        for (int64_t i = 0; i < cap; ++i) {
            CHECK((int64_t)tab[i] < limit);
            if (i > 0 && i < n) CHECK(tab[i] > tab[i - 1]);
            if (i >= n) CHECK(tab[i] == tab[n - 1]);
        }
        CHECK(nunif::swin_producer_tokens_host(ext.data(), n_tiles, kStages, shifts, listed, S, f1_whole, pr, 24, 16, tab, cap - 1, &n2) != nullptr);
        std::free(tab);
    }
}

int main() {
    const int32_t all[14] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, some[14] = {1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0};
    for (int S : {48, 96, 144, 240}) {
        const int sides[5] = {S, S / 2, S / 4, S / 2, S};
        const int step = S >= 144 ? 7 : 1;
        for (int m1 = 1; m1 <= S / 6; m1 += step)
            for (int wrap = 0; wrap < 2; ++wrap) {
                // two tiles: the same count on both axes / different ones; deeper stages scaled down, never above their side
                std::vector<nunif_swin_block_extent> ext(2 * 14);
                for (int t = 0; t < 2; ++t)
                    for (int st = 0, k = 0; st < 5; ++st)
                        for (int i = 0; i < kStages[st]; ++i, ++k) {
                            const int nw = sides[st] / 6, shifted = i % 2 && nw > 1;
                            const int ny = (m1 * nw + S / 6 - 1) / (S / 6), nx = t ? nw : ny;
                            nunif_swin_block_extent &e = ext[(size_t)t * 14 + k];
                            e.n_win[0] = shifted && wrap ? (ny < nw - 1 ? ny : nw - 1) : ny;
                            e.n_win[1] = shifted && wrap ? (nx < nw - 1 ? nx : nw - 1) : nx;
                            e.wrap[0] = e.wrap[1] = shifted && wrap;
                        }
                run(ext, 2, S, all, 0);
                run(ext, 2, S, some, 0);
                run(ext, 1, S, nullptr, 1);
            }
    }
    int64_t n = 0;
    std::vector<nunif_swin_block_extent> e(14, nunif_swin_block_extent{{1, 1}, {0, 0}});
    const int32_t shifts[14] = {0, 3, 0, 3, 0, 3, 0, 3, 0, 3, 0, 3, 0, 3};
    CHECK(nunif::swin_producer_tokens_host(e.data(), 1, kStages, shifts, nullptr, 50, 0, 1, 24, 16, nullptr, 0, &n) != nullptr);
    CHECK(nunif::swin_producer_tokens_host(e.data(), 1, kStages, shifts, nullptr, 48, 0, 7, 24, 16, nullptr, 0, &n) != nullptr);
    CHECK(nunif::swin_producer_tokens_host(e.data(), 1, kStages, shifts, nullptr, 48, 0, 0, 0, 16, nullptr, 0, &n) != nullptr);
    e[3].n_win[0] = 99;
    CHECK(nunif::swin_producer_tokens_host(e.data(), 1, kStages, shifts, nullptr, 48, 0, 1, 24, 16, nullptr, 0, &n) != nullptr);
    if (fails) { std::printf("swin_producer_tokens_host: %d check(s) failed\n", fails); return 1; }
    std::printf("swin_producer_tokens_host: ok\n");
    return 0;
}
