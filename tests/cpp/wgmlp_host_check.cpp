// Stand-alone check of nunif_amd/csrc/wgmlp_host.h (built with the host address and undefined-behaviour sanitizers by
// tests/test_wgmlp_host.py): window counts against brute force, every real token in exactly one window, the launch size, the LDS map,
// workspace regions aligned and disjoint and large enough, and the packed-weight index against packed_layers.h by the inverse layout.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../nunif_amd/csrc/packed_layers.h"
#include "../../nunif_amd/csrc/wgmlp_host.h"

namespace nunif {
void set_error(const char *, ...) {}
}  // namespace nunif

using namespace nunif;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int check_windows() {
    for (int shift = 0; shift < 2; ++shift)
        for (int B = 1; B <= 3; ++B)
            for (int H = 8; H <= 48; H += 8)
                for (int W = 8; W <= 56; W += 8) {
                    CHECK(wgmlp_map_supported(H, W));
                    const int nwy = wgmlp_windows_along(H, shift), nwx = wgmlp_windows_along(W, shift);
                    // brute force: every window that holds at least one real token, and every real token exactly once
                    std::vector<int> hits((size_t)H * W, 0);
                    long windows = 0;
                    for (int wy = -2; wy < nwy + 2; ++wy)
                        for (int wx = -2; wx < nwx + 2; ++wx) {
                            int real = 0;
                            for (int t = 0; t < kWgTokens; ++t) {
                                const int y = wgmlp_token_coord(wy, t >> 3, shift), x = wgmlp_token_coord(wx, t & 7, shift);
                                if (y >= 0 && y < H && x >= 0 && x < W) { ++real; ++hits[(size_t)y * W + x]; }
                            }
                            if (real) {
                                CHECK(wy >= 0 && wy < nwy && wx >= 0 && wx < nwx);
                                ++windows;
                            }
                        }
                    for (int h : hits) CHECK(h == 1);
                    CHECK(wgmlp_window_count(B, H, W, shift) == (long)B * windows);
                    CHECK(windows == (long)nwy * nwx);
                }
    CHECK(wgmlp_window_count(1, 8, 8, 0) == 1 && wgmlp_window_count(1, 8, 8, 1) == 4);
    CHECK(!wgmlp_map_supported(12, 8) && !wgmlp_map_supported(8, 0) && !wgmlp_channels_supported(96) && wgmlp_channels_supported(256));
    for (int C : {128, 256}) {
        CHECK(wgmlp_grid(1, C) == 1 && wgmlp_grid(wgmlp_max_groups(C), C) == (unsigned)wgmlp_max_groups(C));
        CHECK(wgmlp_grid(100000, C) == (unsigned)wgmlp_max_groups(C));
        // the LDS map: both tiles of region A fit it, rows are 16-byte aligned, and the whole is inside the part's 160 KiB
        CHECK(wgmlp_lds_a_halfs(C) >= kWgTokens * (C + kWgLdsPad) && wgmlp_lds_a_halfs(C) >= C * (kWgTokens + kWgLdsPad));
        CHECK((C + kWgLdsPad) % 8 == 0 && (kWgTokens + kWgLdsPad) % 8 == 0 && wgmlp_lds_h_stride(C) % 8 == 0 && wgmlp_lds_a_halfs(C) % 8 == 0);
        CHECK(wgmlp_lds_bytes(C) <= 160 * 1024);
        CHECK(wgmlp_lds_bytes(C) * (C == 128 ? 2 : 1) <= 160 * 1024);
    }
    CHECK(wgmlp_lds_bytes(128) == 52224 && wgmlp_lds_bytes(256) == 103424);
    return 0;
}

static int check_workspace() {
    for (int T = 8; T <= 1024; ++T) {
        const bool ok = T > 16 && (T - 16) % 48 == 0;
        CHECK(wgmlp_tile_supported(T) == ok);
    }
    for (int B : {1, 3, 16})
        for (int T : {64, 112, 256}) {
            const WgWorkspace w = wgmlp_workspace(B, T, 128);
            const size_t S = T - 16, m1 = (size_t)B * S * S;
            for (int i = 0; i < WG_REGIONS; ++i) {
                CHECK(w.off[i] % 256 == 0 && w.bytes[i] > 0 && w.off[i] + w.bytes[i] <= w.total);
                for (int j = 0; j < i; ++j) CHECK(w.off[j] + w.bytes[j] <= w.off[i]);
            }
            CHECK(w.bytes[WG_CAT] == (size_t)B * T * T * 32 * 4 && w.bytes[WG_X1] == (size_t)B * (T + 12) * (T + 12) * 16 * 4);
            CHECK(w.bytes[WG_L1A] == m1 * 128 * 2 && w.bytes[WG_L1B] == w.bytes[WG_L1A] && w.bytes[WG_L1C] == w.bytes[WG_L1A]);
            CHECK(w.bytes[WG_L2A] == m1 / 4 * 256 * 2 && w.bytes[WG_L2B] == w.bytes[WG_L2A]);
            // tmp_a / tmp_b also serve the level-2 blocks: [S/2, S/2, 256] and [S/2, S/2, 512]
            CHECK(w.bytes[WG_TMPA] >= m1 / 4 * 256 * 2 && w.bytes[WG_TMPB] >= m1 / 4 * 512 * 2 && w.bytes[WG_TMPB] == m1 * 256 * 2);
            CHECK(w.bytes[WG_RIMG] == (size_t)B * 3 * (4 * S) * (4 * S) * 4 && w.bytes[WG_IR] == (size_t)B * T * T * 32 * 2);
        }
    return 0;
}

static int check_packing() {
    // every weight of a packed Linear sits where wgmlp_packed_index says, and the index is a bijection onto the fragment array
    const int shapes[4][2] = {{256, 128}, {128, 128}, {64, 64}, {512, 256}};
    for (auto &s : shapes) {
        const int N = s[0], K = s[1];
        auto wt = [&](int n, int k) { return (float)((n * 131 + k * 7) % 2039) - 1000.f; };     // values that round differently in fp16: compared after the same rounding
        const LinearHost L = pack_linear(N, 16, K, K, false, wt, [](int) { return 0.f; });
        CHECK(L.N == N && L.K == K && L.w.size() == (size_t)N * K + kRingPadHalfs);
        std::set<size_t> seen;
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k) {
                const size_t at = wgmlp_packed_index(n, k, K);
                CHECK(at < (size_t)N * K && seen.insert(at).second);
                CHECK((float)L.w[at] == (float)(f16)wt(n, k));
            }
        CHECK(seen.size() == (size_t)N * K);
    }
    return 0;
}

int main() {
    if (check_windows() || check_workspace() || check_packing()) return 1;
    std::printf("wgmlp_host: ok\n");
    return 0;
}
