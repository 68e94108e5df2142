// Stand-alone check of nunif_amd/csrc/swin_tail_groups_host.h under the host sanitizers (tests/test_swin_tail_groups_host.py): every
// table is built into an exactly sized heap buffer (a write past the count it announced is a heap overflow), decoded again and
// compared with the token set enumerated window by window.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../nunif_amd/csrc/swin_tail_groups_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void run(const std::vector<nunif_swin_block_extent> &ext, int S, int shift) {
    const int nw = S / 6, n_tiles = (int)ext.size(), sh = S <= 6 ? 0 : shift;
    std::vector<long> want;
    for (int b = 0; b < n_tiles; ++b) {
        std::set<long> tile;
        for (int wy = 0; wy < nw; ++wy)
            for (int wx = 0; wx < nw; ++wx) {
                const bool ay = wy < ext[b].n_win[0] || (ext[b].wrap[0] && wy == nw - 1), ax = wx < ext[b].n_win[1] || (ext[b].wrap[1] && wx == nw - 1);
                if (!ay || !ax) continue;
                for (int t = 0; t < 36; ++t) tile.insert(((long)b * S + (6 * wy + sh + t / 6) % S) * S + (6 * wx + sh + t % 6) % S);
            }
        want.insert(want.end(), tile.begin(), tile.end());
    }
    int64_t ng = -1, nt = -1;
    CHECK(nunif::swin_tail_groups_host(ext.data(), n_tiles, S, shift, nullptr, 0, &ng, &nt) == nullptr);
    CHECK(nt == (int64_t)want.size() && ng == (nt + 15) / 16);
    nunif_swin_tail_group *tab = (nunif_swin_tail_group *)std::malloc(sizeof(nunif_swin_tail_group) * (size_t)(ng > 0 ? ng : 1));
    int64_t ng2 = -1, nt2 = -1;
    CHECK(nunif::swin_tail_groups_host(ext.data(), n_tiles, S, shift, tab, ng, &ng2, &nt2) == nullptr);
    CHECK(ng2 == ng && nt2 == nt);
    if (ng > 1) CHECK(nunif::swin_tail_groups_host(ext.data(), n_tiles, S, shift, tab, ng - 1, &ng2, &nt2) != nullptr);   // too small: refused
    std::vector<long> got;
    for (int64_t g = 0; g < ng; ++g) {
        const unsigned bw = tab[g].bounds;
        const int cnt = (int)((bw >> 25) & 31u);
        CHECK(cnt >= 1 && cnt <= 16 && (g + 1 == ng || cnt == 16) && tab[g].reserved == 0);
        for (int r = 0; r < cnt; ++r) {
            int p = 0;
            for (int q = 1; q < 6; ++q)
                if (r >= (int)((bw >> (5 * (q - 1))) & 31u)) p = q;
            got.push_back((long)tab[g].adj[p] + r);
        }
    }
    std::free(tab);
    CHECK(got == want);                          // ascending, each token once
}

int main() {
    for (int S : {6, 12, 24, 30, 60, 120})
        for (int shift : {0, 3}) {
            const int nw = S / 6;
            for (int ny = 0; ny <= nw; ++ny)
                for (int nx = 0; nx <= nw; nx += (nw > 6 ? 3 : 1)) {
                    const int wrap = shift && S > 6 ? 1 : 0;
                    const int my = wrap ? (ny < nw ? ny : nw - 1) : ny, mx = wrap ? (nx < nw ? nx : nw - 1) : nx;
                    std::vector<nunif_swin_block_extent> ext = {{{my, mx}, {wrap, wrap}}, {{nw - wrap, mx}, {wrap, wrap}}, {{0, 0}, {0, 0}},
                                                                {{my, nw - wrap}, {wrap, wrap}}};
                    run(ext, S, shift);
                    run({ext[0]}, S, shift);
                }
        }
    int64_t a, b;
    nunif_swin_block_extent e = {{1, 1}, {0, 0}};
    CHECK(nunif::swin_tail_groups_host(&e, 1, 7, 0, nullptr, 0, &a, &b) != nullptr);
    CHECK(nunif::swin_tail_groups_host(&e, 1, 12, 2, nullptr, 0, &a, &b) != nullptr);
    e.n_win[0] = 3;
    CHECK(nunif::swin_tail_groups_host(&e, 1, 12, 0, nullptr, 0, &a, &b) != nullptr);
    if (fails) { std::printf("swin_tail_groups_host: %d check(s) failed\n", fails); return 1; }
    std::printf("swin_tail_groups_host: ok\n");
    return 0;
}
