// The workspace layout of stlizer pass 3 (nunif_amd/csrc/stlizer_pass3_host.h) walked on the host: every region is 256-byte
// aligned, the regions are disjoint and in order, each is as large as the kernels reach (the last element of every vector of the
// history ring, the last partial of the last launch, the last field of the last record), and their end is workspace_bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../nunif_amd/csrc/stlizer_pass3_host.h"

using namespace nunif::pass3;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d %s (N=%lld)\n", __FILE__, __LINE__, #cond, (long long)N); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int check(int64_t N, int64_t iteration) {
    const Layout l = layout(N, iteration);
    CHECK(l.M == N + 3 && l.Mp >= l.M && l.Mp % kTile == 0 && l.Mp - l.M < kTile && l.nparts == 3 * l.tiles);
    struct Region { const char *name; int64_t begin, reach; };
    const int64_t slots = iteration * kMaxIter;
    const std::vector<Region> regions = {
        {"rec", l.rec, l.rec + ((slots - 1) * kRecDoubles + R_END) * 8},
        {"ro", l.ro, l.ro + kRing * 8},
        {"x", l.x, l.x + (3 * 3 * l.Mp + 2 * l.Mp + l.M) * 8},
        {"t", l.t, l.t + (2 * l.Mp + l.M) * 8},
        {"w", l.w, l.w + l.M * 8},
        {"g", l.g, l.g + (2 * l.Mp + l.M) * 8},
        {"q", l.q, l.q + (2 * l.Mp + l.M) * 8},
        {"S", l.S, l.S + ((int64_t)(kRing - 1) * 3 * l.Mp + 2 * l.Mp + l.M) * 8},
        {"Y", l.Y, l.Y + ((int64_t)(kRing - 1) * 3 * l.Mp + 2 * l.Mp + l.M) * 8},
        {"partials", l.partials, partial_offset(l, kLaunchesPerSlot - 1, kQuantities - 1, l.nparts - 1) + 8},
    };
    for (size_t r = 0; r < regions.size(); ++r) {
        const int64_t end = r + 1 < regions.size() ? regions[r + 1].begin : l.total;
        CHECK(regions[r].begin % 256 == 0);
        CHECK(regions[r].begin < regions[r].reach && regions[r].reach <= end);
    }
    CHECK(regions[0].begin == 0 && l.total % 256 == 0);
    // the prefix sums borrow the first partial buffer for 3 * ceil(N / 256) tile sums
    CHECK(3 * ((N + kTile - 1) / kTile) <= l.nparts);
    // touch every record field and every ring slot index through a host copy of the small regions
    std::vector<double> rec((size_t)(slots * kRecDoubles), 0.0);
    for (int64_t j = 0; j < slots; ++j)
        for (int f = 0; f < R_END; ++f) rec[(size_t)(j * kRecDoubles + f)] = 1.0;
    std::vector<int> seen(kRing, 0);
    for (int head = 0; head < kRing; ++head)
        for (int i = 0; i < kHistory; ++i) {
            const int s = ring_slot(head, i);
            CHECK(s >= 0 && s < kRing && s != (head + 1) % kRing);             // the candidate slot is never a valid pair's
            seen[(size_t)s] = 1;
        }
    for (int s : seen) CHECK(s == 1);
    return 0;
}

int main() {
    for (int64_t N : {1LL, 257LL, 1048576LL})
        for (int64_t iteration : {1LL, 100LL, 1024LL})
            if (check(N, iteration)) return 1;
    const int64_t N = 0;
    CHECK(!shape_ok(0, 1) && !shape_ok(kMaxN + 1, 1) && !shape_ok(1, 0) && !shape_ok(1, kMaxIteration + 1) && shape_ok(kMaxN, kMaxIteration));
    // the three exits after a re-evaluation, in torch's order; each threshold from both sides; a NaN passes every test
    const double nan = std::nan("");
    CHECK(exit_after_code(1.0, 1.0, 1.0) == 0);
    CHECK(exit_after_code(1e-7, 1.0, 1.0) == 3 && exit_after_code(1.0000001e-7, 1.0, 1.0) == 0);
    CHECK(exit_after_code(1.0, 1e-9, 1.0) == 4 && exit_after_code(1.0, 1.0000001e-9, 1.0) == 0);
    CHECK(exit_after_code(1.0, 1.0, 0.9999999e-9) == 5 && exit_after_code(1.0, 1.0, 1e-9) == 0);      // strict for the loss
    CHECK(exit_after_code(1e-8, 1e-10, 0.0) == 3 && exit_after_code(1.0, 1e-10, 0.0) == 4 && exit_after_code(1.0, 0.0, 0.0) == 4);
    CHECK(exit_after_code(nan, nan, nan) == 0 && exit_after_code(nan, 1e-10, 0.0) == 4 && exit_after_code(nan, nan, 0.0) == 5);
    std::printf("stlizer_pass3_host: ok\n");
    return 0;
}
