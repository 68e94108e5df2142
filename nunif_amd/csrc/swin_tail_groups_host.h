// The token groups of the C = 192 tail of a frame render (nunif_hip_swin_unet_tail_groups of nunif_hip.h): host-only integer math, kept
// in a header of its own so that a stand-alone program can run it under the host sanitizers (tests/cpp/swin_tail_groups_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/nunif_hip.h"

namespace nunif {

// In [tile][y][x] order the tokens of a tile's active windows are one run per
// active row — of a shifted block, columns [S - 3, S) of row y run on into [0, ..) of row y + 1, and the last row of a tile into the
// first of the next — so the runs are merged as they are met and cut into groups of 16 slots; a group holds up to 6 pieces.
// Returns 0, or a message (static storage) for the caller to report.
inline const char *swin_tail_groups_host(const nunif_swin_block_extent *ext, int32_t n_tiles, int32_t S, int32_t shift,
                                         nunif_swin_tail_group *out, int64_t cap, int64_t *n_groups, int64_t *n_tokens) {
    if (!(ext && n_groups && n_tokens && n_tiles > 0)) return "tail_groups: bad argument";
    if (!(S >= 6 && S % 6 == 0 && (shift == 0 || shift == 3) && (int64_t)n_tiles * S * S < ((int64_t)1 << 31)))
        return "tail_groups: tile count, side or shift unsupported";
    const int nw = S / 6;
    if (S <= 6) shift = 0;
    constexpr int kPieces = 6;
    constexpr uint32_t kNoPieces = 16u | 16u << 5 | 16u << 10 | 16u << 15 | 16u << 20;     // pieces 1 .. 5 absent
    int64_t ng = 0, nt = 0;
    nunif_swin_tail_group g;
    int cnt = 0, pieces = 0;
    int64_t run_end = -1;                  // one past the last token taken (a token that continues it opens no new piece)
    auto close = [&]() -> const char * {
        if (cnt == 0) return nullptr;
        g.bounds |= (uint32_t)cnt << 25;
        for (int p = pieces; p < kPieces; ++p) {
            g.adj[p] = 0;
            if (p >= 1) g.bounds |= 16u << (5 * (p - 1));
        }
        if (out) {
            if (ng >= cap) return "tail_groups: the table holds too few groups";
            out[ng] = g;
        }
        ++ng;
        cnt = 0; pieces = 0;
        return nullptr;
    };
    auto take = [&](int64_t first, int n) -> const char * {         // tokens [first, first + n)
        const char *rc;
        while (n > 0) {
            const bool joins = cnt > 0 && first == run_end;
            if (cnt == 16 || (cnt > 0 && !joins && pieces == kPieces))
                if ((rc = close())) return rc;
            if (cnt == 0) { g = nunif_swin_tail_group(); }
            if (cnt == 0 || first != run_end) {
                g.adj[pieces] = (int32_t)(first - cnt);
                if (pieces >= 1) g.bounds |= (uint32_t)cnt << (5 * (pieces - 1));
                ++pieces;
            }
            const int k = std::min(n, 16 - cnt);
            cnt += k; nt += k; first += k; n -= k;
            run_end = first;
            // the inside of a long run: whole groups of one piece, written directly
            if (cnt == 16 && n >= 16) {
                if ((rc = close())) return rc;
                const int64_t whole = n / 16;
                if (out && ng + whole > cap) return "tail_groups: the table holds too few groups";
                if (out)
                    for (int64_t j = 0; j < whole; ++j) {
                        nunif_swin_tail_group &o = out[ng + j];
                        o = nunif_swin_tail_group();
                        o.adj[0] = (int32_t)(first + 16 * j);
                        o.bounds = kNoPieces | 16u << 25;
                    }
                ng += whole; nt += 16 * whole; first += 16 * whole; n -= (int)(16 * whole);
                run_end = first;
            }
        }
        return nullptr;
    };
    std::vector<char> on[2];
    for (int b = 0; b < n_tiles; ++b) {
        for (int ax = 0; ax < 2; ++ax) {
            if (ext[b].n_win[ax] < 0 || ext[b].n_win[ax] > nw) return "tail_groups: more windows than the side holds";
            on[ax].assign(S, 0);
            for (int w = 0; w < nw; ++w) {
                if (!(w < ext[b].n_win[ax] || (ext[b].wrap[ax] && w == nw - 1))) continue;
                for (int t = 0; t < 6; ++t) on[ax][(6 * w + shift + t) % S] = 1;
            }
        }
        int runs[2][2], n_runs = 0;          // the active columns: a prefix of windows and / or the wrap window's [S - 3, S)
        for (int x0 = 0; x0 < S;) {
            if (!on[1][x0]) { ++x0; continue; }
            int x1 = x0;
            while (x1 < S && on[1][x1]) ++x1;
            if (n_runs == 2) return "tail_groups: internal: more than two column runs";
            runs[n_runs][0] = x0; runs[n_runs][1] = x1; ++n_runs;
            x0 = x1;
        }
        const bool whole_rows = n_runs == 1 && runs[0][0] == 0 && runs[0][1] == S;
        for (int y = 0; y < S; ++y) {
            if (!on[0][y]) continue;
            const char *rc;
            if (whole_rows) {                 // consecutive whole rows are one run
                int y1 = y;
                while (y1 < S && on[0][y1]) ++y1;
                if ((rc = take(((int64_t)b * S + y) * S, (y1 - y) * S))) return rc;
                y = y1 - 1;
                continue;
            }
            for (int k = 0; k < n_runs; ++k)
                if ((rc = take(((int64_t)b * S + y) * S + runs[k][0], runs[k][1] - runs[k][0]))) return rc;
        }
    }
    if (const char *rc = close()) return rc;
    *n_groups = ng; *n_tokens = nt;
    return nullptr;
}

}  // namespace nunif
