// The tokens the producers of a swin_unet frame render have to write (nunif_hip_swin_unet_producer_tokens of nunif_hip.h): host-only
// integer math, kept in a header of its own so that a stand-alone program can run it under the host sanitizers
// (tests/cpp/swin_producer_tokens_host_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/nunif_hip.h"

namespace nunif {

// Everything is separable per axis, as the extents are: per tile and axis the READ set of a stage is the union over its blocks of the
// tokens of the block's active windows (both halves of a wrap window; a block that is not `listed` runs whole tiles and reads every
// token), and a tile's token set is the product of its two axes — a superset of the union of the blocks' own products, and one run or
// two per row.  With P(A)[i] = A[2 i] | A[2 i + 1] (the parents of a 2 x 2 block) and Ch(A)[i] = A[i / 2] (its children), walking back:
//   up1 lists the level-2 tokens    UP1 = P(R5)             and rewrites their children in place (a superset of R5),
//   up2 lists the level-3 tokens    UP2 = P(R4)             and rewrites their children in place,
//   down2 (both passes) writes      N3  = R3 | UP2,
//   down1 writes                    N2  = R2 | Ch(N3) | UP1 (Ch(N3) holds Ch(UP2): the skip tokens up2 adds onto),
//   the stem writes                 N1  = R1 | Ch(N2)       (Ch(N2) holds Ch(UP1): the skip tokens up1 adds onto), every token
//                                                           if `f1_whole` (the 4x net: proj2 reads the whole level-1 map).
// Returns 0, or a message (static storage) for the caller to report.
inline const char *swin_producer_tokens_host(const nunif_swin_block_extent *ext, int32_t n_tiles, const int32_t *blocks_per_stage,
                                             const int32_t *shifts, const int32_t *listed, int32_t S, int32_t f1_whole,
                                             int32_t producer, int32_t patch_h, int32_t patch_w, uint32_t *out, int64_t cap,
                                             int64_t *n_out) {
    if (!(ext && blocks_per_stage && shifts && n_out && n_tiles > 0)) return "producer_tokens: bad argument";
    if (!(S >= 24 && S % 24 == 0 && (int64_t)n_tiles * S * S < ((int64_t)1 << 31))) return "producer_tokens: tile count or side unsupported";
    if (producer < NUNIF_SWIN_PRODUCER_STEM || producer > NUNIF_SWIN_PRODUCER_UP1) return "producer_tokens: unknown producer";
    if (producer == NUNIF_SWIN_PRODUCER_STEM && (patch_h <= 0 || patch_w <= 0)) return "producer_tokens: the stem needs its patch size";
    int first[6] = {0};
    for (int st = 0; st < 5; ++st) {
        if (blocks_per_stage[st] < 1) return "producer_tokens: a stage without blocks";
        first[st + 1] = first[st] + blocks_per_stage[st];
    }
    const int n_blocks = first[5];
    const int size[5] = {S, S / 2, S / 4, S / 2, S};
    for (int i = 0; i < n_blocks; ++i)
        if (shifts[i] != 0 && shifts[i] != 3) return "producer_tokens: shift unsupported";
    typedef std::vector<char> Set;
    auto parents = [](const Set &a) { Set p(a.size() / 2); for (size_t i = 0; i < p.size(); ++i) p[i] = a[2 * i] | a[2 * i + 1]; return p; };
    auto children = [](const Set &a) { Set c(a.size() * 2); for (size_t i = 0; i < c.size(); ++i) c[i] = a[i / 2]; return c; };
    auto join = [](Set &a, const Set &b) { for (size_t i = 0; i < a.size(); ++i) a[i] |= b[i]; };
    int64_t n = 0;
    auto put = [&](uint32_t v) -> bool {
        if (out) {
            if (n >= cap) return false;
            out[n] = v;
        }
        ++n;
        return true;
    };
    Set want[2];
    std::vector<int> ys, runs;         // wanted rows; wanted columns as [x0, x1) pairs
    for (int b = 0; b < n_tiles; ++b) {
        // (consecutive tiles of a grid mostly have the same extents: the sets of the tile before are reused)
        bool same = b > 0;
        for (int i = 0; same && i < n_blocks; ++i) {
            const nunif_swin_block_extent &p = ext[(size_t)(b - 1) * n_blocks + i], &q = ext[(size_t)b * n_blocks + i];
            same = p.n_win[0] == q.n_win[0] && p.n_win[1] == q.n_win[1] && p.wrap[0] == q.wrap[0] && p.wrap[1] == q.wrap[1];
        }
        for (int ax = 0; ax < 2 && !same; ++ax) {
            Set R[5];
            for (int st = 0; st < 5; ++st) {
                const int Ss = size[st], nw = Ss / 6;
                R[st].assign(Ss, 0);
                for (int i = first[st]; i < first[st + 1]; ++i) {
                    if (listed && !listed[i]) { R[st].assign(Ss, 1); break; }
                    const nunif_swin_block_extent &e = ext[(size_t)b * n_blocks + i];
                    if (e.n_win[ax] < 0 || e.n_win[ax] > nw) return "producer_tokens: more windows than the side holds";
                    const int shift = Ss <= 6 ? 0 : shifts[i];
                    for (int w = 0; w < nw; ++w) {
                        if (!(w < e.n_win[ax] || (e.wrap[ax] && w == nw - 1))) continue;
                        for (int t = 0; t < 6; ++t) R[st][(6 * w + shift + t) % Ss] = 1;
                    }
                }
            }
            const Set up1 = parents(R[4]), up2 = parents(R[3]);
            Set n3 = R[2];
            join(n3, up2);
            Set n2 = R[1];
            join(n2, children(n3));
            join(n2, up1);
            Set n1 = R[0];
            join(n1, children(n2));
            if (f1_whole) n1.assign(S, 1);
            switch (producer) {
                case NUNIF_SWIN_PRODUCER_STEM: want[ax] = n1; break;
                case NUNIF_SWIN_PRODUCER_DOWN1: want[ax] = n2; break;
                case NUNIF_SWIN_PRODUCER_DOWN2: want[ax] = n3; break;
                case NUNIF_SWIN_PRODUCER_UP2: want[ax] = up2; break;
                default: want[ax] = up1; break;
            }
        }
        if (producer == NUNIF_SWIN_PRODUCER_STEM) {
            // spatial output patches of patch_h x patch_w tokens, in the kernel's own order: a patch with one wanted token runs whole
            const int nty = (S + patch_h - 1) / patch_h, ntx = (S + patch_w - 1) / patch_w;
            Set py(nty, 0), px(ntx, 0);
            for (int y = 0; y < S; ++y) py[y / patch_h] |= want[0][y];
            for (int x = 0; x < S; ++x) px[x / patch_w] |= want[1][x];
            for (int ty = 0; ty < nty; ++ty)
                for (int tx = 0; tx < ntx; ++tx)
                    if (py[ty] && px[tx] && !put((uint32_t)((b * nty + ty) * ntx + tx))) return "producer_tokens: the table is too small";
            continue;
        }
        const int Ss = (int)want[0].size();
        if (!same) {
            ys.clear(); runs.clear();
            for (int y = 0; y < Ss; ++y)
                if (want[0][y]) ys.push_back(y);
            for (int x = 0; x < Ss;) {
                if (!want[1][x]) { ++x; continue; }
                int x1 = x;
                while (x1 < Ss && want[1][x1]) ++x1;
                runs.push_back(x); runs.push_back(x1);
                x = x1;
            }
        }
        int per_row = 0;
        for (size_t k = 0; k < runs.size(); k += 2) per_row += runs[k + 1] - runs[k];
        const int64_t add = (int64_t)ys.size() * per_row;
        if (out) {
            if (n + add > cap) return "producer_tokens: the table is too small";
            uint32_t *o = out + n;
            for (int y : ys) {
                const uint32_t row = (uint32_t)((b * Ss + y) * Ss);
                for (size_t k = 0; k < runs.size(); k += 2)
                    for (int x = runs[k]; x < runs[k + 1]; ++x) *o++ = row + (uint32_t)x;
            }
        }
        n += add;
    }
    *n_out = n;
    // a token launch walks whole groups of 32: the last one is filled up with its last token (such a lane computes and stores what
    // that token's own lane does)
    if (producer != NUNIF_SWIN_PRODUCER_STEM && out && n > 0) {
        const uint32_t last = out[n - 1];
        for (int64_t i = n; i < (n + 31) / 32 * 32; ++i) {
            if (i >= cap) return "producer_tokens: the table is too small";
            out[i] = last;
        }
    }
    return nullptr;
}

}  // namespace nunif
