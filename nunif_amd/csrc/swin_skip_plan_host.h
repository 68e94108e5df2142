// The plan of a swin_unet frame render that skips padding-only work: the window extents of a tile
// (nunif_hip_swin_unet_tile_extents of nunif_hip.h) and everything one tile minibatch uploads — window lists, C = 192 group tables,
// producer lists — laid out in one buffer of words.  Host-only integer math, kept in a header of its own so that a stand-alone program
// can run it under the host sanitizers (tests/cpp/swin_skip_plan_host_check.cpp); swin_unet.cpp has the device half (skip_plan).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/nunif_hip.h"
#include "swin_producer_tokens_host.h"
#include "swin_tail_groups_host.h"

namespace nunif {

// a message with up to three numbers in it (%lld), in static storage like the literal ones
inline const char *swin_plan_msg(const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
    static thread_local char buf[160];
    std::snprintf(buf, sizeof(buf), fmt, a, b, c);
    return buf;
}

// One axis of one block, walking BACKWARDS: `e` = tokens [0, e) of the block's OUTPUT that a consumer needs (e >= 1).  Fills the
// windows that must run and returns the prefix of the block's INPUT that those windows read as unmasked keys.
inline int swin_block_extent_back(int e, int S, int shift, int32_t *n_win, int32_t *wrap) {
    const int nw = S / 6;
    if (S <= 6) shift = 0;                 // torchvision disables the shift when one window covers the map
    if (shift == 0) {
        *n_win = std::min(nw, (e + 5) / 6);
        *wrap = 0;
        return std::min(S, 6 * *n_win);
    }
    // shifted by 3: window w < nw - 1 holds tokens [6 w + 3, 6 w + 9), the wrap window (nw - 1) holds [S - 3, S) and [0, 3) in two
    // mask regions.  Tokens [0, 3) are always needed, so the wrap window always runs; its far half enters as masked keys only.
    *n_win = std::min(nw - 1, (std::max(e - 3, 0) + 5) / 6);
    *wrap = 1;
    return *n_win == nw - 1 ? S : 3 + 6 * *n_win;
}

// nunif_hip_swin_unet_tile_extents: see nunif_hip.h.  Everything is separable per axis — the stitch reads a rectangle of a tile, a
// token needs the rectangle of its window, PatchDown / PatchUp are 2 x 2 per pixel — so each axis is walked on its own from the stitch
// back to the stem.  Returns 0, or a message (static storage) for the caller to report.
inline const char *swin_tile_extents_host(const nunif_tile_grid *g, int32_t tile_index, const int32_t *blocks_per_stage,
                                          const int32_t *shifts, int32_t to_image_fused, nunif_swin_block_extent *out) {
    (void)to_image_fused;      // fused or not, ToImage maps one token to scale x scale pixels: the extents are the same
    if (!(g && blocks_per_stage && shifts && out)) return "tile_extents: NULL argument";
    if (!(tile_index >= 0 && tile_index < g->h_blocks * g->w_blocks)) return swin_plan_msg("tile_extents: tile %lld outside the grid", tile_index);
    const int S = g->tile_size - 16;
    if (!(S > 0 && S % 24 == 0 && g->scale > 0 && g->out_tile_size == S * g->scale))
        return swin_plan_msg("tile_extents: the grid is not a swin_unet grid (tile %lld, output tile %lld)", g->tile_size, g->out_tile_size);
    int first[6] = {0};
    for (int st = 0; st < 5; ++st) {
        if (blocks_per_stage[st] < 0) return "tile_extents: negative block count";
        first[st + 1] = first[st] + blocks_per_stage[st];
    }
    const int size[5] = {S, S / 2, S / 4, S / 2, S};
    const int ti[2] = {tile_index / g->w_blocks, tile_index % g->w_blocks};
    const int y_len[2] = {g->y_h, g->y_w};
    for (int ax = 0; ax < 2; ++ax) {
        // stitch_kernel (stitch.hip) reads pixel t = Y - output_tile_step * i of tile i for every output row / column Y of the frame
        // with 0 <= t < out_tile_size, blend margins included: the prefix [0, min(out_tile_size, y_len - output_tile_step * i))
        const int n_px = std::min(g->out_tile_size, y_len[ax] - g->output_tile_step * ti[ax]);
        auto stage_back = [&](int st, int e) {         // e: needed prefix of the stage's output -> of its input
            for (int i = blocks_per_stage[st] - 1; i >= 0; --i) {
                nunif_swin_block_extent &o = out[first[st] + i];
                if (e <= 0) { o.n_win[ax] = 0; o.wrap[ax] = 0; continue; }
                e = swin_block_extent_back(e, size[st], shifts[first[st] + i], &o.n_win[ax], &o.wrap[ax]);
            }
            return std::max(e, 0);
        };
        const int e5 = n_px <= 0 ? 0 : std::min(S, (n_px + g->scale - 1) / g->scale);    // to_image: one token -> scale x scale pixels
        const int top_in = stage_back(4, e5);                          // swin5 reads PatchUp(swin4) + the swin1 skip
        const int e4_in = stage_back(3, (top_in + 1) / 2);             // PatchUp: token i of the fine map reads token i / 2
        const int e3_in = stage_back(2, (e4_in + 1) / 2);
        // a skip connection takes the larger of its two consumers; PatchDown: token j reads tokens 2 j and 2 j + 1
        const int e2_in = stage_back(1, std::min(size[1], std::max(2 * e3_in, e4_in)));
        (void)stage_back(0, std::min(size[0], std::max(2 * e2_in, top_in)));
    }
    return nullptr;
}

// What the plan builder reads of a net.
struct SwinSkipNet {
    int32_t blocks[5];         // blocks of swin1 .. swin5
    int32_t dim[5];            // channels of each stage
    bool fast[5];              // every block of the stage runs the fused attention / register-chained tail kernels
    bool has_proj2;            // the 4x net: proj2 reads the whole level-1 map
    bool producer_lists;       // level 3 can apply: base_dim 96 and down2 as two K = 384 passes
};

// One piece of a plan; offsets in 32-bit words from the start of the plan's device allocation.
//   BLOCK96 / BLOCK192: block `block` of stage `stage` runs the `n` windows at `list`, one entry per active window,
//     (tile in the minibatch << 16 | window row << 8 | window column), tile-major.  C = 96: the attention kernel writes window i of the
//     list at slot i of the window-major att map and the tail walks `pixmap` (token 36 i + t -> pixel; n_tokens ints that
//     launch_winmap_list_build fills on the device).  C = 192: the attention kernel writes a listed window at its own pixels and the tail
//     walks `groups`, the same n_tokens tokens in pixel order packed 16 to a group (n_groups of 8 words, swin_tail_groups_host.h).
//   PRODUCER: producer `stage` (NUNIF_SWIN_PRODUCER_*) walks the `n` tokens at `list` (filled up to a multiple of 32,
//     swin_producer_tokens_host.h).  A producer without an entry runs whole tiles.
enum { SWIN_SKIP_BLOCK96 = 0, SWIN_SKIP_BLOCK192 = 1, SWIN_SKIP_PRODUCER = 2 };
struct SwinSkipEntry {
    int kind, stage, block, shift;
    size_t list, groups, pixmap;
    int64_t n, n_groups, n_tokens;
};

// layout of the allocation: words (all lists and group tables, one upload) | the C = 96 token tables, 256-byte aligned
struct SwinSkipPlanHost {
    std::vector<uint32_t> words;
    size_t table_bytes = 0;
    std::vector<SwinSkipEntry> entries;       // blocks in forward order, then producers; empty: the minibatch runs whole tiles
    // level 3: the producers use their lists, all of them or none.  One without an entry runs whole tiles — the stem and down1 always (their lists
    // measured no faster), the others where their set is the whole map.  That is safe in any mix: a whole-tile producer WRITES a superset,
    // and what it READS is whole only behind producers that write whole maps too (the stem and down1 in front of everything; a whole set
    // of up2 / up1 makes every set in front of it whole through the recurrence)
    bool producers = false;
    size_t list_bytes() const { return (words.size() * 4 + 255) / 256 * 256; }
    size_t bytes() const { return list_bytes() + table_bytes; }
};

// The plan of tile minibatch [tile_begin, tile_begin + B) of grid g at NUNIF_SWIN_SKIP_PAD level `level` (1 = level-1 C = 96 blocks
// only, 2 = every fast block, 3 = the producers as well).  What a tile runs depends on the grid and the tile's index alone — never on
// the minibatch — so any split of a frame into minibatches computes the same bits.
//
// INVARIANT the skipping rests on: WRITTEN IS A SUPERSET OF READ — no launch of a frame render reads a token that no launch of the
// same frame wrote before it, so nothing stale (a previous frame's or geometry's values, finite or not) is ever an operand.
//   * Blocks.  A block that lists reads and updates, in place, exactly the tokens of its listed windows, the far half of a shifted
//     block's wrap window included (read as masked keys).  A C = 96 tail walks the compact list through `pixmap`, and the compact att
//     map is written in full before it is read; a C = 192 tail walks the tokens of exactly the windows its attention ran (`groups`).
//     A block that does not list (the generic path, a stage that is not all `fast`, a minibatch with nothing to leave out) runs whole
//     tiles and reads every token of its map.
//   * Producers (the stem, PatchDown down1 / both passes of down2, PatchUp up2 / up1).  Level 3: down2, up2 and up1 list (the stem and
//     down1 run whole tiles, a superset: their lists measured no faster); a producer that lists writes the tokens that anything
//     behind it in the frame reads — the read set of the consuming stage, the 2 x 2 parents of what a PatchDown must produce, the
//     inputs of a PatchUp whose children are read, and the skip tokens a PatchUp adds onto in place
//     (swin_producer_tokens_host.h has the recurrence) — and reads only what the producer in front of it wrote.  The
//     lists are used together or not at all; a block that runs whole tiles makes its stage's read set the whole map.  Levels 0 - 2,
//     tile mode, taps: every producer processes whole tiles, which is a superset of everything.
//   * The un-fused to_image and the 4x net's proj2 run whole tiles: proj2 reads the whole level-1 map, so the stem of that net writes
//     all of it (f1_whole), and the whole top map it writes is what the un-fused to_image reads.
// Returns 0, or a message (static storage) for the caller to report; *plan is then unspecified.
inline const char *swin_skip_plan_host(const nunif_tile_grid *g, int32_t tile_begin, int32_t B, int32_t level, const SwinSkipNet &net,
                                       SwinSkipPlanHost *plan) {
    if (!(g && plan && B > 0)) return "skip_plan: bad argument";
    *plan = SwinSkipPlanHost();
    const int S = g->tile_size - 16;
    // (a list entry packs the tile in 16 bits and a window coordinate in 8; the tails index 96 tok elements in 32 bits)
    if (!(S > 6 && S / 6 < 256 && B < 65536 && 96LL * B * S * S < (1LL << 31))) return "skip_plan: tile side or minibatch unsupported";
    std::vector<int32_t> shifts;
    for (int st = 0; st < 5; ++st) {
        if (net.blocks[st] < 0) return "skip_plan: negative block count";
        for (int i = 0; i < net.blocks[st]; ++i) shifts.push_back(i % 2 == 1 ? 3 : 0);      // swin_unet.py:30
    }
    const size_t n_blocks = shifts.size();
    std::vector<nunif_swin_block_extent> ext((size_t)B * n_blocks);          // [tile][block]
    std::vector<int32_t> listed(n_blocks, 0);
    const char *msg;
    for (int b = 0; b < B; ++b)
        if ((msg = swin_tile_extents_host(g, tile_begin + b, net.blocks, shifts.data(), 0, ext.data() + (size_t)b * n_blocks))) return msg;
    std::vector<uint32_t> &words = plan->words;
    auto align8 = [&]() { words.resize((words.size() + 7) / 8 * 8); };
    int first = 0;
    for (int st = 0; st < 5; first += net.blocks[st], ++st) {
        const int dim = net.dim[st];
        // level 1: level 1 of the 1x / 2x nets and swin1 of the 4x net; level 2: every stage of fast blocks
        if (!net.fast[st] || !(level >= 2 ? dim == 96 || dim == 192 : (st == 0 || st == 4) && dim == 96)) continue;
        const int Ss = st == 0 || st == 4 ? S : (st == 2 ? S / 4 : S / 2), nw = Ss / 6;       // this stage's token map
        if (Ss <= 6) continue;
        for (int i = 0; i < net.blocks[st]; ++i) {
            const size_t at = words.size();
            for (int b = 0; b < B; ++b) {
                const nunif_swin_block_extent &e = ext[(size_t)b * n_blocks + first + i];
                auto active = [&](int ax, int w) { return w < e.n_win[ax] || (e.wrap[ax] && w == nw - 1); };
                for (int wy = 0; wy < nw; ++wy) {
                    if (!active(0, wy)) continue;
                    for (int wx = 0; wx < nw; ++wx)
                        if (active(1, wx)) words.push_back((uint32_t)b << 16 | (uint32_t)wy << 8 | (uint32_t)wx);
                }
            }
            const size_t n = words.size() - at;
            if (n == (size_t)B * nw * nw || n == 0) { words.resize(at); continue; }   // nothing to leave out: the whole-tile path
            SwinSkipEntry en = {dim == 192 ? SWIN_SKIP_BLOCK192 : SWIN_SKIP_BLOCK96, st, i, shifts[first + i], at, 0, 0, (int64_t)n, 0, 36 * (int64_t)n};
            if (dim == 192) {
                // the same tokens in pixel order, 16 to a group: 8 words per group behind the list, 32-byte aligned
                std::vector<nunif_swin_block_extent> eb(B);
                for (int b = 0; b < B; ++b) eb[b] = ext[(size_t)b * n_blocks + first + i];
                // (one pass: 36 n tokens fill ceil(36 n / 16) groups; the slack is for a group closed early, which the builder never needs)
                const int64_t cap = (36 * (int64_t)n + 15) / 16 + 8;
                align8();
                en.groups = words.size();
                words.resize(en.groups + 8 * (size_t)cap);
                static_assert(sizeof(nunif_swin_tail_group) == 8 * sizeof(uint32_t), "a group is 8 words of the plan");
                int64_t n_tokens = 0;
                if ((msg = swin_tail_groups_host(eb.data(), B, Ss, en.shift, (nunif_swin_tail_group *)&words[en.groups], cap, &en.n_groups, &n_tokens)))
                    return msg;
                words.resize(en.groups + 8 * (size_t)en.n_groups);
                if (n_tokens != en.n_tokens) return swin_plan_msg("internal: %lld grouped tokens for %lld windows", n_tokens, (long long)n);
            }
            plan->entries.push_back(en);
            listed[first + i] = 1;
        }
    }
    if (plan->entries.empty()) return nullptr;
    // level 3: what the producers write, behind the lists in the same upload.  down2, up2, up1: the stem and down1 keep whole tiles
    // (96 % of their work is listed on a 1080p frame, and their listed launches measured no faster than the whole ones: DESIGN.md 4.13b)
    plan->producers = level >= 3 && net.producer_lists;
    for (int pr = NUNIF_SWIN_PRODUCER_DOWN2; plan->producers && pr <= NUNIF_SWIN_PRODUCER_UP1; ++pr) {
        const int Sp = pr == NUNIF_SWIN_PRODUCER_UP1 ? S / 2 : S / 4;
        const int64_t whole = (int64_t)B * Sp * Sp;
        auto tokens = [&](uint32_t *out, int64_t cap, int64_t *n) {
            return swin_producer_tokens_host(ext.data(), B, net.blocks, shifts.data(), listed.data(), S, net.has_proj2 ? 1 : 0, pr, 0, 0, out, cap, n);
        };
        int64_t n = 0;
        if ((msg = tokens(nullptr, 0, &n))) return msg;
        if (n <= 0 || n > whole) return swin_plan_msg("internal: producer %lld lists %lld of %lld", pr, n, whole);
        if (n == whole) continue;              // nothing to leave out: no entry
        const int64_t cap = (n + 31) / 32 * 32;
        align8();
        const size_t at = words.size();
        words.resize(at + (size_t)cap);
        if ((msg = tokens(&words[at], cap, &n))) return msg;
        plan->entries.push_back({SWIN_SKIP_PRODUCER, pr, 0, 0, at, 0, 0, n, 0, n});
    }
    size_t pix = plan->list_bytes() / 4;
    for (SwinSkipEntry &en : plan->entries)
        if (en.kind == SWIN_SKIP_BLOCK96) { en.pixmap = pix; pix += (size_t)en.n_tokens; }
    plan->table_bytes = pix * 4 - plan->list_bytes();
    return nullptr;
}

}  // namespace nunif
