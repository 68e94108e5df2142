// Stand-alone check of nunif_amd/csrc/swin_skip_plan_host.h under the host sanitizers (tests/test_swin_skip_plan_host.py): the plans of
// tiles 64, 112 and 160 on a ragged and an exactly filled frame each, minibatches 1, 3 and the whole grid, levels 1 - 3, for a 2x-like,
// a 4x-like and a 4xl-like net.  Every list is compared with a brute-force enumeration from the extents, every group table and producer
// list with a direct call of its builder into an exactly sized heap buffer; offsets, alignment and padding are checked, and what a tile
// runs must not depend on the minibatch.  Prints one "plan {...}" record per plan of the two golden frames (minibatch 3).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nunif_amd/csrc/swin_skip_plan_host.h"

using namespace nunif;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// nunif_hip_tile_grid_init for a swin_unet net (offset 8 * scale, blend 4 * scale): create_config of the reference's seam_blending.py
static nunif_tile_grid make_grid(int x_h, int x_w, int scale, int tile) {
    nunif_tile_grid g = {};
    const int io = 8, ib = 4, step = tile - (2 * io + ib);
    int hb = 0, wb = 0, in_h = 0, in_w = 0;
    while (in_h < x_h + 2 * io) { in_h = hb * step + tile; ++hb; }
    while (in_w < x_w + 2 * io) { in_w = wb * step + tile; ++wb; }
    g.x_h = x_h; g.x_w = x_w; g.scale = scale; g.offset = 8 * scale; g.tile_size = tile; g.blend_size = 4 * scale;
    g.y_h = x_h * scale; g.y_w = x_w * scale; g.h_blocks = hb; g.w_blocks = wb;
    g.pad_l = io; g.pad_r = in_w - (x_w + io); g.pad_t = io; g.pad_b = in_h - (x_h + io);
    g.y_buffer_h = in_h * scale; g.y_buffer_w = in_w * scale;
    g.input_tile_step = step; g.output_tile_step = step * scale; g.out_tile_size = tile * scale - 16 * scale;
    return g;
}

static const SwinSkipNet kNet2x = {{2, 2, 6, 2, 2}, {96, 192, 192, 192, 96}, {true, true, true, true, true}, false, true};
static const SwinSkipNet kNet4x = {{2, 2, 6, 2, 2}, {96, 192, 192, 192, 192}, {true, true, true, true, true}, true, true};
static const SwinSkipNet kNet4xl = {{2, 2, 6, 2, 2}, {192, 384, 384, 384, 384}, {false, false, false, false, false}, true, false};

static int side_of(int S, int st) { return st == 0 || st == 4 ? S : (st == 2 ? S / 4 : S / 2); }
static int first_of(const SwinSkipNet &net, int st) { int f = 0; for (int k = 0; k < st; ++k) f += net.blocks[k]; return f; }

static const SwinSkipEntry *find_entry(const SwinSkipPlanHost &p, int kind_producer, int stage, int block) {
    for (const SwinSkipEntry &e : p.entries)
        if ((e.kind == SWIN_SKIP_PRODUCER) == (kind_producer != 0) && e.stage == stage && e.block == block) return &e;
    return nullptr;
}

// the tokens a group table names, in table order (nunif_hip.h: slot r of a group is adj[p] + r, p the last piece that starts at or before r)
static std::vector<int64_t> group_tokens(const uint32_t *w, int64_t n_groups) {
    std::vector<int64_t> out;
    for (int64_t k = 0; k < n_groups; ++k) {
        nunif_swin_tail_group g;
        std::memcpy(&g, w + 8 * k, sizeof(g));
        const int cnt = (int)(g.bounds >> 25 & 31);
        CHECK(cnt >= 1 && cnt <= 16);
        for (int r = 0; r < cnt; ++r) {
            int p = 0;
            for (int q = 1; q < 6; ++q)
                if ((int)(g.bounds >> (5 * (q - 1)) & 31) <= r) p = q;
            out.push_back((int64_t)g.adj[p] + r);
        }
    }
    return out;
}

// What one plan makes one tile (index b of its minibatch) run: per block the windows, per producer the tokens, both relative to the tile
struct TileWork {
    std::vector<std::vector<uint32_t>> windows;      // [block]
    std::vector<std::vector<int64_t>> tokens;        // [producer DOWN2 .. UP1]
};

static TileWork tile_work(const SwinSkipPlanHost &p, const SwinSkipNet &net, int S, int b) {
    TileWork tw;
    for (int st = 0; st < 5; ++st)
        for (int i = 0; i < net.blocks[st]; ++i) {
            const int nw = side_of(S, st) / 6;
            std::vector<uint32_t> v;
            if (const SwinSkipEntry *e = find_entry(p, 0, st, i)) {
                for (int64_t k = 0; k < e->n; ++k)
                    if ((int)(p.words[e->list + k] >> 16) == b) v.push_back(p.words[e->list + k] & 0xffff);
            } else {                                 // no entry: whole tiles
                for (int wy = 0; wy < nw; ++wy)
                    for (int wx = 0; wx < nw; ++wx) v.push_back((uint32_t)wy << 8 | (uint32_t)wx);
            }
            tw.windows.push_back(v);
        }
    for (int pr = NUNIF_SWIN_PRODUCER_DOWN2; pr <= NUNIF_SWIN_PRODUCER_UP1; ++pr) {
        const int64_t Sp = pr == NUNIF_SWIN_PRODUCER_UP1 ? S / 2 : S / 4, per = Sp * Sp;
        std::vector<int64_t> v;
        if (const SwinSkipEntry *e = find_entry(p, 1, pr, 0)) {
            for (int64_t k = 0; k < e->n; ++k)
                if ((int64_t)p.words[e->list + k] / per == b) v.push_back((int64_t)p.words[e->list + k] % per);
        } else {
            for (int64_t t = 0; t < per; ++t) v.push_back(t);
        }
        tw.tokens.push_back(v);
    }
    return tw;
}

static unsigned long long fnv1a64(const std::vector<uint32_t> &words) {
    unsigned long long h = 1469598103934665603ull;
    for (uint32_t w : words)
        for (int k = 0; k < 4; ++k) { h ^= (w >> (8 * k)) & 255u; h *= 1099511628211ull; }
    return h;
}

static void print_record(const nunif_tile_grid &g, int t0, int B, int level, const SwinSkipPlanHost &p) {
    std::printf("plan {\"tile\": %d, \"h\": %d, \"w\": %d, \"scale\": %d, \"tile_begin\": %d, \"B\": %d, \"level\": %d, \"n_words\": %zu, \"fnv1a64\": \"%016llx\", \"pieces\": [",
                g.tile_size, g.x_h, g.x_w, g.scale, t0, B, level, p.words.size(), fnv1a64(p.words));
    for (size_t k = 0; k < p.entries.size(); ++k) {
        const SwinSkipEntry &e = p.entries[k];
        const int kind = e.kind == SWIN_SKIP_BLOCK96 ? 96 : (e.kind == SWIN_SKIP_BLOCK192 ? 192 : 0);
        std::printf("%s{\"kind\": %d, \"stage\": %d, \"block\": %d, \"shift\": %d, \"list\": %zu, \"n\": %lld, \"groups\": %zu, \"n_groups\": %lld}", k ? ", " : "",
                    kind, e.stage, e.block, e.shift, e.list, (long long)e.n, e.groups, (long long)e.n_groups);
    }
    std::printf("], \"table_bytes\": %zu}\n", p.table_bytes);
}

// one plan against the brute force; returns it for the per-tile comparison
static SwinSkipPlanHost check_plan(const nunif_tile_grid &g, int t0, int B, int level, const SwinSkipNet &net) {
    SwinSkipPlanHost p;
    const char *msg = swin_skip_plan_host(&g, t0, B, level, net, &p);
    CHECK(msg == nullptr);
    if (msg) { std::printf("  %s\n", msg); return p; }
    const int S = g.tile_size - 16;
    int32_t shifts[14];
    int n_blocks = 0;
    for (int st = 0; st < 5; ++st)
        for (int i = 0; i < net.blocks[st]; ++i) shifts[n_blocks++] = i % 2 ? 3 : 0;
    std::vector<nunif_swin_block_extent> ext((size_t)B * n_blocks);
    for (int b = 0; b < B; ++b) CHECK(swin_tile_extents_host(&g, t0 + b, net.blocks, shifts, 0, &ext[(size_t)b * n_blocks]) == nullptr);
    // pieces in the order they must lie in the buffer: [first word, one past the last)
    struct Span { size_t a, b; };
    std::vector<Span> spans, tables;
    std::vector<int32_t> listed(n_blocks, 0);
    size_t n_expected = 0;
    for (int st = 0; st < 5; ++st)
        for (int i = 0; i < net.blocks[st]; ++i) {
            const int Ss = side_of(S, st), nw = Ss / 6, blk = first_of(net, st) + i, dim = net.dim[st];
            std::vector<uint32_t> want;
            for (int b = 0; b < B; ++b) {
                const nunif_swin_block_extent &e = ext[(size_t)b * n_blocks + blk];
                for (int wy = 0; wy < nw; ++wy)
                    for (int wx = 0; wx < nw; ++wx)
                        if ((wy < e.n_win[0] || (e.wrap[0] && wy == nw - 1)) && (wx < e.n_win[1] || (e.wrap[1] && wx == nw - 1)))
                            want.push_back((uint32_t)b << 16 | (uint32_t)wy << 8 | (uint32_t)wx);
            }
            const bool eligible = net.fast[st] && Ss > 6 && (level >= 2 ? dim == 96 || dim == 192 : (st == 0 || st == 4) && dim == 96);
            const bool lists = eligible && !want.empty() && want.size() != (size_t)B * nw * nw;
            const SwinSkipEntry *e = find_entry(p, 0, st, i);
            CHECK((e != nullptr) == lists);
            if (!e) continue;
            ++n_expected;
            listed[blk] = 1;
            CHECK(e->kind == (dim == 192 ? SWIN_SKIP_BLOCK192 : SWIN_SKIP_BLOCK96) && e->shift == shifts[blk]);
            CHECK(e->n == (int64_t)want.size() && e->n_tokens == 36 * e->n && e->list + want.size() <= p.words.size());
            if (e->list + want.size() > p.words.size()) continue;
            CHECK(std::equal(want.begin(), want.end(), p.words.begin() + e->list));
            spans.push_back({e->list, e->list + want.size()});
            if (dim == 96) {
                CHECK(e->n_groups == 0);
                tables.push_back({e->pixmap, e->pixmap + (size_t)e->n_tokens});
                continue;
            }
            std::vector<nunif_swin_block_extent> eb(B);
            for (int b = 0; b < B; ++b) eb[b] = ext[(size_t)b * n_blocks + blk];
            int64_t ng = 0, nt = 0, ng2 = 0;
            CHECK(swin_tail_groups_host(eb.data(), B, Ss, shifts[blk], nullptr, 0, &ng, &nt) == nullptr);
            CHECK(ng == e->n_groups && nt == e->n_tokens && e->groups % 8 == 0 && e->groups + 8 * (size_t)ng <= p.words.size());
            if (ng != e->n_groups || e->groups + 8 * (size_t)ng > p.words.size()) continue;
            nunif_swin_tail_group *tab = (nunif_swin_tail_group *)std::malloc(sizeof(nunif_swin_tail_group) * (size_t)ng);
            CHECK(swin_tail_groups_host(eb.data(), B, Ss, shifts[blk], tab, ng, &ng2, &nt) == nullptr && ng2 == ng);
            CHECK(std::memcmp(tab, &p.words[e->groups], sizeof(nunif_swin_tail_group) * (size_t)ng) == 0);
            std::free(tab);
            spans.push_back({e->groups, e->groups + 8 * (size_t)ng});
            // the tail walks exactly the tokens of the windows the attention runs, each once
            std::vector<int64_t> toks = group_tokens(&p.words[e->groups], ng), from_windows;
            const int shift = Ss <= 6 ? 0 : shifts[blk];
            for (uint32_t w : want)
                for (int t = 0; t < 36; ++t) {
                    const int y = (6 * (int)(w >> 8 & 255) + shift + t / 6) % Ss, x = (6 * (int)(w & 255) + shift + t % 6) % Ss;
                    from_windows.push_back(((int64_t)(w >> 16) * Ss + y) * Ss + x);
                }
            std::sort(from_windows.begin(), from_windows.end());
            CHECK(toks == from_windows);
        }
    // producers: level 3, and only in a plan whose blocks list
    const bool producers = level >= 3 && net.producer_lists && n_expected > 0;
    CHECK(p.producers == producers);
    for (int pr = NUNIF_SWIN_PRODUCER_STEM; pr <= NUNIF_SWIN_PRODUCER_UP1; ++pr) {
        const SwinSkipEntry *e = find_entry(p, 1, pr, 0);
        if (!producers || pr < NUNIF_SWIN_PRODUCER_DOWN2) { CHECK(e == nullptr); continue; }
        const int Sp = pr == NUNIF_SWIN_PRODUCER_UP1 ? S / 2 : S / 4;
        int64_t n = 0, n2 = 0;
        CHECK(swin_producer_tokens_host(ext.data(), B, net.blocks, shifts, listed.data(), S, net.has_proj2, pr, 0, 0, nullptr, 0, &n) == nullptr);
        CHECK((e != nullptr) == (n != (int64_t)B * Sp * Sp));
        if (!e) continue;
        ++n_expected;
        const size_t cap = (size_t)(n + 31) / 32 * 32;
        CHECK(e->n == n && e->list % 8 == 0 && e->list + cap <= p.words.size());
        if (e->n != n || e->list + cap > p.words.size()) continue;
        uint32_t *tab = (uint32_t *)std::malloc(sizeof(uint32_t) * cap);
        CHECK(swin_producer_tokens_host(ext.data(), B, net.blocks, shifts, listed.data(), S, net.has_proj2, pr, 0, 0, tab, (int64_t)cap, &n2) == nullptr);
        CHECK(n2 == n && std::memcmp(tab, &p.words[e->list], sizeof(uint32_t) * cap) == 0);
        std::free(tab);
        spans.push_back({e->list, e->list + cap});
    }
    CHECK(p.entries.size() == n_expected);
    // the pieces lie in entry order without overlap; what is between them is alignment padding (zero, under 8 words) and the buffer ends
    // with the last piece; the token tables follow 256-byte aligned and back to back
    size_t at = 0;
    for (const Span &s : spans) {
        CHECK(s.a >= at && s.a - at < 8 && s.b <= p.words.size());
        for (size_t k = at; k < s.a && k < p.words.size(); ++k) CHECK(p.words[k] == 0);
        at = s.b;
    }
    CHECK(at == p.words.size());
    CHECK(p.list_bytes() % 256 == 0 && p.list_bytes() >= 4 * p.words.size() && p.list_bytes() < 4 * p.words.size() + 256);
    at = p.list_bytes() / 4;
    for (const Span &s : tables) { CHECK(s.a == at); at = s.b; }
    CHECK(p.bytes() == at * 4 && p.table_bytes == at * 4 - p.list_bytes());
    if (p.entries.empty()) CHECK(p.words.empty() && p.bytes() == 0);
    return p;
}

// every minibatch split of a frame: each plan against the brute force, each tile's work against the whole-grid plan's
static void check_frame(int tile, int h, int w, int scale, const SwinSkipNet &net, bool expect_entries, bool golden) {
    const nunif_tile_grid g = make_grid(h, w, scale, tile);
    const int n_tiles = g.h_blocks * g.w_blocks, S = tile - 16;
    CHECK(n_tiles >= 4);
    for (int level = 1; level <= 3; ++level) {
        const SwinSkipPlanHost whole = check_plan(g, 0, n_tiles, level, net);
        CHECK(!whole.entries.empty() == expect_entries);
        for (int mb : {1, 3}) {
            bool any = false;
            for (int t0 = 0; t0 < n_tiles; t0 += mb) {
                const int B = std::min(mb, n_tiles - t0);
                const SwinSkipPlanHost p = check_plan(g, t0, B, level, net);
                any = any || !p.entries.empty();
                if (golden && mb == 3 && !p.entries.empty()) print_record(g, t0, B, level, p);
                for (int b = 0; b < B; ++b) {
                    const TileWork mine = tile_work(p, net, S, b), ref = tile_work(whole, net, S, t0 + b);
                    CHECK(mine.windows == ref.windows);
                    CHECK(mine.tokens == ref.tokens);
                }
            }
            CHECK(any == expect_entries);
        }
    }
}

int main() {
    // (tile, ragged frame, net): the 112 and 160 frames are the golden ones (tests/golden/swin_skip_plan_words.json)
    check_frame(64, 60, 70, 2, kNet2x, true, false);
    check_frame(112, 130, 98, 2, kNet2x, true, true);
    check_frame(160, 150, 146, 4, kNet4x, true, true);
    // frames that fill their 2 x 2 tiles exactly (side S + input step): nothing to leave out, no entries
    check_frame(64, 92, 92, 2, kNet2x, false, false);
    check_frame(112, 188, 188, 2, kNet2x, false, false);
    check_frame(160, 284, 284, 4, kNet4x, false, false);
    // no fast stage: every block runs whole tiles
    check_frame(160, 150, 146, 4, kNet4xl, false, false);

    SwinSkipPlanHost p;
    nunif_tile_grid g = make_grid(130, 98, 2, 112);
    CHECK(swin_skip_plan_host(&g, 0, 4, 3, kNet2x, &p) == nullptr);
    CHECK(swin_skip_plan_host(&g, 2, 3, 3, kNet2x, &p) != nullptr);            // tile 4 of 4
    CHECK(swin_skip_plan_host(&g, -1, 1, 3, kNet2x, &p) != nullptr);
    CHECK(swin_skip_plan_host(&g, 0, 0, 3, kNet2x, &p) != nullptr);
    CHECK(swin_skip_plan_host(nullptr, 0, 1, 3, kNet2x, &p) != nullptr && swin_skip_plan_host(&g, 0, 1, 3, kNet2x, nullptr) != nullptr);
    SwinSkipNet bad = kNet2x;
    bad.blocks[2] = -6;
    CHECK(swin_skip_plan_host(&g, 0, 1, 3, bad, &p) != nullptr);
    nunif_tile_grid cunet = g;                 // not a swin_unet grid: another offset, a side that is no multiple of 24
    cunet.out_tile_size = g.tile_size * g.scale - 56;
    CHECK(swin_skip_plan_host(&cunet, 0, 1, 3, kNet2x, &p) != nullptr);
    cunet = make_grid(130, 98, 2, 100);
    CHECK(swin_skip_plan_host(&cunet, 0, 1, 3, kNet2x, &p) != nullptr);
    nunif_swin_block_extent e[14];
    const int32_t shifts[14] = {0, 3, 0, 3, 0, 3, 0, 3, 0, 3, 0, 3, 0, 3};
    CHECK(swin_tile_extents_host(&g, 4, kNet2x.blocks, shifts, 0, e) != nullptr);
    CHECK(swin_tile_extents_host(&g, 3, bad.blocks, shifts, 0, e) != nullptr);
    CHECK(swin_tile_extents_host(&cunet, 0, kNet2x.blocks, shifts, 0, e) != nullptr);
    CHECK(swin_tile_extents_host(&g, 3, kNet2x.blocks, shifts, 0, nullptr) != nullptr);
    if (fails) { std::printf("swin_skip_plan_host: %d check(s) failed\n", fails); return 1; }
    std::printf("swin_skip_plan_host: ok\n");
    return 0;
}
