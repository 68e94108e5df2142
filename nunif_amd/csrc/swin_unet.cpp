// Host side of the waifu2x swin_unet engine: weight repacking, workspace, launch sequence, whole-frame render.
//
// Reference: waifu2x/models/swin_unet.py SwinUNetBase.__init__/forward :119-199 (layer inventory and data flow),
// nunif/utils/seam_blending.py tiled_render :48-106 (frame loop).  State-dict keys are the reference's.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <list>
#include <string>
#include <vector>

#include "packed_layers.h"
#include "swin_skip_plan_host.h"

namespace nunif {

int launch_stitch(const float *tile_out, float *y, const nunif_tile_grid *g, int C, hipStream_t s, int y0 = 0, int rows = -1,
                  int compact = 0);

namespace {

struct Block {
    PackedLinear qkv, proj, mlp0, mlp3;
    // generic path (LayerNorm variants, head counts other than 6: swin_unet_4xl): mlp.0 / mlp.3 in the PLAIN k order for
    // gemm_kernel, LayerNormNoBias weights (nunif/modules/norm.py:17-22)
    PackedLinear mlp0p, mlp3p;
    float *norm1 = nullptr, *norm2 = nullptr;
    bool fast = true;             // fused qkv+attention / register-chained tail kernels apply
    float *attn_bias = nullptr;   // [heads][36][48]
    f16 *tail_stream = nullptr;   // proj | mlp.0 | mlp.3 fragments in proj_mlp_kernel's consumption order
    f16 *tail_ws = nullptr;       // C = 192: per-slice fragments of the weight-stationary tail (swin_block_tail_ws.hip)
    // LDS-resident attention (swin_qkv_attn_r.hip): per head Wq | Wk | Wv fragments, q rows / q bias pre-multiplied by
    // head_dim^-0.5 * log2(e); fp32 bias table [heads][36][52] * log2(e) read as the MFMA C operand, padded keys = -1000
    f16 *qkv_res = nullptr;
    float *qkv_rbias = nullptr;
    float *attn_btab32 = nullptr;
    // C = 96: one kernel per block (swin_block96.hip): proj (chained k) | mlp fragments, compact reversed bias table
    f16 *b96_tail = nullptr;
    float *b96_btab = nullptr;
};

// A block's entry of a plan (SwinSkipEntry, swin_skip_plan_host.h) as device pointers; list == NULL: the block runs whole tiles
struct SkipBlock {
    unsigned *list = nullptr;
    int *pixmap = nullptr;
    const nunif_swin_tail_group *groups = nullptr;
    long n_groups = 0, n_tokens = 0;
    int n_windows = 0;
};

// A producer's entry of a plan as a device pointer: `n` output tokens (PatchDown) or input tokens (PatchUp).  list == NULL: the
// whole-tile launch.
struct ProducerList {
    const unsigned *list = nullptr;
    unsigned n = 0;
};

// One plan per (grid, tile minibatch, level).  Everything of a plan lives in ONE device allocation: the words the host builder laid out
// (uploaded once, `host` keeps the source alive for the asynchronous copy) and behind them the token tables, which a kernel builds
// from the lists on the stream that first uses the plan (launch_winmap_list_build) — `ready` orders any other stream behind that.
struct SkipPlan {
    nunif_tile_grid grid = {};
    int tile_begin = 0, B = 0;
    int level = 0;                        // NUNIF_SWIN_SKIP_PAD of the call that built it
    SwinSkipPlanHost host;
    std::vector<SkipBlock> stage[5];      // host.entries resolved against `dev`; empty where the stage runs whole
    ProducerList producer[5];             // indexed by NUNIF_SWIN_PRODUCER_*
    void *dev = nullptr;
    size_t bytes = 0;
    hipStream_t built_on = nullptr;
    hipEvent_t ready = nullptr;
    void release() {
        if (ready) (void)hipEventDestroy(ready);
        (void)hipFree(dev);               // (synchronises the device: no launch that reads the plan is still in flight)
    }
};

}  // namespace
}  // namespace nunif

using namespace nunif;

// Pure integer host functions (declared in nunif_hip.h): swin_skip_plan_host.h, swin_producer_tokens_host.h, swin_tail_groups_host.h
extern "C" int nunif_hip_swin_unet_tile_extents(const nunif_tile_grid *g, int32_t tile_index, const int32_t *blocks_per_stage,
                                                const int32_t *shifts, int32_t to_image_fused, nunif_swin_block_extent *out) {
    const char *msg = swin_tile_extents_host(g, tile_index, blocks_per_stage, shifts, to_image_fused, out);
    NUNIF_REQUIRE(!msg, "%s", msg);
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_swin_unet_producer_tokens(const nunif_swin_block_extent *ext, int32_t n_tiles, const int32_t *blocks_per_stage,
                                                   const int32_t *shifts, const int32_t *listed, int32_t S, int32_t f1_whole,
                                                   int32_t producer, int32_t patch_h, int32_t patch_w, uint32_t *out, int64_t cap,
                                                   int64_t *n_out) {
    const char *msg = swin_producer_tokens_host(ext, n_tiles, blocks_per_stage, shifts, listed, S, f1_whole, producer, patch_h, patch_w,
                                                out, cap, n_out);
    NUNIF_REQUIRE(!msg, "%s", msg);
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_swin_unet_tail_groups(const nunif_swin_block_extent *ext, int32_t n_tiles, int32_t S, int32_t shift,
                                               nunif_swin_tail_group *out, int64_t cap, int64_t *n_groups, int64_t *n_tokens) {
    const char *msg = swin_tail_groups_host(ext, n_tiles, S, shift, out, cap, n_groups, n_tokens);
    NUNIF_REQUIRE(!msg, "%s", msg);
    return NUNIF_HIP_OK;
}

struct nunif_swin_unet : DeviceOwner {       // owns every device allocation made at create time
    int scale_factor = 2;
    int C = 96, heads = 6;
    int C1 = 48, C1P = 64;            // stem conv1 channels (real / padded to a multiple of 32)
    int top_dim = 96;                 // channels of level 1 on the decoder side (C for 1x/2x, 2C for 4x)
    float *stem1_w = nullptr, *stem1_b = nullptr;
    PackedLinear stem2, down1, down2, up2, up1, proj2, to_image, to_image_pre;
    PackedLinear down2b;                    // second tap row of down2 when 4 * Cin > 1024 (swin_unet_4xl: K = 1536 as two K = 768 passes)
    bool down2_split = false;
    f16 *to_image_chained = nullptr;  // ToImage weights in the chained k order, for the fused head of the last C = 96 block
    f16 *stemf_w1 = nullptr, *stemf_w2 = nullptr;   // fused stem (swin_stem.hip)
    int dir = 0;                      // direction of the next kernel (snake order); next_dir() flips it
    int att_wm = 1;                   // NUNIF_ATT_WM=0: C = 96 att map pixel-major (8-byte partial-line stores) as in round 2
    int gelu32 = 0;                   // tails with the fp32-polynomial GELU: the 1x net (swin_gelu.h); NUNIF_SWIN_GELU32=0/1 overrides
    int block96 = 0;                  // NUNIF_BLOCK96=1: C = 96 blocks as ONE kernel (swin_block96.hip) instead of attention + tail
    bool has_proj2 = false;
    std::vector<Block> swin[5];
    DeviceBuf s1, f1, f2, f3, g1, qkv, att, hid, tile_out;
    // token -> pixel tables of the window-major C = 96 tail (launch_winmap_build), one per shift, for the geometry last seen
    DeviceBuf winmap[2];
    int winmap_B = 0, winmap_S = 0;
    // pad skipping of the frame entry points: one plan (window lists + token tables) per grid and tile
    // minibatch, of every grid the handle has rendered.  Most recently used first, so a handle that alternates between frame
    // sizes or minibatches finds its plans again; evicted from the back beyond kMaxPlans / kMaxPlanBytes.
    std::list<SkipPlan> plans;
    size_t plan_bytes = 0;
    const SkipPlan *plan = nullptr;   // the plan of the forward_impl call under way (NULL: whole tiles)
    void drop_plan(std::list<SkipPlan>::iterator it) {
        it->release();
        plan_bytes -= it->bytes;
        plans.erase(it);
    }
    void clear_plans() {
        while (!plans.empty()) drop_plan(plans.begin());
        plan = nullptr;
    }
    int device = 0;
    // debug taps (tests only): when on, every stage's fp16 output is snapshotted device-side
    struct Tap { std::string name; void *dev; size_t bytes; };
    bool taps_on = false;
    std::vector<Tap> taps;
    void clear_taps() { for (auto &t : taps) (void)hipFree(t.dev); taps.clear(); }
};

namespace nunif {
namespace {

// proj | mlp.0 | mlp.3 as one linear stream of 1-KiB fragments in the order proj_mlp_kernel (swin_block_tail.hip) and the block96
// kernel consume them; returns the number of fragments written
size_t put_tail_stream(const std::vector<f16> &proj, const std::vector<f16> &h0, const std::vector<f16> &h3, int dim, std::vector<f16> &stream) {
    const int KS = dim / 32, NT = dim / 16, SH = 2 * dim / 32;
    size_t fi = 0;
    auto put = [&](const std::vector<f16> &src, int frag) { copy_frag(src, frag, stream, &fi); };
    for (int sx = 0; sx < KS; ++sx)
        for (int ks = 0; ks < KS; ++ks) { put(proj, (2 * sx) * KS + ks); put(proj, (2 * sx + 1) * KS + ks); }
    for (int sx = 0; sx < SH; ++sx) {
        for (int ks = 0; ks < KS; ++ks) { put(h0, (2 * sx) * KS + ks); put(h0, (2 * sx + 1) * KS + ks); }
        for (int nt = 0; nt < NT; ++nt) put(h3, nt * SH + sx);
    }
    return fi;
}

int make_stage(nunif_swin_unet *h, const TensorMap &m, const std::string &key, int dim, int layers,
               std::vector<Block> *blocks) {
    blocks->resize(layers);
    const int heads = h->heads;
    for (int i = 0; i < layers; ++i) {
        const std::string p = key + ".block." + std::to_string(i) + ".";
        Block &bl = (*blocks)[i];
        int rc;
        if ((rc = linear_from(h, m, p + "attn.qkv", 3 * dim, dim, 16, &bl.qkv))) return rc;
        const bool has_norm = m.find(p + "norm1.weight") != m.end();
        bl.fast = heads == 6 && (dim == 96 || dim == 192) && !has_norm;
        if (has_norm) {
            // LayerNormNoBias (swin_unet_4xl, swin_unet.py:390-391): x = x + attn(norm1(x)); x = x + mlp(norm2(x))
            const HostTensor *n1, *n2;
            if ((rc = find(m, p + "norm1.weight", &n1)) || (rc = find(m, p + "norm2.weight", &n2))) return rc;
            NUNIF_REQUIRE(n1->numel == dim && n2->numel == dim, "%snorm: shape", p.c_str());
            NUNIF_REQUIRE(m.find(p + "norm1.bias") == m.end(), "%snorm1: LayerNorm with bias is not a reference variant", p.c_str());
            std::vector<float> g1(n1->data, n1->data + dim), g2(n2->data, n2->data + dim);
            if ((rc = h->upload(g1, &bl.norm1)) || (rc = h->upload(g2, &bl.norm2))) return rc;
        }
        if (!bl.fast) {
            if ((rc = linear_from(h, m, p + "attn.proj", dim, dim, 16, &bl.proj)) ||
                (rc = linear_from(h, m, p + "mlp.0", 2 * dim, dim, 16, &bl.mlp0p)) ||
                (rc = linear_from(h, m, p + "mlp.3", dim, 2 * dim, 16, &bl.mlp3p)))
                return rc;
        }
        if (bl.fast) {
            const HostTensor *w, *b;
            if ((rc = find(m, p + "attn.qkv.weight", &w)) || (rc = find(m, p + "attn.qkv.bias", &b))) return rc;
            const float qs = (1.0f / sqrtf((float)(dim / heads))) * 1.4426950408889634f;
            const float *wd = w->data;
            std::vector<f16> hs = pack_nt_ks(3 * dim, 3 * dim, dim, [=](int n, int k) {
                return wd[(size_t)n * dim + k] * (n < dim ? qs : 1.0f); });
            // per head: Wq tiles, Wk tiles, Wv tiles, each (nt, ks) fragment-major — the order qkv_attn_r_kernel reads them
            const int KS = dim / 32, NTH = (dim / heads) / 16, nf = 3 * (dim / 16) * KS;
            std::vector<f16> stream((size_t)nf * 512, (f16)0.0f);
            size_t fi = 0;
            for (int hh = 0; hh < heads; ++hh)
                for (int part = 0; part < 3; ++part)
                    for (int nt = 0; nt < NTH; ++nt)
                        for (int ks = 0; ks < KS; ++ks)
                            copy_frag(hs, (size_t)(part * (dim / 16) + hh * NTH + nt) * KS + ks, stream, &fi);
            if ((rc = h->upload(stream, &bl.qkv_res))) return rc;
            std::vector<float> rb(3 * dim);
            for (int n = 0; n < 3 * dim; ++n) rb[n] = b->data[n] * (n < dim ? qs : 1.0f);
            if ((rc = h->upload(rb, &bl.qkv_rbias))) return rc;
        }
        LinearHost hp, h0, h3;
        if (bl.fast) {
        if ((rc = linear_from(h, m, p + "attn.proj", dim, dim, 16, &bl.proj, false, &hp))) return rc;
        if ((rc = linear_from(h, m, p + "mlp.0", 2 * dim, dim, 16, &bl.mlp0, true, &h0))) return rc;   // chained
        if ((rc = linear_from(h, m, p + "mlp.3", dim, 2 * dim, 16, &bl.mlp3, true, &h3))) return rc;   // chained
        }
        if (bl.fast) {
            const int KS = dim / 32, SH = 2 * dim / 32;
            const int nf = proj_mlp_stream_frags(dim);
            std::vector<f16> stream((size_t)(nf + 15) / 16 * 16 * 512, (f16)0.0f);     // whole 16-fragment chunks
            const size_t fi = put_tail_stream(hp.w, h0.w, h3.w, dim, stream);
            NUNIF_REQUIRE((int)fi == nf, "internal: tail stream has %zu fragments, expected %d", fi, nf);
            if ((rc = h->upload(stream, &bl.tail_stream))) return rc;
            if (dim == 192) {
                // weight-stationary tail: output-channel slice w of 4 owns proj / mlp.3 tiles 3w..3w+2 and mlp.0 tiles 6w..6w+5
                //   Wp [w][nt 3][ks 6] (plain k order) | W0 [w][nt 6][ks 6] | W3 [w][nt 3][ks 12] (both chained)
                std::vector<f16> ws((size_t)proj_mlp_ws_stream_frags() * 512, (f16)0.0f);
                size_t wi = 0;
                auto putw = [&](const std::vector<f16> &src, int frag) { copy_frag(src, frag, ws, &wi); };
                for (int w = 0; w < 4; ++w)
                    for (int nt = 0; nt < 3; ++nt)
                        for (int ks = 0; ks < KS; ++ks) putw(hp.w, (3 * w + nt) * KS + ks);
                for (int w = 0; w < 4; ++w)
                    for (int nt = 0; nt < 6; ++nt)
                        for (int ks = 0; ks < KS; ++ks) putw(h0.w, (6 * w + nt) * KS + ks);
                for (int w = 0; w < 4; ++w)
                    for (int nt = 0; nt < 3; ++nt)
                        for (int ks = 0; ks < SH; ++ks) putw(h3.w, (3 * w + nt) * SH + ks);
                NUNIF_REQUIRE((int)wi == proj_mlp_ws_stream_frags(), "internal: ws tail stream has %zu fragments", wi);
                if ((rc = h->upload(ws, &bl.tail_ws))) return rc;
            }
        }
        const HostTensor *tab;
        if ((rc = find(m, p + "attn.relative_position_bias_table", &tab))) return rc;
        NUNIF_REQUIRE(tab->numel == 121 * heads, "%s: bias table shape", p.c_str());
        if (bl.fast && dim == 96) {
            // fused block kernel: attn.proj re-packed in the chained k order (its B operand is the attention output taken
            // straight from the accumulators of head pairs), followed by the mlp part of the tail stream unchanged
            const HostTensor *pw;
            if ((rc = find(m, p + "attn.proj.weight", &pw))) return rc;
            const float *pd = pw->data;
            std::vector<f16> hpc = pack_nt_ks(dim, dim, dim, [=](int n, int k) { return pd[(size_t)n * dim + k]; }, true);
            std::vector<f16> stream((size_t)swin_block96_tail_frags() * 512, (f16)0.0f);
            const size_t fi = put_tail_stream(hpc, h0.w, h3.w, dim, stream);
            NUNIF_REQUIRE((int)fi == swin_block96_tail_frags(), "internal: block96 stream has %zu fragments", fi);
            if ((rc = h->upload(stream, &bl.b96_tail))) return rc;
            // R[h][i] = log2(e) * table[120 - i][h]: the keys of a 2 x 2 block are then at +0, +1, +11, +12 from the
            // lane's index (swin_block96.hip); floats 124.. of a head = -1000 (padded keys)
            const int stride = swin_block96_btab_floats() / heads;
            std::vector<float> rt((size_t)heads * stride, -1000.0f);
            for (int hh = 0; hh < heads; ++hh) {
                for (int i2 = 0; i2 < 121; ++i2) rt[(size_t)hh * stride + i2] = tab->data[(size_t)(120 - i2) * heads + hh] * 1.4426950408889634f;
                rt[(size_t)hh * stride + 121] = rt[(size_t)hh * stride + 122] = rt[(size_t)hh * stride + 123] = 0.0f;
            }
            if ((rc = h->upload(rt, &bl.b96_btab))) return rc;
        }
        // bias[h][q][key] = table[(yq-yk+5)*11 + (xq-xk+5)][h]  (torchvision relative_position_index, window 6x6);
        // the 12 padding key columns get -1e30 so that exp() makes them exactly 0.
        std::vector<float> bias((size_t)heads * 36 * 48);
        for (int hh = 0; hh < heads; ++hh)
            for (int q = 0; q < 36; ++q)
                for (int k = 0; k < 48; ++k) {
                    float v = -1.0e30f;
                    if (k < 36) {
                        const int idx = (q / 6 - k / 6 + 5) * 11 + (q % 6 - k % 6 + 5);
                        v = tab->data[(size_t)idx * heads + hh];
                    }
                    bias[((size_t)hh * 36 + q) * 48 + k] = v;
                }
        if ((rc = h->upload(bias, &bl.attn_bias))) return rc;
        // fp32 table read as the MFMA C operand: [heads][36 queries][52], log2(e) * bias.  Key COLUMNS follow the token
        // placement of qkv_attn_r_kernel (win_token, swin_qkv_attn_r.hip): columns 0..31 = keys 0..31, column 32 + 4 g =
        // key 32 + g (register 0 of lane group g in key tile 2); the other columns of tile 2 are padding the kernel never
        // exponentiates (-1000 all the same)
        std::vector<float> btab32((size_t)heads * 36 * 52, 0.0f);
        for (int hh = 0; hh < heads; ++hh)
            for (int q = 0; q < 36; ++q)
                for (int k = 0; k < 48; ++k) {
                    const int key = k < 32 ? k : (((k - 32) & 3) == 0 ? 32 + ((k - 32) >> 2) : -1);
                    btab32[((size_t)hh * 36 + q) * 52 + k] =
                        key >= 0 ? bias[((size_t)hh * 36 + q) * 48 + key] * 1.4426950408889634f : -1000.0f;
                }
        if ((rc = h->upload(btab32, &bl.attn_btab32))) return rc;
    }
    return NUNIF_HIP_OK;
}

int run_gemm(const PackedLinear &L, const f16 *a, int B, int Hi, int Wi, int Cin, int Ho, int Wo, int stride, int oy,
             int ox, int kw, int mode, int act, float slope, const f16 *res, void *out, int ldo, int ps,
             hipStream_t s, const char *tag, int rev = 0) {
    GemmArgs g = gemm_map_args(L, a, B, Hi, Wi, Cin, Ho, Wo, out, stride, kw, oy, ox);
    g.mode = mode; g.act = act; g.slope = slope; g.res = res; g.ldo = ldo; g.ps = ps; g.rev = rev;
    return launch_gemm(g, s, tag);
}

// x = PatchUp(a) + skip, in place over the skip map (swin_unet.py:65-82,189-196): the resident-weight kernel when it takes the
// shape (every launch of that shape, whatever the batch: results must not depend on the tile minibatch), else the generic GEMM
// `pl` (frame renders): only the listed input tokens; a launch that cannot take the list is an error, never a whole-tile launch
int run_patchup(const PackedLinear &L, const f16 *a, int B, int H, int W, int Cq, f16 *skip, hipStream_t s, const char *tag, int rev,
                const ProducerList *pl = nullptr) {
    PatchUpArgs p = {a, L.w, L.bias, skip, skip, B, H, W, Cq, rev};
    if (pl && pl->list) { p.list = pl->list; p.n_list = pl->n; }
    if (L.K == 192 && L.n_real == 4 * Cq && patchup_supported(p)) return launch_patchup(p, s);
    NUNIF_REQUIRE(!p.list, "%s: no listed form of this PatchUp", tag);
    return run_gemm(L, a, B, H, W, L.K, H, W, 1, 0, 0, 1, 1, 0, 0.f, skip, skip, Cq, 1, s, tag, rev);
}

// PatchDown pass without a residual (swin_unet.py:45-62): a [B, 2 Ho, 2 Wo, Cin] -> out [B, Ho, Wo, 192], K = 384 = the taps of
// input row(s) 2 y + oy ..; the K-outer prefetching kernel when it takes the shape (every launch of that shape), else the generic GEMM
// acc: out += the pass (down2's second tap row).  `pl` as run_patchup's, output tokens.
int run_patchdown(const PackedLinear &L, const f16 *a, int B, int Ho, int Wo, int Cin, int oy, f16 *out, hipStream_t s, const char *tag,
                  int rev, const ProducerList *pl = nullptr, int acc = 0) {
    PatchDownArgs p;
    p.a = a; p.w = L.w; p.bias = L.bias; p.out = out; p.B = B; p.Ho = Ho; p.Wo = Wo; p.Cin = Cin; p.oy = oy; p.rev = rev; p.acc = acc;
    if (pl && pl->list) { p.list = pl->list; p.n_list = pl->n; }
    if (L.K == 384 && L.n_real == 192 && patchdown_supported(p)) return launch_patchdown(p, s);
    NUNIF_REQUIRE(!p.list, "%s: no listed form of this PatchDown", tag);
    if (acc) return run_gemm(L, a, B, 2 * Ho, 2 * Wo, Cin, Ho, Wo, 2, oy, 0, 2, 0, 0, 0.f, out, out, L.n_real, 1, s, tag, rev);
    return run_gemm(L, a, B, 2 * Ho, 2 * Wo, Cin, Ho, Wo, 2, oy, 0, 2, 0, 0, 0.f, nullptr, out, L.n_real, 1, s, tag, rev);
}

int run_linear(const PackedLinear &L, const f16 *a, int B, int H, int W, int act, const f16 *res, f16 *out,
               hipStream_t s, const char *tag, int rev = 0) {
    return run_gemm(L, a, B, H, W, L.K, H, W, 1, 0, 0, 1, 0, act, 0.f, res, out, L.n_real, 1, s, tag, rev);
}

int tap(nunif_swin_unet *h, const std::string &name, const void *src, size_t bytes, hipStream_t s) {
    if (!h->taps_on) return NUNIF_HIP_OK;
    void *p = nullptr;
    NUNIF_HIP_CHECK(hipMalloc(&p, bytes));
    NUNIF_HIP_CHECK(hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToDevice, s));
    h->taps.push_back({name, p, bytes});
    return NUNIF_HIP_OK;
}

// Snake order: consecutive kernels walk their tokens in opposite directions, so each one starts on the lines its
// predecessor touched last (still in the 256-MB memory-side cache) — measured +1.3 % on the 1080p 2x frame with only the
// attention kernels reversed.  Results do not depend on the walk order.
static int next_dir(nunif_swin_unet *h) {
    const int d = h->dir;
    h->dir ^= 1;
    return d;
}

int run_stage(nunif_swin_unet *h, std::vector<Block> &blocks, f16 *x, int B, int S, int dim, hipStream_t s,
              const char *name, const TailToImage *to_image = nullptr, const std::vector<SkipBlock> *skip = nullptr) {
    f16 *qkv = (f16 *)h->qkv.p, *att = (f16 *)h->att.p;
    const size_t tok = (size_t)B * S * S;
    int rc;
    for (size_t i = 0; i < blocks.size(); ++i) {
        Block &bl = blocks[i];
        const int shift = (i % 2 == 1) ? 3 : 0;      // swin_unet.py:30
        const std::string tn = std::string(name) + ".b" + std::to_string(i);
        // fast blocks (6 heads, no norm): qkv Linear + attention in one kernel (one window per wave, weights resident in LDS);
        // the 3C-wide qkv map never exists in HBM.  Everything else takes the generic composition below.
        if (!bl.fast) {
            // generic block (swin_unet_4xl: 12 heads, LayerNormNoBias): every Linear on gemm_kernel, attention on the
            // fused-qkv-map kernel, the two LayerNorms as their own pass.  att / hid double as the normalised maps.
            f16 *hid = (f16 *)h->hid.p;
            const f16 *xin = x;
            if (bl.norm1) {
                if ((rc = launch_layernorm_nobias(x, hid, bl.norm1, (long)tok, dim, s))) return rc;
                xin = hid;
            }
            if ((rc = run_linear(bl.qkv, xin, B, S, S, 0, nullptr, qkv, s, "gemm_qkv", next_dir(h)))) return rc;
            if ((rc = tap(h, tn + ".qkv", qkv, tok * 3 * dim * 2, s))) return rc;
            if ((rc = launch_window_attn(qkv, att, bl.attn_bias, B, S, S, h->heads, dim / h->heads, shift, s))) return rc;
            if ((rc = tap(h, tn + ".attn", att, tok * dim * 2, s))) return rc;
            if ((rc = run_linear(bl.proj, att, B, S, S, 0, x, x, s, "gemm_proj", next_dir(h)))) return rc;
            xin = x;
            if (bl.norm2) {
                if ((rc = launch_layernorm_nobias(x, att, bl.norm2, (long)tok, dim, s))) return rc;
                xin = att;
            }
            if ((rc = run_linear(bl.mlp0p, xin, B, S, S, 1, nullptr, hid, s, "gemm_mlp0", next_dir(h)))) return rc;
            if ((rc = run_linear(bl.mlp3p, hid, B, S, S, 0, x, x, s, "gemm_mlp3", next_dir(h)))) return rc;
            if ((rc = tap(h, tn + ".out", x, tok * dim * 2, s))) return rc;
            continue;
        }
        const bool last_blk = i + 1 == blocks.size();
        if (dim == 96 && bl.b96_tail && h->block96 && !h->taps_on) {
            // C = 96: the whole block in one kernel, x updated in place (swin_block96.hip)
            if ((rc = launch_swin_block96(x, bl.qkv_res, bl.qkv_rbias, bl.b96_btab, bl.b96_tail, bl.proj.bias, bl.mlp0.bias,
                                          bl.mlp3.bias, B, S, S, shift, s, last_blk ? to_image : nullptr, next_dir(h))))
                return rc;
            if (last_blk && to_image) break;
            continue;
        }
        // C = 96: att travels in window-major order (full-line stores in the attention kernel, the tail walks its tokens in
        // window order); debug taps want the pixel-major map the oracle has
        // (the tail indexes the window-major map in 32 bits: 96 tok elements; larger launches take the pixel-major map)
        const bool att_wm = dim == 96 && h->att_wm && !h->taps_on && 96L * (long)tok < (1L << 31);
        // frame renders: only the windows the stitch depends on (skip_plan).  C = 96: att is then compact, slot i = window i of the
        // list; C = 192: att stays pixel-major, written at the listed windows only, and the tail walks the same tokens (sk->groups)
        const SkipBlock *sk = skip && i < skip->size() && (*skip)[i].list && (dim == 192 ? (*skip)[i].groups != nullptr : att_wm)
                                  ? &(*skip)[i] : nullptr;
        if ((rc = launch_qkv_attn_r(x, att, bl.qkv_res, bl.qkv_rbias, bl.attn_btab32, B, S, S, dim, h->heads, shift, s, next_dir(h),
                                    att_wm ? 1 : 0, sk ? sk->list : nullptr, sk ? sk->n_windows : 0)))
            return rc;
        if ((rc = tap(h, tn + ".attn", att, tok * dim * 2, s))) return rc;
        // x = y + mlp(y), y = x + proj(attn): three GEMMs chained through registers, one read + one write of x
        const bool last = i + 1 == blocks.size();
        if (dim == 192) {
            // C = 192: weights stationary in registers / LDS (swin_block_tail_ws.hip)
            if ((rc = launch_proj_mlp_ws(att, x, bl.tail_ws, bl.proj.bias, bl.mlp0.bias, bl.mlp3.bias, (long)tok, s, next_dir(h), h->gelu32,
                                         sk ? sk->groups : nullptr, sk ? sk->n_groups : 0, sk ? sk->n_tokens : 0)))
                return rc;
        } else {
            const int eff_shift = S <= 6 ? 0 : shift;
            WinMap wmap = {att_wm ? 1 : 0, S, S, eff_shift, nullptr};
            if (sk) {
                wmap.pixmap = sk->pixmap;
            } else if (att_wm) {
                if (h->winmap_S != S || B > h->winmap_B) {
                    // (re)build both tables on this stream: every launch that reads them is ordered behind it.  The table of a
                    // larger batch contains the smaller one's as its prefix (token n -> batch n / (36 windows per image))
                    for (int k = 0; k < 2; ++k) {
                        if ((rc = h->winmap[k].ensure(tok * sizeof(int)))) return rc;
                        if ((rc = launch_winmap_build((int *)h->winmap[k].p, B, S, S, k ? 3 : 0, s))) return rc;
                    }
                    h->winmap_B = B; h->winmap_S = S;
                }
                wmap.pixmap = (const int *)h->winmap[eff_shift ? 1 : 0].p;
            }
            if ((rc = launch_proj_mlp(att, x, bl.tail_stream, bl.proj.bias, bl.mlp0.bias, bl.mlp3.bias, sk ? 36L * sk->n_windows : (long)tok, dim, s,
                                      last ? to_image : nullptr, next_dir(h), &wmap, h->gelu32)))
                return rc;
        }
        if (last && to_image) break;               // x of the last block is not materialised
        if ((rc = tap(h, tn + ".out", x, tok * dim * 2, s))) return rc;
    }
    return NUNIF_HIP_OK;
}

int ensure_workspace(nunif_swin_unet *h, int B, int T) {
    const size_t S = T - 16, S2 = S / 2, S4 = S / 4, C = h->C;
    const size_t t1 = (size_t)B * S * S, t2 = (size_t)B * S2 * S2, t3 = (size_t)B * S4 * S4;
    const size_t top = h->top_dim;
    int rc;
    if ((rc = h->s1.ensure((size_t)B * (T - 14) * (T - 14) * h->C1P * 2))) return rc;
    if ((rc = h->f1.ensure(t1 * C * 2))) return rc;
    if ((rc = h->f2.ensure(t2 * 2 * C * 2))) return rc;
    if ((rc = h->f3.ensure(t3 * 2 * C * 2))) return rc;
    if (h->has_proj2 && (rc = h->g1.ensure(t1 * top * 2))) return rc;
    const size_t qkv_elems = std::max(t1 * 3 * std::max(C, top), t2 * 6 * C);
    if ((rc = h->qkv.ensure(qkv_elems * 2))) return rc;
    if ((rc = h->att.ensure(std::max(t1 * std::max(C, top), t2 * 2 * C) * 2))) return rc;
    if ((rc = h->hid.ensure(std::max(t1 * 2 * std::max(C, top), t2 * 4 * C) * 2))) return rc;
    return NUNIF_HIP_OK;
}

// Plan bytes per tile of 256 whose every block lists: 4 C = 96 blocks x 1 600 windows x 148 B + 2 200 windows of the 10 C = 192 blocks
// x (4 B + 36 / 16 groups x 32 B) = 0.95 + 0.17 MB, so kMaxPlanBytes holds about 950 tiles: 21 geometries of 1080p (a plan lists every
// tile of its minibatch once one of them has windows to leave out).  The producer lists (down2, up2, up1) add 4 B per token: (14 400 + 2 x 3 600) x 4 B =
// 0.09 MB per tile of 256.
constexpr size_t kMaxPlans = 1024, kMaxPlanBytes = (size_t)1 << 30;

// The device half of a plan with entries: one allocation, one upload of plan->host.words, the C = 96 token tables built behind them on
// `s`, the entries resolved to device pointers.  On failure the caller releases what was made.
int upload_plan(SkipPlan *plan, int S, hipStream_t s) {
    const SwinSkipPlanHost &host = plan->host;
    if (hipMalloc(&plan->dev, host.bytes()) != hipSuccess) {
        set_error("hipMalloc(%zu) of the window lists failed", host.bytes());
        return NUNIF_HIP_ENOMEM;
    }
    plan->bytes = host.bytes();
    if (hipMemcpyAsync(plan->dev, host.words.data(), host.words.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipEventCreateWithFlags(&plan->ready, hipEventDisableTiming) != hipSuccess) {
        set_error("upload of the window lists failed");
        return NUNIF_HIP_EHIP;
    }
    unsigned *dev = (unsigned *)plan->dev;
    for (const SwinSkipEntry &e : host.entries) {
        if (e.kind == SWIN_SKIP_PRODUCER) {
            plan->producer[e.stage] = {dev + e.list, (unsigned)e.n};
            continue;
        }
        std::vector<SkipBlock> &blocks = plan->stage[e.stage];
        if (blocks.size() <= (size_t)e.block) blocks.resize(e.block + 1);
        SkipBlock &sb = blocks[e.block];
        sb.list = dev + e.list;
        sb.n_windows = (int)e.n;
        sb.n_tokens = (long)e.n_tokens;
        if (e.kind == SWIN_SKIP_BLOCK192) {
            sb.groups = (const nunif_swin_tail_group *)(dev + e.groups);
            sb.n_groups = (long)e.n_groups;
            continue;
        }
        sb.pixmap = (int *)(dev + e.pixmap);
        int rc = launch_winmap_list_build(sb.pixmap, sb.list, sb.n_windows, S, S, e.shift, s);
        if (rc) return rc;
    }
    if (hipEventRecord(plan->ready, s) != hipSuccess) { set_error("hipEventRecord failed"); return NUNIF_HIP_EHIP; }
    return NUNIF_HIP_OK;
}

// The plan of tile minibatch [t0, t0 + B) of grid g (frame entry points only; NULL: whole tiles): the cached one, or a new one from
// swin_skip_plan_host (which has the INVARIANT the skipping rests on).  A plan enters the cache complete or not at all.
int skip_plan(nunif_swin_unet *h, const nunif_tile_grid *g, int t0, int B, int level, hipStream_t s, const SkipPlan **out) {
    *out = nullptr;
    const int S = g->tile_size - 16, nw = S / 6;
    if (!h->att_wm || h->taps_on || h->block96 || S <= 6 || nw >= 256 || B >= 65536 || 96L * B * S * S >= (1L << 31) ||
        g->out_tile_size != S * g->scale)
        return NUNIF_HIP_OK;
    for (auto it = h->plans.begin(); it != h->plans.end(); ++it)
        if (it->tile_begin == t0 && it->B == B && it->level == level && memcmp(g, &it->grid, sizeof(*g)) == 0) {
            h->plans.splice(h->plans.begin(), h->plans, it);
            if (it->dev && it->built_on != s) NUNIF_HIP_CHECK(hipStreamWaitEvent(s, it->ready, 0));
            *out = &*it;
            return NUNIF_HIP_OK;
        }
    SwinSkipNet net = {};
    for (int st = 0; st < 5; ++st) {
        net.blocks[st] = (int32_t)h->swin[st].size();
        net.dim[st] = st == 0 ? h->C : (st == 4 ? h->top_dim : 2 * h->C);
        net.fast[st] = std::all_of(h->swin[st].begin(), h->swin[st].end(), [](const Block &bl) { return bl.fast; });
    }
    net.has_proj2 = h->has_proj2;
    net.producer_lists = h->C == 96 && h->down2_split;
    SkipPlan plan;
    plan.grid = *g; plan.tile_begin = t0; plan.B = B; plan.level = level; plan.built_on = s;
    const char *msg = swin_skip_plan_host(g, t0, B, level, net, &plan.host);
    NUNIF_REQUIRE(!msg, "%s", msg);
    // (a plan without entries is cached all the same, with dev == NULL: the next frame finds it)
    int rc = plan.host.entries.empty() ? NUNIF_HIP_OK : upload_plan(&plan, S, s);
    if (rc) {
        plan.release();
        return rc;
    }
    h->plan_bytes += plan.bytes;
    h->plans.push_front(std::move(plan));
    while (h->plans.size() > kMaxPlans || (h->plan_bytes > kMaxPlanBytes && h->plans.size() > 1)) h->drop_plan(std::prev(h->plans.end()));
    *out = &h->plans.front();
    return NUNIF_HIP_OK;
}

// What both stems (Stem1Args, StemFusedArgs) read of their input: tiles, or the frame and where its tiles lie; the rest is zeroed
template <typename Args>
void stem_input(Args *a, const float *x, const float *frame, const nunif_tile_grid *grid, int tile_begin, int B, int T) {
    memset(a, 0, sizeof(*a));
    a->x = frame ? frame : x;
    if (frame) {
        a->frame_mode = 1; a->H = grid->x_h; a->W = grid->x_w; a->wb = grid->w_blocks;
        a->istep = grid->input_tile_step; a->pad_t = grid->pad_t; a->pad_l = grid->pad_l; a->tile_begin = tile_begin;
    }
    a->B = B; a->T = T; a->slope = 0.1f;
}

// x: tile mode [B,3,T,T] or (frame != NULL) the frame + grid; z: [B,3,S*s,S*s]
int forward_impl(nunif_swin_unet *h, const float *x, const float *frame, const nunif_tile_grid *grid,
                 int tile_begin, float *z, int B, int T, hipStream_t s, int skip_pad = 0) {
    const int S = T - 16, C = h->C;
    NUNIF_REQUIRE(T > 16 && S % 12 == 0 && S % 16 == 0, "tile_size %d is not valid for swin_unet", T);
    int rc;
    if ((rc = ensure_workspace(h, B, T))) return rc;
    h->plan = nullptr;
    if (frame && skip_pad && (rc = skip_plan(h, grid, tile_begin, B, skip_pad, s, &h->plan))) return rc;
    auto skip_of = [&](int st) { return h->plan && !h->plan->stage[st].empty() ? &h->plan->stage[st] : nullptr; };
    f16 *s1 = (f16 *)h->s1.p, *f1 = (f16 *)h->f1.p, *f2 = (f16 *)h->f2.p, *f3 = (f16 *)h->f3.p;
    // level 3: the producers' lists, all of them or none (the INVARIANT of swin_skip_plan_host.h) — none where a listed kernel is switched off
    bool lp = h->plan && h->plan->host.producers;
    if (lp) {
        PatchDownArgs d1, d2;
        d1.B = B; d1.Ho = d1.Wo = S / 4; d1.Cin = 2 * (int)C; d1.oy = 0; d1.rev = 0;
        d2 = d1; d2.oy = 1; d2.acc = 1;
        PatchUpArgs u2 = {f3, nullptr, nullptr, f2, f2, B, S / 4, S / 4, 2 * (int)C, 0}, u1 = {f2, nullptr, nullptr, f1, f1, B, S / 2, S / 2, h->top_dim, 0};
        lp = patchdown_supported(d1) && patchdown_supported(d2) && patchup_supported(u2) && patchup_supported(u1);
    }
    auto prod_of = [&](int pr) { return lp ? &h->plan->producer[pr] : nullptr; };

    h->dir = 1;                                    // the stem walks upwards; everything after it alternates
    if (h->stemf_w2 && stem_fused_supported(h->C1, (int)C)) {
        StemFusedArgs sf;
        stem_input(&sf, x, frame, grid, tile_begin, B, T);
        sf.w1 = h->stemf_w1; sf.w2 = h->stemf_w2; sf.b2 = h->stem2.bias; sf.out = f1;
        if ((rc = launch_stem_fused(sf, s))) return rc;
    } else {
        Stem1Args a1;
        stem_input(&a1, x, frame, grid, tile_begin, B, T);
        a1.w = h->stem1_w; a1.bias = h->stem1_b; a1.C1 = h->C1; a1.C1P = h->C1P; a1.out = s1;
        if ((rc = launch_stem1(a1, s))) return rc;
        // conv2 3x3 VALID + LeakyReLU(0.1) + crop 6 (swin_unet.py:135-137,182): s1 already starts at conv1 row/col 6
        if ((rc = run_gemm(h->stem2, s1, B, T - 14, T - 14, h->C1P, S, S, 1, 0, 0, 3, 0, 2, 0.1f, nullptr, f1, C, 1, s,
                           "gemm_stem2", next_dir(h))))
            return rc;
    }
    if ((rc = tap(h, "stem", f1, (size_t)B * S * S * C * 2, s))) return rc;
    if ((rc = run_stage(h, h->swin[0], f1, B, S, C, s, "swin1", nullptr, skip_of(0)))) return rc;                          // swin1 -> x3
    if ((rc = run_patchdown(h->down1, f1, B, S / 2, S / 2, C, 0, f2, s, "gemm_down1", next_dir(h), prod_of(NUNIF_SWIN_PRODUCER_DOWN1)))) return rc;
    if ((rc = tap(h, "down1", f2, (size_t)B * (S / 2) * (S / 2) * 2 * C * 2, s))) return rc;
    if ((rc = run_stage(h, h->swin[1], f2, B, S / 2, 2 * C, s, "swin2", nullptr, skip_of(1)))) return rc;                  // swin2 -> x4
    if (h->down2_split) {
        if ((rc = run_patchdown(h->down2, f2, B, S / 4, S / 4, 2 * C, 0, f3, s, "gemm_down2", next_dir(h), prod_of(NUNIF_SWIN_PRODUCER_DOWN2)))) return rc;
    } else if ((rc = run_gemm(h->down2, f2, B, S / 2, S / 2, 2 * C, S / 4, S / 4, 2, 0, 0, 2, 0, 0, 0.f, nullptr, f3,
                              2 * C, 1, s, "gemm_down2", next_dir(h))))
        return rc;
    // the second tap row accumulates onto the first's output: the same listed tokens
    if (h->down2_split && (rc = run_patchdown(h->down2b, f2, B, S / 4, S / 4, 2 * C, 1, f3, s, "gemm_down2b", next_dir(h),
                                              prod_of(NUNIF_SWIN_PRODUCER_DOWN2), 1)))
        return rc;
    if ((rc = tap(h, "down2", f3, (size_t)B * (S / 4) * (S / 4) * 2 * C * 2, s))) return rc;
    if ((rc = run_stage(h, h->swin[2], f3, B, S / 4, 2 * C, s, "swin3", nullptr, skip_of(2)))) return rc;                  // swin3
    // x = up2(x5) + x4, written in place over x4 (each lane reads then writes its own 8 bytes)
    if ((rc = run_patchup(h->up2, f3, B, S / 4, S / 4, 2 * C, f2, s, "gemm_up2", next_dir(h), prod_of(NUNIF_SWIN_PRODUCER_UP2)))) return rc;
    if ((rc = tap(h, "up2", f2, (size_t)B * (S / 2) * (S / 2) * 2 * C * 2, s))) return rc;
    if ((rc = run_stage(h, h->swin[3], f2, B, S / 2, 2 * C, s, "swin4", nullptr, skip_of(3)))) return rc;                  // swin4
    f16 *top = f1;
    if (h->has_proj2) {
        // 4x: x = up1(x) + proj2(x3)   (swin_unet.py:166,195-196)
        top = (f16 *)h->g1.p;
        if ((rc = run_linear(h->proj2, f1, B, S, S, 0, nullptr, top, s, "gemm_proj2", next_dir(h)))) return rc;
    }
    if ((rc = run_patchup(h->up1, f2, B, S / 2, S / 2, h->top_dim, top, s, "gemm_up1", next_dir(h), prod_of(NUNIF_SWIN_PRODUCER_UP1)))) return rc;
    if ((rc = tap(h, "up1", top, (size_t)B * S * S * h->top_dim * 2, s))) return rc;
    // to_image + pixel_shuffle + clamp(0,1) (ToImage.forward :110-116, wrapper eval clamp :225-226): fused into the
    // last block's tail kernel when that block runs on the resident C = 96 kernel (1x / 2x nets)
    if (h->top_dim == 96 && h->swin[4].back().fast && h->to_image_chained && !h->taps_on) {
        TailToImage ti;
        ti.w = h->to_image_chained; ti.bias = h->to_image.bias; ti.out = z; ti.H = S; ti.W = S; ti.ps = h->scale_factor;
        ti.n_real = h->to_image.n_real;
        return run_stage(h, h->swin[4], top, B, S, h->top_dim, s, "swin5", &ti, skip_of(4));
    }
    if ((rc = run_stage(h, h->swin[4], top, B, S, h->top_dim, s, "swin5", nullptr, skip_of(4)))) return rc;                // swin5
    if (h->scale_factor == 8) {
        f16 *pre = (f16 *)h->att.p;                 // the attention scratch map is free again: [B,S,S,192]
        if ((rc = run_gemm(h->to_image_pre, top, B, S, S, h->top_dim, S, S, 1, 0, 0, 1, 0, 2, 0.2f, nullptr, pre, 192, 1, s,
                           "gemm_to_image_pre", next_dir(h))))
            return rc;
        top = pre;
    }
    if ((rc = run_gemm(h->to_image, top, B, S, S, h->top_dim, S, S, 1, 0, 0, 1, 2, 0, 0.f, nullptr, z, 0,
                       h->scale_factor, s, "gemm_to_image", next_dir(h))))
        return rc;
    return NUNIF_HIP_OK;
}

}  // namespace
}  // namespace nunif

extern "C" int nunif_hip_swin_unet_create(const nunif_tensor_desc *tensors, int32_t n_tensors,
                                          int32_t scale_factor, nunif_swin_unet **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "swin_unet_create: NULL argument");
    NUNIF_REQUIRE(scale_factor == 1 || scale_factor == 2 || scale_factor == 4 || scale_factor == 8,
                  "swin_unet_create: scale_factor %d unsupported (1, 2, 4, 8)", scale_factor);
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_swin_unet *h = new nunif_swin_unet();
    (void)hipGetDevice(&h->device);
    if (const char *v = getenv("NUNIF_BLOCK96")) h->block96 = atoi(v);
    if (const char *v = getenv("NUNIF_ATT_WM")) h->att_wm = atoi(v);
    h->gelu32 = scale_factor == 1;
    if (const char *v = getenv("NUNIF_SWIN_GELU32")) h->gelu32 = atoi(v);
    h->scale_factor = scale_factor;
    const std::string P = "unet.";
    int rc = NUNIF_HIP_OK;
    do {
        const HostTensor *w0, *b0, *w2, *b2;
        if ((rc = find(m, P + "patch.0.weight", &w0)) || (rc = find(m, P + "patch.0.bias", &b0)) ||
            (rc = find(m, P + "patch.2.weight", &w2)) || (rc = find(m, P + "patch.2.bias", &b2)))
            break;
        if (w2->shape.size() != 4 || w0->shape.size() != 4 || w0->shape[1] != 3) {
            set_error("patch conv: unexpected shape"); rc = NUNIF_HIP_EINVAL; break;
        }
        const int C = (int)w2->shape[0];
        const int C1 = (int)w0->shape[0];
        if (C % 96 != 0 || C1 * 2 != C) { set_error("base_dim %d unsupported", C); rc = NUNIF_HIP_EUNSUPPORTED; break; }
        h->C = C; h->heads = C / 16; h->C1 = C1; h->C1P = pad_to(C1, 32);
        h->has_proj2 = scale_factor >= 4;
        h->top_dim = h->has_proj2 ? 2 * C : C;
        {
            std::vector<float> w(w0->data, w0->data + w0->numel), b(b0->data, b0->data + b0->numel);
            if ((rc = h->upload(w, &h->stem1_w)) || (rc = h->upload(b, &h->stem1_b))) break;
        }
        {   // conv2 [C][C1][3][3] -> W[n][k = (dy*3+dx)*C1P + ci], zero for the padded input channels
            const float *wd = w2->data;
            const int C1P = h->C1P;
            rc = make_linear(h, C, 16, 9 * C1P, [=](int n, int k) {
                const int tap = k / C1P, ci = k % C1P;
                return ci < C1 ? wd[((size_t)n * C1 + ci) * 9 + tap] : 0.0f;
            }, bias_at(b2->data), &h->stem2);
            if (rc) break;
        }
        if (stem_fused_supported(C1, C)) {
            const float *w0d = w0->data, *b0d = b0->data, *wd = w2->data;
            std::vector<f16> p1 = pack_nt_ks(C1, pad_to(C1, 16), 32, [=](int n, int k) {
                return k < 27 ? w0d[(size_t)n * 27 + k] : (k == 27 ? b0d[n] : 0.0f); });
            const int K2 = 448;
            std::vector<f16> stream = pack_ks_nt(C, C, K2, [=](int n, int k) {
                const int tap = k / C1, ci = k % C1;
                return k < 9 * C1 ? wd[((size_t)n * C1 + ci) * 9 + tap] : 0.0f; }, false, 0);
            if ((rc = h->upload(p1, &h->stemf_w1)) || (rc = h->upload(stream, &h->stemf_w2))) break;
        }
        if ((rc = make_stage(h, m, P + "swin1", C, 2, &h->swin[0]))) break;
        if ((rc = make_stage(h, m, P + "swin2", 2 * C, 2, &h->swin[1]))) break;
        if ((rc = make_stage(h, m, P + "swin3", 2 * C, 6, &h->swin[2]))) break;
        if ((rc = make_stage(h, m, P + "swin4", 2 * C, 2, &h->swin[3]))) break;
        if ((rc = make_stage(h, m, P + "swin5", h->top_dim, 2, &h->swin[4]))) break;
        auto make_down = [&](const std::string &key, int cin, int cout, PackedLinear *L) -> int {
            const HostTensor *w, *b;
            int r;
            if ((r = find(m, key + ".conv.weight", &w)) || (r = find(m, key + ".conv.bias", &b))) return r;
            NUNIF_REQUIRE(w->numel == (int64_t)cout * cin * 4, "%s: shape", key.c_str());
            const float *wd = w->data;   // [cout][cin][2][2] -> k = (i*2+j)*cin + ci
            return make_linear(h, cout, 16, 4 * cin, [=](int n, int k) {
                const int tap = k / cin, ci = k % cin;
                return wd[((size_t)n * cin + ci) * 4 + tap];
            }, bias_at(b->data), L);
        };
        auto make_up = [&](const std::string &key, int cin, int cq, PackedLinear *L) -> int {
            const HostTensor *w, *b;
            int r;
            if ((r = find(m, key + ".proj.weight", &w)) || (r = find(m, key + ".proj.bias", &b))) return r;
            NUNIF_REQUIRE(w->numel == (int64_t)4 * cq * cin, "%s: shape", key.c_str());
            const float *wd = w->data, *bd = b->data;   // rows c*4 + q  ->  q*cq + c   (pixel_shuffle(2) channel order)
            return make_linear(h, 4 * cq, 16, cin, [=](int n, int k) {
                const int q = n / cq, c = n % cq;
                return wd[((size_t)(c * 4 + q)) * cin + k];
            }, [=](int n) { return bd[(n % cq) * 4 + n / cq]; }, L);
        };
        if ((rc = make_down(P + "down1", C, 2 * C, &h->down1))) break;
        // the base_dim-96 nets' down2 runs the same way (K = 768, one token tile per wave on gemm_kernel<24,1>)
        // as two K = 384 passes on the resident-weight gemm_res_kernel<12,2>
        // (measured on the 2x net: gemm_kernel<24,1> 172 us -> 2 x 114 us - the 200 us of down1 stay = 30 us less per frame)
        {
            // gemm_kernel keeps a token's whole K extent in registers (K <= 1024): the 2x2 stride-2 conv over 2C = 384
            // channels runs as its two tap ROWS, the second accumulating onto the first's output
            const HostTensor *w, *b;
            if ((rc = find(m, P + "down2.conv.weight", &w)) || (rc = find(m, P + "down2.conv.bias", &b))) break;
            const int cin = 2 * C, cout = 2 * C;
            if (w->numel != (int64_t)cout * cin * 4) { set_error("down2: shape"); rc = NUNIF_HIP_EINVAL; break; }
            const float *wd = w->data;
            if ((rc = make_linear(h, cout, 16, 2 * cin, [=](int n, int k) {
                    const int dx = k / cin, ci = k % cin; return wd[((size_t)n * cin + ci) * 4 + dx]; }, bias_at(b->data), &h->down2)) ||
                (rc = make_linear(h, cout, 16, 2 * cin, [=](int n, int k) {
                    const int dx = k / cin, ci = k % cin; return wd[((size_t)n * cin + ci) * 4 + 2 + dx]; }, bias_at(nullptr), &h->down2b)))
                break;
            h->down2_split = true;
        }
        if ((rc = make_up(P + "up2", 2 * C, 2 * C, &h->up2))) break;
        if ((rc = make_up(P + "up1", 2 * C, h->top_dim, &h->up1))) break;
        if (h->has_proj2 && (rc = linear_from(h, m, P + "proj2", 2 * C, C, 16, &h->proj2))) break;
        if (scale_factor == 8) {
            // ToImage of the 8x net (swin_unet.py:96-101): Linear -> LeakyReLU(0.2) -> Linear, both 192 wide
            if ((rc = linear_from(h, m, P + "to_image.proj.0", 192, h->top_dim, 16, &h->to_image_pre)) ||
                (rc = linear_from(h, m, P + "to_image.proj.2", 192, 192, 16, &h->to_image)))
                break;
        } else if ((rc = linear_from(h, m, P + "to_image.proj", 3 * scale_factor * scale_factor, h->top_dim, 16, &h->to_image)))
            break;
        if (h->top_dim == 96 && 3 * scale_factor * scale_factor <= 16) {
            const HostTensor *tw;
            if ((rc = find(m, P + "to_image.proj.weight", &tw))) break;
            const float *wd = tw->data;
            const int nr = 3 * scale_factor * scale_factor, K = h->top_dim;
            std::vector<f16> ch = pack_nt_ks(nr, pad_to(nr, 16), K, [=](int n, int k) { return wd[(size_t)n * K + k]; }, true);
            if ((rc = h->upload(ch, &h->to_image_chained))) break;
        }
    } while (0);
    if (rc) {
        nunif_hip_swin_unet_destroy(h);
        return rc;
    }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_swin_unet_debug_taps(nunif_swin_unet *h, int32_t enable) {
    NUNIF_REQUIRE(h, "debug_taps: NULL handle");
    h->clear_taps();
    h->taps_on = enable != 0;
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_swin_unet_get_tap(nunif_swin_unet *h, int32_t index, char *name, int32_t name_cap,
                                           void *host_dst, int64_t cap_bytes, int64_t *nbytes) {
    NUNIF_REQUIRE(h && nbytes, "get_tap: NULL argument");
    if (index < 0 || index >= (int)h->taps.size()) return 1;   // end of list
    const auto &t = h->taps[index];
    if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    *nbytes = (int64_t)t.bytes;
    if (host_dst) {
        NUNIF_REQUIRE(cap_bytes >= (int64_t)t.bytes, "get_tap: buffer too small");
        NUNIF_HIP_CHECK(hipDeviceSynchronize());
        NUNIF_HIP_CHECK(hipMemcpy(host_dst, t.dev, t.bytes, hipMemcpyDeviceToHost));
    }
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_swin_unet_destroy(nunif_swin_unet *h) {
    if (!h) return;
    h->clear_taps();
    h->clear_plans();
    h->free_all();
    for (DeviceBuf *b : {&h->s1, &h->f1, &h->f2, &h->f3, &h->g1, &h->qkv, &h->att, &h->hid, &h->tile_out, &h->winmap[0], &h->winmap[1]}) b->release();
    delete h;
}

extern "C" int nunif_hip_swin_unet_forward(nunif_swin_unet *h, const float *x, float *z, int32_t batch,
                                           int32_t tile_size, void *stream) {
    NUNIF_REQUIRE(h && x && z && batch > 0, "swin_unet_forward: bad argument");
    return forward_impl(h, x, nullptr, nullptr, 0, z, batch, tile_size, (hipStream_t)stream);
}

// NUNIF_SWIN_SKIP_PAD, read at call time: 0 = the frame entry points push whole tiles through every block, as the tile entry always
// does; 1 = only the level-1 C = 96 blocks leave windows out (A/B runs against the C = 192 skipping); 2 = every fast block; unset or
// >= 3 = the producers as well (down2, up2, up1 list; the stem and down1 keep whole tiles)
static int skip_pad_level() {
    const char *v = getenv("NUNIF_SWIN_SKIP_PAD");
    if (!v) return 3;
    const int l = atoi(v);
    return l <= 0 ? 0 : std::min(l, 3);
}

// tiles [t_begin, t_end) of the frame in minibatches of batch_size, into the handle's tile store ([tile][3][To][To])
static int render_tiles(nunif_swin_unet *h, const float *x, const nunif_tile_grid &g, int t_begin, int t_end, int batch_size,
                        int tile_size, hipStream_t s) {
    const size_t To = g.out_tile_size;
    const int skip_pad = skip_pad_level();
    for (int t0 = t_begin; t0 < t_end; t0 += batch_size) {
        const int rc = forward_impl(h, nullptr, x, &g, t0, (float *)h->tile_out.p + (size_t)t0 * 3 * To * To, std::min(batch_size, t_end - t0),
                                    tile_size, s, skip_pad);
        if (rc) return rc;
    }
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_swin_unet_down2_test(nunif_swin_unet *h, const void *a, void *out, int32_t B, int32_t Ho, int32_t Wo,
                                              int32_t acc_form, void *stream) {
    NUNIF_REQUIRE(h && a && out && B > 0 && Ho > 0 && Wo > 0 && h->down2_split, "down2_test: bad argument");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = run_patchdown(h->down2, (const f16 *)a, B, Ho, Wo, 2 * h->C, 0, (f16 *)out, s, "gemm_down2", 0))) return rc;
    if (acc_form) {
        NUNIF_REQUIRE(patchdown_acc_enabled(), "down2_test: the accumulating PatchDown form is switched off");
        return run_patchdown(h->down2b, (const f16 *)a, B, Ho, Wo, 2 * h->C, 1, (f16 *)out, s, "gemm_down2b", 1, nullptr, 1);
    }
    return run_gemm(h->down2b, (const f16 *)a, B, 2 * Ho, 2 * Wo, 2 * h->C, Ho, Wo, 2, 1, 0, 2, 0, 0, 0.f, (const f16 *)out, out, 2 * h->C, 1, s,
                    "gemm_down2b", 1);
}

extern "C" int nunif_hip_swin_unet_tail192_test(nunif_swin_unet *h, int32_t stage, int32_t block, const void *att, void *x,
                                                int64_t n_tokens, const nunif_swin_tail_group *groups, int64_t n_groups,
                                                int64_t n_listed, int32_t rev, void *stream) {
    NUNIF_REQUIRE(h && att && x && n_tokens > 0 && stage >= 0 && stage < 5 && block >= 0 && block < (int)h->swin[stage].size(),
                  "tail192_test: bad argument");
    const Block &bl = h->swin[stage][block];
    NUNIF_REQUIRE(bl.fast && bl.tail_ws, "tail192_test: stage %d block %d has no C = 192 tail", stage, block);
    return launch_proj_mlp_ws((const f16 *)att, (f16 *)x, bl.tail_ws, bl.proj.bias, bl.mlp0.bias, bl.mlp3.bias, (long)n_tokens,
                              (hipStream_t)stream, rev ? 1 : 0, h->gelu32, groups, (long)n_groups, (long)n_listed);
}

extern "C" int nunif_hip_swin_unet_render(nunif_swin_unet *h, const float *x, float *y, int32_t x_h, int32_t x_w,
                                          int32_t tile_size, int32_t batch_size, void *stream) {
    NUNIF_REQUIRE(h && x && y && batch_size > 0, "swin_unet_render: bad argument");
    // (the reference registers its experimental 8x net with scale = 4 / offset = 64, swin_unet.py:309, which no tile grid
    //  can serve: only the per-tile forward exists for it)
    NUNIF_REQUIRE(h->scale_factor != 8, "swin_unet_render: the 8x net has no consistent tile geometry; use forward");
    const int s = h->scale_factor;
    nunif_tile_grid g;
    int rc = nunif_hip_tile_grid_init(x_h, x_w, s, 8 * s, tile_size, 4 * s, &g);   // offsets/blend: swin_unet.py:213,234,267
    if (rc) return rc;
    const int n_tiles = g.h_blocks * g.w_blocks;
    const size_t To = g.out_tile_size;
    if ((rc = h->tile_out.ensure((size_t)n_tiles * 3 * To * To * sizeof(float)))) return rc;
    if ((rc = render_tiles(h, x, g, 0, n_tiles, batch_size, tile_size, (hipStream_t)stream))) return rc;
    return launch_stitch((const float *)h->tile_out.p, y, &g, 3, (hipStream_t)stream);
}

// ---- tile-ROW sharding of ONE huge image (SURVEY.md §8e fallback): a rank renders the tiles of its tile rows, neighbours
// exchange the (out_tile_size - output_tile_step)-row overlap band of their boundary tile rows, every rank stitches its own
// band of output rows.  The tile store of the handle is addressed like the whole-frame render's ([tile][3][To][To]), so the
// stitch kernel — and therefore the blend recurrence — is the same one: a sharded render is bit-identical to a whole one.
static int rows_grid(nunif_swin_unet *h, int32_t x_h, int32_t x_w, int32_t tile_size, nunif_tile_grid *g) {
    NUNIF_REQUIRE(h->scale_factor != 8, "swin_unet: the 8x net has no consistent tile geometry");
    const int s = h->scale_factor;
    int rc = nunif_hip_tile_grid_init(x_h, x_w, s, 8 * s, tile_size, 4 * s, g);
    if (rc) return rc;
    const size_t To = g->out_tile_size;
    return h->tile_out.ensure((size_t)g->h_blocks * g->w_blocks * 3 * To * To * sizeof(float));
}

extern "C" int nunif_hip_swin_unet_render_tile_rows(nunif_swin_unet *h, const float *x, int32_t x_h, int32_t x_w,
                                                    int32_t tile_size, int32_t batch_size, int32_t row_begin,
                                                    int32_t row_end, void *stream) {
    NUNIF_REQUIRE(h && x && batch_size > 0, "swin_unet_render_tile_rows: bad argument");
    nunif_tile_grid g;
    int rc = rows_grid(h, x_h, x_w, tile_size, &g);
    if (rc) return rc;
    NUNIF_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= g.h_blocks, "tile rows [%d, %d) outside the grid of %d rows",
                  row_begin, row_end, g.h_blocks);
    return render_tiles(h, x, g, row_begin * g.w_blocks, row_end * g.w_blocks, batch_size, tile_size, (hipStream_t)stream);
}

// band: [w_blocks][3][n_rows][To] fp32 = output rows [row0, row0 + n_rows) of every tile of tile row `tile_row`
extern "C" int nunif_hip_swin_unet_tile_row_band(nunif_swin_unet *h, int32_t x_h, int32_t x_w, int32_t tile_size,
                                                 int32_t tile_row, int32_t row0, int32_t n_rows, float *band,
                                                 int32_t import_band, void *stream) {
    NUNIF_REQUIRE(h && band, "swin_unet_tile_row_band: bad argument");
    nunif_tile_grid g;
    int rc = rows_grid(h, x_h, x_w, tile_size, &g);
    if (rc) return rc;
    const int To = g.out_tile_size;
    NUNIF_REQUIRE(0 <= tile_row && tile_row < g.h_blocks && row0 >= 0 && n_rows > 0 && row0 + n_rows <= To, "tile_row_band: bad window");
    float *store = (float *)h->tile_out.p + (size_t)tile_row * g.w_blocks * 3 * To * To + (size_t)row0 * To;
    // (tile, channel) planes: To * To apart in the store, n_rows * To apart in the band
    const size_t planes = (size_t)g.w_blocks * 3;
    if (import_band)
        NUNIF_HIP_CHECK(hipMemcpy2DAsync(store, (size_t)To * To * 4, band, (size_t)n_rows * To * 4, (size_t)n_rows * To * 4, planes,
                                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else
        NUNIF_HIP_CHECK(hipMemcpy2DAsync(band, (size_t)n_rows * To * 4, store, (size_t)To * To * 4, (size_t)n_rows * To * 4, planes,
                                         hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_swin_unet_stitch_rows(nunif_swin_unet *h, float *y_band, int32_t x_h, int32_t x_w, int32_t tile_size,
                                               int32_t y_row_begin, int32_t y_row_end, void *stream) {
    NUNIF_REQUIRE(h && y_band, "swin_unet_stitch_rows: bad argument");
    nunif_tile_grid g;
    int rc = rows_grid(h, x_h, x_w, tile_size, &g);
    if (rc) return rc;
    return launch_stitch((const float *)h->tile_out.p, y_band, &g, 3, (hipStream_t)stream, y_row_begin, y_row_end - y_row_begin, 1);
}
