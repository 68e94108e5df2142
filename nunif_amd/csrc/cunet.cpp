// Host side of the waifu2x CUNet engine: weight repacking, workspace, launch sequence, whole-frame render.
//
// Reference: waifu2x/models/cunet.py — UNet1 :31-67, UNet2 :70-121, CUNet :172-203 (layer inventory, crops, the
// cascade z = crop(z1, 20) + unet2(z1)); nunif/utils/seam_blending.py tiled_render :48-106 (frame loop; CUNet has
// blend_size None -> plain overwrite).  State-dict keys are the reference's.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "packed_layers.h"

namespace nunif {
int launch_stitch(const float *tile_out, float *y, const nunif_tile_grid *g, int C, hipStream_t s, int y0 = 0, int rows = -1,
                  int compact = 0);
}

using namespace nunif;

namespace {

struct ConvW : PackedConv { int stride = 1;
               PackedLinear gemm;               // 2x2 stride-2 convs: the same weights in gemm_kernel's [n-tile][k-step] order (K = 4 Cin)
               // 3x3 convs with 128 / 256 inputs and more than 64 outputs (the two bottom convs of unet2): the SAME weights as
               // streams of 64 output channels each, so that every slice runs on the LDS-DMA conv with K halves
               // (conv3_dma_kernel<4, 64, ., 1, 2, KS>), writing its channels of the NHWC map through ConvArgs::ldo
               std::vector<ConvSlice> slice;
               f16 *head_w = nullptr; };        // 64 -> 3 image heads: the tap-scatter form's fragments (cunet_head.hip), row n = 3 tap + c
struct UpW : PackedLinear { int cq = 0; };       // ConvTranspose2d 2x2 s2
struct SEW { float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr; int C = 0; };
struct C3W { float *w = nullptr, *b = nullptr; int C = 0; f16 *frag = nullptr; };   // frag: MFMA A fragments of the fused stem (K = 27 taps + bias)

}  // namespace

struct nunif_cunet : DeviceOwner {
    // kind 0 / 1: CUNet / UpCUNet; 2: waifu2x.vgg_7 (vgg_7.py:6-30: seven 3x3 VALID convs, scale 1, offset 7);
    // 3: waifu2x.upconv_7 (upconv_7.py:6-35: six 3x3 VALID convs + ConvTranspose2d(256, 3, 4, 2, 3), scale 2, offset 14)
    int kind = 0;
    C3W st_first; ConvW st_conv[6]; UpW st_deconv; int st_n = 0;      // the plain conv stacks
    int no_clip = 0;
    int up = 0;                 // 1: UpCUNet (unet1 ends in ConvTranspose2d(64, 3, 4, 2, 3); scale 2, offset 36)
    UpW u1bottom_up;            // that head as a 2x2-window gather GEMM (K = 4*64) with a pixel-shuffle store
    // unet1
    C3W u1c1a; ConvW u1c1b, u1down, u1c2a, u1c2b, u1c3, u1bottom; SEW u1se2; UpW u1up;
    // unet2
    C3W u2c1a; ConvW u2c1b, u2down1, u2c2a, u2c2b, u2down2, u2c3a, u2c3b, u2c4a, u2c4b, u2c5, u2bottom;
    SEW u2se2, u2se3, u2se4; UpW u2up3, u2up4;
    DeviceBuf t[12], z1, sums, scale, tile_out;
    // debug taps (tests only): when on, the map each launch wrote is copied device-side at once (the 12 buffers are reused down the
    // net); the launches themselves are the ones that run with taps off
    struct Tap { std::string name; void *dev; size_t bytes; };
    bool taps_on = false;
    std::vector<Tap> taps;
    void clear_taps() { for (auto &t : taps) (void)hipFree(t.dev); taps.clear(); }
};

namespace {

// Conv2d weight [Cout][Cin][k][k] -> MFMA A fragments in [k-step][n-tile] order, reduction index = tap*Cin + ci
// cin_real < cin: the producer stores its cin_real channels padded with zeros to cin (a multiple of 32)
int make_conv(nunif_cunet *h, const TensorMap &m, const std::string &key, int cin, int cout, int k, int stride, ConvW *c,
              int cin_real = 0) {
    if (cin_real <= 0) cin_real = cin;
    ConvHost host;
    int rc;
    if ((rc = conv_from(h, m, key, cout, 16, cin_real, cin, k, c, true, 0, &host))) return rc;
    c->stride = stride;
    if (k == 3 && stride == 1 && cin_real == cin && (cin == 128 || cin == 256) && cout > 64 && cout % 64 == 0 &&
        (rc = upload_slices(h, host, std::vector<int>(cout / 64, 4), &c->slice)))
        return rc;
    if (k == 3 && stride == 1 && cin_real == 64 && cin == 64 && cout == 3) {
        // tap-scatter head: row n = 3 tap + co over the 64 input channels
        const float *wd = m.at(key + ".weight").data;
        if ((rc = h->upload(pack_nt_ks(27, 32, 64, [=](int n, int ci) { return wd[((size_t)(n % 3) * 64 + ci) * 9 + n / 3]; }),
                            &c->head_w)))
            return rc;
    }
    if (k == 2 && stride == 2 && cin_real == cin && c->N == cout && c->N % 32 == 0) {
        // k = stride: a 2 x 2 gather GEMM (the PatchDown form of gemm_kernel: every input pixel is read exactly once, the token
        // tile's whole K extent sits in registers) instead of the K-looped conv_kernel with its nine-tap machinery
        c->gemm.bias = c->bias; c->gemm.N = c->gemm.n_real = c->N; c->gemm.K = 4 * cin;
        return h->upload(ks_nt_to_nt_ks(host.stream, 4 * cin / 32, c->N / 16), &c->gemm.w);
    }
    return NUNIF_HIP_OK;
}

// ConvTranspose2d(cin, cout, 2, 2) weight [cin][cout][2][2] -> Linear cin -> 4*cout with pixel-shuffle column order
// n = q*cout + co, q = i*2 + j  (gemm_kernel mode 1), fragments in [n-tile][k-step] order
int make_up(nunif_cunet *h, const TensorMap &m, const std::string &key, int cin, int cout, UpW *u) {
    const HostTensor *w, *b;
    int rc;
    if ((rc = find(m, key + ".weight", &w)) || (rc = find(m, key + ".bias", &b))) return rc;
    NUNIF_REQUIRE(w->numel == (int64_t)cin * cout * 4 && b->numel == cout, "%s: unexpected shape", key.c_str());
    const float *wd = w->data, *bd = b->data;
    u->cq = cout;
    return make_linear(h, 4 * cout, 16, cin, [=](int n, int ci) { return wd[((size_t)ci * cout + n % cout) * 4 + n / cout]; },
                       [=](int n) { return bd[n % cout]; }, u);
}

// ConvTranspose2d(cin, cout, 4, 2, 3), weight [cin][cout][4][4]:  out[oy][ox] = b + sum in[iy][ix] W[ky][kx] over
// oy = 2 iy - 3 + ky.  The 2x2 input window (rows j, j+1; cols i, i+1) produces exactly the 2x2 output pixels
// (2j-1 .. 2j) x (2i-1 .. 2i): window row dy contributes to output row parity a through ky = a + 2 (1 - dy) (same for
// columns).  So the head is a gather GEMM over the (H-1)^2 windows, K = (dy*2+dx)*cin + ci (gemm_kernel taps with
// kw = 2), N = co*4 + a*2 + b, stored by gemm_kernel mode 2 with oshift = -1 into the (2H-4)^2 plane.
int make_deconv4(nunif_cunet *h, const TensorMap &m, const std::string &key, int cin, int cout, UpW *u) {
    const HostTensor *w, *b;
    int rc;
    if ((rc = find(m, key + ".weight", &w)) || (rc = find(m, key + ".bias", &b))) return rc;
    NUNIF_REQUIRE(w->numel == (int64_t)cin * cout * 16 && b->numel == cout, "%s: unexpected shape", key.c_str());
    const float *wd = w->data, *bd = b->data;
    u->cq = cout;
    return make_linear(h, 4 * cout, 16, 4 * cin, [=](int n, int k) {
        const int co = n / 4, a = (n >> 1) & 1, bb = n & 1;
        const int tap = k / cin, ci = k % cin, dy = tap >> 1, dx = tap & 1;
        const int ky = a + 2 * (1 - dy), kx = bb + 2 * (1 - dx);
        return wd[(((size_t)ci * cout + co) * 4 + ky) * 4 + kx];
    }, [=](int n) { return bd[n / 4]; }, u);
}

// cout_pad > cout: the extra output channels get zero weights / bias (LeakyReLU(0) = 0), so the next conv sees Cin % 32 == 0
int make_c3(nunif_cunet *h, const TensorMap &m, const std::string &key, int cout, C3W *c, int cout_pad = 0) {
    const HostTensor *w, *b;
    int rc;
    if ((rc = find(m, key + ".weight", &w)) || (rc = find(m, key + ".bias", &b))) return rc;
    NUNIF_REQUIRE(w->numel == (int64_t)cout * 27 && b->numel == cout, "%s: unexpected shape (3 input channels)", key.c_str());
    if (cout_pad <= cout) {
        c->C = cout;
        if (cout % 16 == 0) {
            // the same conv as cout / 16 MFMA A fragments for stem_fused_kernel (swin_stem.hip): row n, k = ci*9 + ky*3 + kx
            // (the weight's own layout), k = 27: the bias (the B operand carries a constant one there), k > 27: zero
            const float *wd = w->data, *bd = b->data;
            if ((rc = h->upload(pack_nt_ks(cout, cout, 32, [=](int n, int k) {
                     return k < 27 ? wd[(size_t)n * 27 + k] : (k == 27 ? bd[n] : 0.0f); }, false, 0), &c->frag)))
                return rc;
        }
        if ((rc = h->upload_f32(w, &c->w))) return rc;
        return h->upload_f32(b, &c->b);
    }
    std::vector<float> wp((size_t)cout_pad * 27, 0.0f), bp(cout_pad, 0.0f);
    std::copy(w->data, w->data + (size_t)cout * 27, wp.begin());
    std::copy(b->data, b->data + cout, bp.begin());
    c->C = cout_pad;
    if ((rc = h->upload(wp, &c->w))) return rc;
    return h->upload(bp, &c->b);
}

int make_se(nunif_cunet *h, const TensorMap &m, const std::string &key, int C, SEW *s) {
    const HostTensor *w1, *b1, *w2, *b2;
    int rc;
    if ((rc = find(m, key + ".conv1.weight", &w1)) || (rc = find(m, key + ".conv1.bias", &b1)) ||
        (rc = find(m, key + ".conv2.weight", &w2)) || (rc = find(m, key + ".conv2.bias", &b2)))
        return rc;
    NUNIF_REQUIRE(w1->numel == (int64_t)C * C / 8 && w2->numel == (int64_t)C * C / 8, "%s: unexpected shape", key.c_str());
    s->C = C;
    if ((rc = h->upload_f32(w1, &s->w1)) || (rc = h->upload_f32(b1, &s->b1)) || (rc = h->upload_f32(w2, &s->w2)) ||
        (rc = h->upload_f32(b2, &s->b2)))
        return rc;
    return NUNIF_HIP_OK;
}

int tap_copy(nunif_cunet *h, const char *name, const void *src, size_t bytes, hipStream_t s) {
    void *p = nullptr;
    NUNIF_HIP_CHECK(hipMalloc(&p, bytes));
    h->taps.push_back({name, p, bytes});
    NUNIF_HIP_CHECK(hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToDevice, s));
    return NUNIF_HIP_OK;
}

// one branch per launch when taps are off
#define CUNET_TAP(name, src, bytes) \
    do { if (h->taps_on) { int trc_ = tap_copy(h, name, src, bytes, s); if (trc_) return trc_; } } while (0)

int run_conv(const ConvW &c, const f16 *a, const f16 *a2, int H2, int crop2, int B, int Hi, f16 *out, float *out32,
             const float *add32, int addH, int add_crop, int clamp01, int act, hipStream_t s) {
    ConvArgs g = conv_args(c, a, B, Hi, Hi, out, c.stride);
    g.a2 = a2; g.H2 = H2; g.W2 = H2; g.crop2 = crop2;
    g.act = act; g.slope = 0.1f;
    g.out32 = out32; g.add32 = add32; g.addH = addH; g.addW = addH; g.add_crop = add_crop;
    g.clamp01 = clamp01;
    if (c.head_w && out32 && !out && !a2 && act == 0) {
        // the 64 -> 3 image heads in tap-scatter form (cunet_head.hip), every launch of that shape
        CunetHeadArgs hg = {a, c.head_w, c.bias, out32, add32, B, Hi, Hi, g.Ho, g.Wo, addH, addH, add_crop, clamp01};
        if (cunet_head_supported(hg)) return launch_cunet_head(hg, s);
    }
    // (every launch of such a conv takes the sliced form or none does: a result must not depend on the tile minibatch)
    static const bool sliced = !(getenv("NUNIF_CUNET_SLICED") && atoi(getenv("NUNIF_CUNET_SLICED")) == 0);
    if (sliced && !c.slice.empty() && out && !out32 && !a2) return launch_conv_sliced(g, c.slice, s);
    return launch_conv(g, s);
}

static inline bool down_gemm_enabled() { const char *e = getenv("NUNIF_CUNET_DOWN_GEMM"); return e ? atoi(e) != 0 : true; }

// Conv2d(k = stride = 2) + LeakyReLU (cunet.py:37,78,81) as a gather GEMM
int run_down(const ConvW &c, const f16 *a, int B, int Hi, f16 *out, hipStream_t s) {
    if (!c.gemm.w || !down_gemm_enabled()) return run_conv(c, a, nullptr, 0, 0, B, Hi, out, nullptr, nullptr, 0, 0, 0, 2, s);
    {   // 64 -> 64: the K-outer prefetching kernel of the swin PatchDown (swin_patchdown.hip), every launch of that shape
        PatchDownArgs p;
        p.a = a; p.w = c.gemm.w; p.bias = c.bias; p.out = out; p.B = B; p.Ho = Hi / 2; p.Wo = Hi / 2; p.Cin = c.Cin; p.oy = 0;
        p.rev = 0; p.N = c.N; p.act = 2; p.slope = 0.1f;
        if (Hi % 2 == 0 && patchdown_supported(p)) return launch_patchdown(p, s);
    }
    GemmArgs g = gemm_map_args(c.gemm, a, B, Hi, Hi, c.Cin, Hi / 2, Hi / 2, out, 2, 2);
    g.act = 2; g.slope = 0.1f;
    return launch_gemm(g, s, "cunet_down");
}

// ConvTranspose2d(k = stride = 2) + LeakyReLU as a pixel-shuffle GEMM; with `skip`: + crop(skip, crop) in the epilogue, so that
// the next conv reads ONE input (`conv3(crop(x1) + x2)`, cunet.py:58-60,111-118 — the add used to ride in that conv's staging,
// which a DMA-staged conv cannot do)
int run_up(const UpW &u, const f16 *a, int B, int Hi, f16 *out, hipStream_t s, const f16 *skip = nullptr, int skip_side = 0,
           int crop = 0, const float *in_scale = nullptr) {
    if (u.K == 64 && u.cq == 64 && skip) {
        // 64 -> 4 x 64 with a cropped skip: the resident-weight prefetching kernel (cunet_up.hip), every launch of that shape.  Its
        // limits on the batch (the SE scale table of at most 128 images in LDS, 32-bit byte offsets into the skip and output maps)
        // are met by running it over groups of images: which kernel runs must not depend on the tile minibatch
        const long skip_img = (long)skip_side * skip_side * 64 * 2, out_img = 4L * Hi * Hi * 64 * 2;
        const long fit = std::min<long>(((1L << 32) - 1) / std::max(skip_img, out_img), in_scale ? 128 : B);
        const int nb = (int)std::max<long>(1, std::min<long>(B, fit));
        CunetUpArgs cu = {a, u.w, u.bias, skip, out, in_scale, nb, Hi, skip_side, crop, 0.1f};
        if (cunet_up_supported(cu)) {
            for (int b0 = 0; b0 < B; b0 += nb) {
                cu.B = std::min(nb, B - b0);
                cu.a = a + (size_t)b0 * Hi * Hi * 64;
                cu.res = skip + (size_t)b0 * skip_side * skip_side * 64;
                cu.out = out + (size_t)b0 * 4 * Hi * Hi * 64;
                cu.in_scale = in_scale ? in_scale + (size_t)b0 * 64 : nullptr;
                int rc = launch_cunet_up(cu, s);
                if (rc) return rc;
            }
            return NUNIF_HIP_OK;
        }
    }
    GemmArgs g = gemm_map_args(u, a, B, Hi, Hi, u.K, Hi, Hi, out);
    g.mode = 1; g.act = 2; g.slope = 0.1f; g.ldo = u.cq;
    if (skip) { g.res = skip; g.res_H = skip_side; g.res_W = skip_side; g.res_crop = crop; }
    g.in_scale = in_scale;                // the squeeze-excitation scale of `a`, applied as the fragments are loaded
    return launch_gemm(g, s, "cunet_up");
}

int run_deconv4(const UpW &u, const f16 *a, int B, int Hi, float *out, int no_clamp, hipStream_t s) {
    GemmArgs g = gemm_map_args(u, a, B, Hi, Hi, u.K / 4, Hi - 1, Hi - 1, out, 1, 2);
    g.mode = 2; g.ldo = 0; g.ps = 2; g.oshift = -1; g.OH = 2 * Hi - 4; g.OW = 2 * Hi - 4; g.no_clamp = no_clamp;
    return launch_gemm(g, s, "upcunet_bottom");
}

// SE blocks whose map has ONE consumer, a transposed-conv GEMM: pooled + MLP here, the channel scale rides in that GEMM's loads
static inline bool se_fuse_enabled() { const char *e = getenv("NUNIF_CUNET_SE_FUSE"); return e ? atoi(e) != 0 : true; }

static inline bool stem_fused_enabled() { const char *e = getenv("NUNIF_CUNET_STEM"); return e ? atoi(e) != 0 : true; }

// first UNetConv of a U-Net through stem_fused_kernel<32, 64, 0>: c3 carries the input geometry (tile / frame mode), c2.stream is
// already in the kernel's [k-step][n-tile] order with k = tap * 32 + ci (make_conv)
int run_stem(const C3ConvArgs &c3, const C3W &c1, const ConvW &c2, f16 *out, hipStream_t s) {
    StemFusedArgs sf;
    memset(&sf, 0, sizeof(sf));
    sf.x = c3.x; sf.frame_mode = c3.frame_mode; sf.H = c3.H; sf.W = c3.W; sf.wb = c3.wb; sf.istep = c3.istep;
    sf.pad_t = c3.pad_t; sf.pad_l = c3.pad_l; sf.tile_begin = c3.tile_begin;
    sf.B = c3.B; sf.T = c3.T; sf.w1 = c1.frag; sf.w2 = c2.stream; sf.b2 = c2.bias; sf.out = out; sf.slope = c3.slope;
    sf.C1 = 32; sf.C = 64; sf.crop = 0;
    return launch_stem_fused(sf, s);
}

// waifu2x.vgg_7 / waifu2x.upconv_7: first conv on the VALU (3 input channels), the 3x3 VALID convs on conv_kernel with
// LeakyReLU(0.1), image head = last conv (fp32 planar, clamp) or the 4x4 s2 p3 ConvTranspose as a gather GEMM.
// x: tile mode [B,3,T,T] or frame + grid; z: [B,3,T-14,T-14] (vgg_7) / [B,3,2T-28,2T-28] (upconv_7)
int forward_stack(nunif_cunet *h, const float *x, const float *frame, const nunif_tile_grid *grid, int tile_begin, float *z,
                  int B, int T, hipStream_t s) {
    NUNIF_REQUIRE(T > 14, "tile_size %d is too small (7 convolutions of 3x3)", T);
    int rc, cmax = 0;
    for (int i = 0; i < h->st_n; ++i) cmax = std::max(cmax, h->st_conv[i].N);
    const size_t bytes = (size_t)B * (T - 2) * (T - 2) * std::max(cmax, h->st_first.C) * sizeof(f16);
    if ((rc = h->t[0].ensure(bytes)) || (rc = h->t[1].ensure(bytes))) return rc;
    f16 *cur = (f16 *)h->t[0].p, *nxt = (f16 *)h->t[1].p;
    C3ConvArgs c3;
    memset(&c3, 0, sizeof(c3));
    if (frame) {
        c3.x = frame; c3.frame_mode = 1; c3.H = grid->x_h; c3.W = grid->x_w; c3.wb = grid->w_blocks;
        c3.istep = grid->input_tile_step; c3.pad_t = grid->pad_t; c3.pad_l = grid->pad_l; c3.tile_begin = tile_begin;
    } else {
        c3.x = x;
    }
    c3.B = B; c3.T = T; c3.w = h->st_first.w; c3.bias = h->st_first.b; c3.C = h->st_first.C; c3.out = cur; c3.slope = 0.1f;
    if ((rc = launch_c3_conv(c3, s))) return rc;
    int side = T - 2;
    CUNET_TAP("net.0", cur, (size_t)B * side * side * h->st_first.C * sizeof(f16));      // (upconv_7: 16 channels padded to 32)
    const int n_mid = h->kind == 2 ? h->st_n - 1 : h->st_n;          // vgg_7: the last conv is the image head
    for (int i = 0; i < n_mid; ++i) {
        if ((rc = run_conv(h->st_conv[i], cur, nullptr, 0, 0, B, side, nxt, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
        std::swap(cur, nxt);
        side -= 2;
        CUNET_TAP(("net." + std::to_string(2 * (i + 1))).c_str(), cur, (size_t)B * side * side * h->st_conv[i].N * sizeof(f16));
    }
    if (h->kind == 2)
        return run_conv(h->st_conv[h->st_n - 1], cur, nullptr, 0, 0, B, side, nullptr, z, nullptr, 0, 0, 1, 0, s);
    return run_deconv4(h->st_deconv, cur, B, side, z, 0, s);
}

// x: tile mode [B,3,T,T] or (frame != NULL) frame + grid; z: [B,3,T-56,T-56] (CUNet) / [B,3,2T-72,2T-72] (UpCUNet)
int forward_impl(nunif_cunet *h, const float *x, const float *frame, const nunif_tile_grid *grid, int tile_begin,
                 float *z, int B, int T, hipStream_t s) {
    if (h->taps_on) h->clear_taps();                // the taps are those of the LAST forward (of a render: of its last minibatch)
    if (h->kind >= 2) return forward_stack(h, x, frame, grid, tile_begin, z, B, T, s);
    NUNIF_REQUIRE(T % 4 == 0 && T >= 64, "tile_size %d is not valid for cunet (multiple of 4, >= 64)", T);
    const size_t b = B;
    const int a1 = T - 2, x1 = T - 4, d1 = x1 / 2, e1 = d1 - 2, f1 = d1 - 4, g1 = 2 * f1, h1 = g1 - 2;
    const int T2 = h->up ? 2 * h1 - 4 : g1 - 4;
    const int a2 = T2 - 2, y1 = T2 - 4, d2 = y1 / 2, e2 = d2 - 2, y2 = d2 - 4, d3 = y2 / 2, e3 = d3 - 2, f3 = d3 - 4;
    const int g3 = 2 * f3, e4 = g3 - 2, f4 = g3 - 4, g4 = 2 * f4, h5 = g4 - 2, To = g4 - 4;
    NUNIF_REQUIRE(g1 == x1 - 8 && g3 == y2 - 8 && g4 == y1 - 32 && To == (h->up ? 2 * T - 72 : T - 56),
                  "internal: cunet geometry");
    auto sz = [&](int side, int ch) { return b * side * side * ch * sizeof(f16); };
    int rc;
    // live-range packing of the fp16 maps onto 12 buffers
    enum { A = 0, X1, D, E, F, G, H, Y1, X2, U3, P, Q };
    if ((rc = h->t[A].ensure(std::max(sz(a1, 32), sz(a2, 32)))) || (rc = h->t[X1].ensure(sz(x1, 64))) ||
        (rc = h->t[D].ensure(std::max({sz(d1, 64), sz(d2, 64), sz(d3, 128)}))) ||
        (rc = h->t[E].ensure(std::max({sz(e1, 128), sz(e2, 64), sz(e3, 256), sz(e4, 64)}))) ||
        (rc = h->t[F].ensure(std::max({sz(f1, 64), sz(f3, 128), sz(f4, 64)}))) ||
        (rc = h->t[G].ensure(std::max({sz(g1, 64), sz(g3, 128), sz(g4, 64)}))) ||
        (rc = h->t[H].ensure(std::max(sz(h1, 64), sz(h5, 64)))) || (rc = h->t[Y1].ensure(sz(y1, 64))) ||
        (rc = h->t[X2].ensure(sz(y2, 128))) || (rc = h->z1.ensure(b * 3 * T2 * T2 * sizeof(float))) ||
        (rc = h->sums.ensure(b * 128 * 256 * sizeof(float))) || (rc = h->scale.ensure(b * 256 * sizeof(float))))
        return rc;
    f16 *tA = (f16 *)h->t[A].p, *tX1 = (f16 *)h->t[X1].p, *tD = (f16 *)h->t[D].p, *tE = (f16 *)h->t[E].p;
    f16 *tF = (f16 *)h->t[F].p, *tG = (f16 *)h->t[G].p, *tH = (f16 *)h->t[H].p, *tY1 = (f16 *)h->t[Y1].p;
    f16 *tX2 = (f16 *)h->t[X2].p;
    float *z1 = (float *)h->z1.p, *sums = (float *)h->sums.p, *scale = (float *)h->scale.p;

    // ---------------- unet1 (cunet.py:52-67) ----------------
    C3ConvArgs c3;
    memset(&c3, 0, sizeof(c3));
    if (frame) {
        c3.x = frame; c3.frame_mode = 1; c3.H = grid->x_h; c3.W = grid->x_w; c3.wb = grid->w_blocks;
        c3.istep = grid->input_tile_step; c3.pad_t = grid->pad_t; c3.pad_l = grid->pad_l; c3.tile_begin = tile_begin;
    } else {
        c3.x = x;
    }
    c3.B = B; c3.T = T; c3.w = h->u1c1a.w; c3.bias = h->u1c1a.b; c3.C = h->u1c1a.C; c3.out = tA; c3.slope = 0.1f;
    // UNetConv(3, 32, 64) as ONE kernel (conv + LeakyReLU + conv + LeakyReLU, the 32-channel map never leaves LDS): the VALU
    // first conv (0.2 ms per launch at 1.3 TB/s, 27 FMAs per output) and the 32 -> 64 conv's read of its 0.27-GB output are gone
    const bool fused_stem = stem_fused_enabled() && h->u1c1a.frag && h->u2c1a.frag && h->u1c1b.Cin == 32 && h->u1c1b.N == 64;
    if (fused_stem) {
        if ((rc = run_stem(c3, h->u1c1a, h->u1c1b, tX1, s))) return rc;                                                // x1
    } else {
        if ((rc = launch_c3_conv(c3, s))) return rc;
        CUNET_TAP("unet1.conv1.0", tA, sz(a1, 32));
        if ((rc = run_conv(h->u1c1b, tA, nullptr, 0, 0, B, a1, tX1, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;   // x1
    }
    CUNET_TAP("unet1.x1", tX1, sz(x1, 64));
    if ((rc = run_down(h->u1down, tX1, B, x1, tD, s))) return rc;
    CUNET_TAP("unet1.down", tD, sz(d1, 64));
    if ((rc = run_conv(h->u1c2a, tD, nullptr, 0, 0, B, d1, tE, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet1.conv2.0", tE, sz(e1, 128));
    if ((rc = run_conv(h->u1c2b, tE, nullptr, 0, 0, B, e1, tF, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet1.conv2", tF, sz(f1, 64));
    const bool sef = se_fuse_enabled();
    if ((rc = launch_se(tF, sums, scale, h->u1se2.w1, h->u1se2.b1, h->u1se2.w2, h->u1se2.b2, B, (long)f1 * f1, 64, s, sef))) return rc;
    CUNET_TAP("unet1.se2.scale", scale, b * 64 * sizeof(float));
    if (!sef) CUNET_TAP("unet1.x2", tF, sz(f1, 64));
    // conv3(crop(x1, 4) + x2): the add happens in the up-GEMM's epilogue
    if ((rc = run_up(h->u1up, tF, B, f1, tG, s, tX1, x1, 4, sef ? scale : nullptr))) return rc;
    CUNET_TAP("unet1.up_add", tG, sz(g1, 64));
    if ((rc = run_conv(h->u1c3, tG, nullptr, 0, 0, B, g1, tH, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet1.x3", tH, sz(h1, 64));
    // conv_bottom -> z1 (clamped unless no_clip, cunet.py:185-186)
    if (h->up) {
        if ((rc = run_deconv4(h->u1bottom_up, tH, B, h1, z1, h->no_clip ? 1 : 0, s))) return rc;
    } else if ((rc = run_conv(h->u1bottom, tH, nullptr, 0, 0, B, h1, nullptr, z1, nullptr, 0, 0, h->no_clip ? 0 : 1, 0, s)))
        return rc;
    CUNET_TAP("z1", z1, b * 3 * T2 * T2 * sizeof(float));

    // ---------------- unet2 (cunet.py:99-121) ----------------
    memset(&c3, 0, sizeof(c3));
    c3.x = z1; c3.B = B; c3.T = T2; c3.w = h->u2c1a.w; c3.bias = h->u2c1a.b; c3.C = h->u2c1a.C; c3.out = tA; c3.slope = 0.1f;
    if (fused_stem) {
        if ((rc = run_stem(c3, h->u2c1a, h->u2c1b, tY1, s))) return rc;                                                // x1
    } else {
        if ((rc = launch_c3_conv(c3, s))) return rc;
        CUNET_TAP("unet2.conv1.0", tA, sz(a2, 32));
        if ((rc = run_conv(h->u2c1b, tA, nullptr, 0, 0, B, a2, tY1, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;   // x1
    }
    CUNET_TAP("unet2.x1", tY1, sz(y1, 64));
    if ((rc = run_down(h->u2down1, tY1, B, y1, tD, s))) return rc;
    CUNET_TAP("unet2.down1", tD, sz(d2, 64));
    if ((rc = run_conv(h->u2c2a, tD, nullptr, 0, 0, B, d2, tE, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet2.conv2.0", tE, sz(e2, 64));
    if ((rc = run_conv(h->u2c2b, tE, nullptr, 0, 0, B, e2, tX2, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;       // x2
    CUNET_TAP("unet2.conv2", tX2, sz(y2, 128));
    if ((rc = launch_se(tX2, sums, scale, h->u2se2.w1, h->u2se2.b1, h->u2se2.w2, h->u2se2.b2, B, (long)y2 * y2, 128, s))) return rc;
    CUNET_TAP("unet2.se2.scale", scale, b * 128 * sizeof(float));
    CUNET_TAP("unet2.x2", tX2, sz(y2, 128));
    if ((rc = run_down(h->u2down2, tX2, B, y2, tD, s))) return rc;
    CUNET_TAP("unet2.down2", tD, sz(d3, 128));
    if ((rc = run_conv(h->u2c3a, tD, nullptr, 0, 0, B, d3, tE, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet2.conv3.0", tE, sz(e3, 256));
    if ((rc = run_conv(h->u2c3b, tE, nullptr, 0, 0, B, e3, tF, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet2.conv3", tF, sz(f3, 128));
    if ((rc = launch_se(tF, sums, scale, h->u2se3.w1, h->u2se3.b1, h->u2se3.w2, h->u2se3.b2, B, (long)f3 * f3, 128, s, sef))) return rc;
    CUNET_TAP("unet2.se3.scale", scale, b * 128 * sizeof(float));
    if (!sef) CUNET_TAP("unet2.x3", tF, sz(f3, 128));
    // conv4(crop(x2, 4) + x3)
    if ((rc = run_up(h->u2up3, tF, B, f3, tG, s, tX2, y2, 4, sef ? scale : nullptr))) return rc;
    CUNET_TAP("unet2.up3_add", tG, sz(g3, 128));
    if ((rc = run_conv(h->u2c4a, tG, nullptr, 0, 0, B, g3, tE, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet2.conv4.0", tE, sz(e4, 64));
    if ((rc = run_conv(h->u2c4b, tE, nullptr, 0, 0, B, e4, tF, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet2.conv4", tF, sz(f4, 64));
    if ((rc = launch_se(tF, sums, scale, h->u2se4.w1, h->u2se4.b1, h->u2se4.w2, h->u2se4.b2, B, (long)f4 * f4, 64, s, sef))) return rc;
    CUNET_TAP("unet2.se4.scale", scale, b * 64 * sizeof(float));
    if (!sef) CUNET_TAP("unet2.x4", tF, sz(f4, 64));
    // conv5(crop(x1, 16) + x4)
    if ((rc = run_up(h->u2up4, tF, B, f4, tG, s, tY1, y1, 16, sef ? scale : nullptr))) return rc;
    CUNET_TAP("unet2.up4_add", tG, sz(g4, 64));
    if ((rc = run_conv(h->u2c5, tG, nullptr, 0, 0, B, g4, tH, nullptr, nullptr, 0, 0, 0, 2, s))) return rc;
    CUNET_TAP("unet2.x5", tH, sz(h5, 64));
    // z = clamp(crop(z1, 20) + conv_bottom(x5), 0, 1)
    if ((rc = run_conv(h->u2bottom, tH, nullptr, 0, 0, B, h5, nullptr, z, z1, T2, 20, 1, 0, s))) return rc;
    return NUNIF_HIP_OK;
}

}  // namespace

extern "C" int nunif_hip_cunet_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t no_clip,
                                      nunif_cunet **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "cunet_create: NULL argument");
    TensorMap m = tensor_map(tensors, n_tensors);
    nunif_cunet *h = new nunif_cunet();
    h->no_clip = no_clip;
    int rc = NUNIF_HIP_OK;
    do {
        const HostTensor *bw;
        if (m.count("net.12.weight")) {                  // nn.Sequential key layout of vgg_7 / upconv_7
            bw = &m["net.12.weight"];
            const bool upconv = bw->shape.size() == 4 && bw->shape[2] == 4;
            h->kind = upconv ? 3 : 2;
            static const int vgg_c[8] = {3, 32, 32, 64, 64, 128, 128, 3}, up_c[7] = {3, 16, 32, 64, 128, 128, 256};
            const int *ch = upconv ? up_c : vgg_c;
            const int first_pad = (ch[1] + 31) / 32 * 32;
            if ((rc = make_c3(h, m, "net.0", ch[1], &h->st_first, first_pad))) break;
            h->st_n = upconv ? 5 : 6;
            for (int i = 0; i < h->st_n && !rc; ++i) {
                const int cin = i == 0 ? first_pad : ch[i + 1];
                rc = make_conv(h, m, "net." + std::to_string(2 * (i + 1)), cin, ch[i + 2], 3, 1, &h->st_conv[i], ch[i + 1]);
            }
            if (rc) break;
            if (upconv && (rc = make_deconv4(h, m, "net.12", 256, 3, &h->st_deconv))) break;
            break;
        }
        if ((rc = find(m, "unet1.conv_bottom.weight", &bw))) break;
        h->up = (bw->shape.size() == 4 && bw->shape[2] == 4) ? 1 : 0;
        h->kind = h->up;
        const std::string a = "unet1.", b = "unet2.";
        if ((rc = make_c3(h, m, a + "conv1.conv.0", 32, &h->u1c1a))) break;
        if ((rc = make_conv(h, m, a + "conv1.conv.2", 32, 64, 3, 1, &h->u1c1b))) break;
        if ((rc = make_conv(h, m, a + "conv1_down", 64, 64, 2, 2, &h->u1down))) break;
        if ((rc = make_conv(h, m, a + "conv2.conv.0", 64, 128, 3, 1, &h->u1c2a))) break;
        if ((rc = make_conv(h, m, a + "conv2.conv.2", 128, 64, 3, 1, &h->u1c2b))) break;
        if ((rc = make_se(h, m, a + "conv2.seblock", 64, &h->u1se2))) break;
        if ((rc = make_up(h, m, a + "conv2_up", 64, 64, &h->u1up))) break;
        if ((rc = make_conv(h, m, a + "conv3", 64, 64, 3, 1, &h->u1c3))) break;
        if (h->up) {
            if ((rc = make_deconv4(h, m, a + "conv_bottom", 64, 3, &h->u1bottom_up))) break;
        } else if ((rc = make_conv(h, m, a + "conv_bottom", 64, 3, 3, 1, &h->u1bottom))) break;
        if ((rc = make_c3(h, m, b + "conv1.conv.0", 32, &h->u2c1a))) break;
        if ((rc = make_conv(h, m, b + "conv1.conv.2", 32, 64, 3, 1, &h->u2c1b))) break;
        if ((rc = make_conv(h, m, b + "conv1_down", 64, 64, 2, 2, &h->u2down1))) break;
        if ((rc = make_conv(h, m, b + "conv2.conv.0", 64, 64, 3, 1, &h->u2c2a))) break;
        if ((rc = make_conv(h, m, b + "conv2.conv.2", 64, 128, 3, 1, &h->u2c2b))) break;
        if ((rc = make_se(h, m, b + "conv2.seblock", 128, &h->u2se2))) break;
        if ((rc = make_conv(h, m, b + "conv2_down", 128, 128, 2, 2, &h->u2down2))) break;
        if ((rc = make_conv(h, m, b + "conv3.conv.0", 128, 256, 3, 1, &h->u2c3a))) break;
        if ((rc = make_conv(h, m, b + "conv3.conv.2", 256, 128, 3, 1, &h->u2c3b))) break;
        if ((rc = make_se(h, m, b + "conv3.seblock", 128, &h->u2se3))) break;
        if ((rc = make_up(h, m, b + "conv3_up", 128, 128, &h->u2up3))) break;
        if ((rc = make_conv(h, m, b + "conv4.conv.0", 128, 64, 3, 1, &h->u2c4a))) break;
        if ((rc = make_conv(h, m, b + "conv4.conv.2", 64, 64, 3, 1, &h->u2c4b))) break;
        if ((rc = make_se(h, m, b + "conv4.seblock", 64, &h->u2se4))) break;
        if ((rc = make_up(h, m, b + "conv4_up", 64, 64, &h->u2up4))) break;
        if ((rc = make_conv(h, m, b + "conv5", 64, 64, 3, 1, &h->u2c5))) break;
        if ((rc = make_conv(h, m, b + "conv_bottom", 64, 3, 3, 1, &h->u2bottom))) break;
    } while (0);
    if (rc) { nunif_hip_cunet_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_cunet_debug_taps(nunif_cunet *h, int32_t enable) {
    NUNIF_REQUIRE(h, "debug_taps: NULL handle");
    h->clear_taps();
    h->taps_on = enable != 0;
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_cunet_get_tap(nunif_cunet *h, int32_t index, char *name, int32_t name_cap, void *host_dst,
                                       int64_t cap_bytes, int64_t *nbytes) {
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

extern "C" void nunif_hip_cunet_destroy(nunif_cunet *h) {
    if (!h) return;
    h->clear_taps();
    h->free_all();
    for (auto &b : h->t) b.release();
    h->z1.release(); h->sums.release(); h->scale.release(); h->tile_out.release();
    delete h;
}

extern "C" int nunif_hip_cunet_forward(nunif_cunet *h, const float *x, float *z, int32_t batch, int32_t tile_size,
                                       void *stream) {
    NUNIF_REQUIRE(h && x && z && batch > 0, "cunet_forward: bad argument");
    return forward_impl(h, x, nullptr, nullptr, 0, z, batch, tile_size, (hipStream_t)stream);
}

extern "C" int nunif_hip_cunet_render(nunif_cunet *h, const float *x, float *y, int32_t x_h, int32_t x_w,
                                      int32_t tile_size, int32_t batch_size, void *stream) {
    NUNIF_REQUIRE(h && x && y && batch_size > 0, "cunet_render: bad argument");
    nunif_tile_grid g;
    // CUNet: scale 1, offset 28; UpCUNet: scale 2, offset 36 (cunet.py:143,177); vgg_7: 1, 7; upconv_7: 2, 14;
    // blend_size None -> plain overwrite
    static const int kScale[4] = {1, 2, 1, 2}, kOffset[4] = {28, 36, 7, 14};
    int rc = nunif_hip_tile_grid_init(x_h, x_w, kScale[h->kind], kOffset[h->kind], tile_size, 0, &g);
    if (rc) return rc;
    const int n_tiles = g.h_blocks * g.w_blocks;
    const size_t To = g.out_tile_size;
    if ((rc = h->tile_out.ensure((size_t)n_tiles * 3 * To * To * sizeof(float)))) return rc;
    float *tile_out = (float *)h->tile_out.p;
    hipStream_t st = (hipStream_t)stream;
    for (int t0 = 0; t0 < n_tiles; t0 += batch_size) {
        const int nb = std::min(batch_size, n_tiles - t0);
        if ((rc = forward_impl(h, nullptr, x, &g, t0, tile_out + (size_t)t0 * 3 * To * To, nb, tile_size, st))) return rc;
    }
    return launch_stitch(tile_out, y, &g, 3, st);
}
