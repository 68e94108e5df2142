// ZoeDepth metric-bins head over the Depth-Anything V1 core (`--depth-model ZoeD_Any_N / ZoeD_Any_K`) on gfx950 — what
// iw3/zoedepth_model.py:23-27 `_forward` obtains as `model(x)['metric_depth']` from the torch.hub net, and its `torch.nan_to_num`.
// The network is NOT in the reference tree: this follows the published architecture (ZoeDepth `bin_centers_type = "softplus"`:
// un-normed attractors, conditional log-binomial) in the key layout of HuggingFace transformers'
// ZoeDepthMetricDepthEstimationHead, against which tests/zoedepth_ref.py is pinned in float64.
//
// Inputs are the six maps DepthAnythingCore hands over (depth_anything.hip `nunif_hip_depth_anything_forward_features`): the
// 32-channel activation behind output_conv2's first conv + ReLU, layer4_rn, the refinenet outputs r4 .. r1 (all NHWC fp16) and
// the relative depth (fp32).  Everything per pixel:
//   1x1 convs 256 -> 256 / 128 and 128 -> 128        gemm_kernel (swin_kernels.hip), fp16 maps, fp32 accumulation
//   zoe_seed_kernel        seed_bin_regressor.conv2 (256 -> 64) + Softplus -> fp32 bin centres
//   zoe_addup_kernel       bin embedding + bilinear(align_corners=True) of the previous stage's embedding
//   zoe_attractor_kernel   one wave per pixel, lane = bin: attractor conv2 (128 -> 16 / 8 / 4 / 1) + Softplus, the previous centres
//                          upsampled (align_corners=True), dc = mean_a dx / (1 + alpha dx^2); writes the new centres only
//   zoe_final_kernel       one thread per output pixel: [32-channel activation | relative depth | upsampled embedding] -> 80 (GELU)
//                          -> 4 (Softplus), the two linear norms, the temperature, the log-binomial over 64 bins, its softmax and the
//                          expectation against the upsampled centres, nan_to_num.  The B x 64 x H x W volume exists in registers only.
//                          The embedding's share of the 161 -> 80 conv is linear and a bilinear resize's weights sum to 1, so it is
//                          taken BEFORE the resize (a 128 -> 80 GEMM, bias included, on the 8x-grid map) and resized as 80 channels.
//   zoe_prep_kernel        batch_preprocess's tail (iw3/zoedepth_model.py:66-83): reflection_pad2d_loop + clamp(0, 1) + (x - 0.5) / 0.5
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "packed_layers.h"

namespace nunif {

constexpr int kZBins = 64, kZEmb = 128, kZHid = 80, kZHidP = 96, kZRel = 33;   // 32 activation channels + the relative depth

__device__ __forceinline__ float zoe_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }      // nn.Softplus (beta 1, threshold 20)

// F.interpolate(bilinear, align_corners=True): source taps and weights of output coordinate (Y, X)
struct ZoeTap { int y0, y1, x0, x1; float ly, lx; };
__device__ __forceinline__ ZoeTap zoe_tap(int Y, int X, int Hi, int Wi, int Ho, int Wo) {
    const float ry = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, rx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
    const float sy = ry * (float)Y, sx = rx * (float)X;
    ZoeTap t;
    t.y0 = min((int)sy, Hi - 1); t.x0 = min((int)sx, Wi - 1);
    t.y1 = t.y0 + (t.y0 < Hi - 1 ? 1 : 0); t.x1 = t.x0 + (t.x0 < Wi - 1 ? 1 : 0);
    t.ly = sy - (float)t.y0; t.lx = sx - (float)t.x0;
    return t;
}
__device__ __forceinline__ float zoe_mix(const ZoeTap &t, float a, float b, float c, float d) {
    return (1.f - t.ly) * ((1.f - t.lx) * a + t.lx * b) + t.ly * ((1.f - t.lx) * c + t.lx * d);
}

// centres[p][bin] = softplus(b[bin] + sum_k w[bin][k] x[p][k]); x: [P][K] fp16
__global__ void __launch_bounds__(256) zoe_seed_kernel(const f16 *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b,
                                                       float *__restrict__ centres, long P, int K) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= P * kZBins) return;
    const int bin = (int)(id % kZBins);
    const long p = id / kZBins;
    float acc = b[bin];
    for (int k = 0; k < K; ++k) acc = fmaf((float)x[p * K + k], w[(long)bin * K + k], acc);
    centres[id] = zoe_softplus(acc);
}

// y = fp16(emb + bilinear(prev)); emb, y: [B,H,W,128], prev: [B,Hp,Wp,128]; one thread = 8 channels of one pixel
__global__ void __launch_bounds__(256) zoe_addup_kernel(const f16 *__restrict__ emb, const f16 *__restrict__ prev, f16 *__restrict__ y,
                                                        int B, int H, int W, int Hp, int Wp) {
    constexpr int cq = kZEmb / 8;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long)B * H * W * cq) return;
    const int c8 = (int)(id % cq);
    long t = id / cq;
    const int X = (int)(t % W); t /= W;
    const int Y = (int)(t % H), b = (int)(t / H);
    const ZoeTap tp = zoe_tap(Y, X, Hp, Wp, H, W);
    auto ld = [&](int yy, int xx) { return *reinterpret_cast<const f16x8 *>(prev + (((long)b * Hp + yy) * Wp + xx) * kZEmb + c8 * 8); };
    const f16x8 a = ld(tp.y0, tp.x0), bq = ld(tp.y0, tp.x1), c = ld(tp.y1, tp.x0), d = ld(tp.y1, tp.x1);
    const f16x8 e = *reinterpret_cast<const f16x8 *>(emb + id * 8);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)((float)e[j] + zoe_mix(tp, (float)a[j], (float)bq[j], (float)c[j], (float)d[j]));
    *reinterpret_cast<f16x8 *>(y + id * 8) = o;
}

// ZoeDepth AttractorLayerUnnormed behind its conv1 + ReLU.  a1: [B,H,W,128] fp16; w2: [NA][128], b2: [NA]; cprev: [B,Hp,Wp,64]
// fp32; cout: [B,H,W,64] fp32.  One wave per pixel, lane = bin; the 128-long dot products are split over the lanes.
__global__ void __launch_bounds__(256) zoe_attractor_kernel(const f16 *__restrict__ a1, const float *__restrict__ w2,
                                                            const float *__restrict__ b2, const float *__restrict__ cprev,
                                                            float *__restrict__ cout, int B, int H, int W, int Hp, int Wp, int NA,
                                                            float alpha) {
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (long)B * H * W) return;                       // wave-uniform
    const int lane = threadIdx.x & 63;
    const int X = (int)(pix % W);
    const long t = pix / W;
    const int Y = (int)(t % H), b = (int)(t / H);
    const ZoeTap tp = zoe_tap(Y, X, Hp, Wp, H, W);
    auto ld = [&](int yy, int xx) { return cprev[(((long)b * Hp + yy) * Wp + xx) * kZBins + lane]; };
    const float c = zoe_mix(tp, ld(tp.y0, tp.x0), ld(tp.y0, tp.x1), ld(tp.y1, tp.x0), ld(tp.y1, tp.x1));
    const float x0 = (float)a1[pix * kZEmb + lane], x1 = (float)a1[pix * kZEmb + 64 + lane];
    float dc = 0.f;
    for (int a = 0; a < NA; ++a) {
        float s = fmaf(x0, w2[a * kZEmb + lane], x1 * w2[a * kZEmb + 64 + lane]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float dx = zoe_softplus(s + b2[a]) - c;
        dc += dx / (1.f + alpha * dx * dx);                  // inv_attractor, gamma = 2
    }
    cout[pix * kZBins + lane] = c + dc / (float)NA;            // attractor_kind "mean"
}

struct ZoeFinalArgs {
    const f16 *act;       // [B,H,W,32]
    const float *rel;     // [B,H,W]
    const f16 *e80;       // [B,Hp,Wp,96]: mlp.0's embedding columns (+ bias) on the last stage's grid
    const float *centres; // [B,Hp,Wp,64]
    const float *w1;      // [80][33]: mlp.0's columns for the activation and the relative depth
    const float *w2;      // [4][80] then b2[4]
    const float *logbinom;// [64]
    float *out;           // [B,H,W]
    int B, H, W, Hp, Wp;
    float min_temp, max_temp;
};

__global__ void __launch_bounds__(256) zoe_final_kernel(ZoeFinalArgs g) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long)g.B * g.H * g.W) return;
    const int X = (int)(id % g.W);
    const long t = id / g.W;
    const int Y = (int)(t % g.H), b = (int)(t / g.H);
    const ZoeTap tp = zoe_tap(Y, X, g.Hp, g.Wp, g.H, g.W);
    const long p00 = ((long)b * g.Hp + tp.y0) * g.Wp + tp.x0, p01 = ((long)b * g.Hp + tp.y0) * g.Wp + tp.x1;
    const long p10 = ((long)b * g.Hp + tp.y1) * g.Wp + tp.x0, p11 = ((long)b * g.Hp + tp.y1) * g.Wp + tp.x1;
    float in[kZRel];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f16x8 v = *reinterpret_cast<const f16x8 *>(g.act + id * 32 + q * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) in[q * 8 + j] = (float)v[j];
    }
    in[32] = g.rel[id];                      // (the relative depth has the activation's size: its align_corners resize is the identity)
    float o4[4] = {g.w2[4 * kZHid + 0], g.w2[4 * kZHid + 1], g.w2[4 * kZHid + 2], g.w2[4 * kZHid + 3]};
#pragma unroll 1
    for (int jb = 0; jb < kZHid / 8; ++jb) {
        const f16x8 ea = *reinterpret_cast<const f16x8 *>(g.e80 + p00 * kZHidP + jb * 8), eb = *reinterpret_cast<const f16x8 *>(g.e80 + p01 * kZHidP + jb * 8);
        const f16x8 ec = *reinterpret_cast<const f16x8 *>(g.e80 + p10 * kZHidP + jb * 8), ed = *reinterpret_cast<const f16x8 *>(g.e80 + p11 * kZHidP + jb * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int hj = jb * 8 + j;
            float acc = zoe_mix(tp, (float)ea[j], (float)eb[j], (float)ec[j], (float)ed[j]);
            const float *wr = g.w1 + hj * kZRel;
#pragma unroll
            for (int k = 0; k < kZRel; ++k) acc = fmaf(in[k], wr[k], acc);
            const float ge = 0.5f * acc * (1.f + erff(acc * 0.70710678118654752f));        // nn.GELU (erf)
#pragma unroll
            for (int c = 0; c < 4; ++c) o4[c] = fmaf(ge, g.w2[c * kZHid + hj], o4[c]);
        }
    }
    const float eps = 1e-4f;
    const float pa = zoe_softplus(o4[0]) + eps, pb = zoe_softplus(o4[1]) + eps, ta = zoe_softplus(o4[2]) + eps, tb = zoe_softplus(o4[3]) + eps;
    const float prob = pa / (pa + pb);
    const float temp = (g.max_temp - g.min_temp) * (ta / (ta + tb)) + g.min_temp;
    const float lp = logf(fminf(fmaxf(prob, eps), 1.f)), lq = logf(fminf(fmaxf(1.f - prob, eps), 1.f));
    const float inv_t = 1.f / temp;
    float mx = -FLT_MAX;
    for (int k = 0; k < kZBins; ++k) mx = fmaxf(mx, (g.logbinom[k] + (float)k * lp + (float)(kZBins - 1 - k) * lq) * inv_t);
    float num = 0.f, den = 0.f;
#pragma unroll 1
    for (int kb = 0; kb < kZBins / 4; ++kb) {
        const float4 ca = *reinterpret_cast<const float4 *>(g.centres + p00 * kZBins + kb * 4), cb = *reinterpret_cast<const float4 *>(g.centres + p01 * kZBins + kb * 4);
        const float4 cc = *reinterpret_cast<const float4 *>(g.centres + p10 * kZBins + kb * 4), cd = *reinterpret_cast<const float4 *>(g.centres + p11 * kZBins + kb * 4);
        const float cen[4] = {zoe_mix(tp, ca.x, cb.x, cc.x, cd.x), zoe_mix(tp, ca.y, cb.y, cc.y, cd.y), zoe_mix(tp, ca.z, cb.z, cc.z, cd.z),
                              zoe_mix(tp, ca.w, cb.w, cc.w, cd.w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kb * 4 + j;
            const float e = expf((g.logbinom[k] + (float)k * lp + (float)(kZBins - 1 - k) * lq) * inv_t - mx);
            den += e;
            num = fmaf(e, cen[j], num);
        }
    }
    float r = num / den;
    // torch.nan_to_num (iw3/zoedepth_model.py:26)
    if (r != r) r = 0.f;
    else if (r > FLT_MAX) r = FLT_MAX;
    else if (r < -FLT_MAX) r = -FLT_MAX;
    g.out[id] = r;
}

// reflection_pad2d_loop (nunif/modules/reflection_pad2d.py:49-68) pads in steps of at most size - 1 per side, each step
// reflecting about the edges of the map as the steps before left it.  An output coordinate walks the steps backwards.
constexpr int kZPadSteps = 8;
struct ZoePadAxis { int n, lo[kZPadSteps], size[kZPadSteps]; };          // step s pads `lo[s]` in front of a map of `size[s]`
__device__ __forceinline__ int zoe_unpad(const ZoePadAxis &a, int i) {
    for (int s = a.n - 1; s >= 0; --s) {
        i -= a.lo[s];
        if (i < 0) i = -i;
        else if (i >= a.size[s]) i = 2 * (a.size[s] - 1) - i;
    }
    return i;
}
// x: [planes,h,w] -> y: [planes,H,W] = (clamp(pad(x), 0, 1) - 0.5) / 0.5
__global__ void __launch_bounds__(256) zoe_prep_kernel(const float *__restrict__ x, float *__restrict__ y, long planes, int h, int w,
                                                       int H, int W, ZoePadAxis ay, ZoePadAxis ax) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= planes * H * W) return;
    const int X = (int)(id % W);
    const long t = id / W;
    const int Y = (int)(t % H);
    const long pl = t / H;
    const int sy = min(max(zoe_unpad(ay, Y), 0), h - 1), sx = min(max(zoe_unpad(ax, X), 0), w - 1);
    const float v = fminf(fmaxf(x[(pl * h + sy) * w + sx], 0.f), 1.f);
    y[id] = (v - 0.5f) / 0.5f;
}

}  // namespace nunif

using namespace nunif;

namespace {
// the steps of reflection_pad2d_loop along one axis; false when more than kZPadSteps are needed
bool pad_axis(int size, int lo, int hi, ZoePadAxis *a) {
    const int base = size;
    a->n = 0;
    while (lo != 0 || hi != 0) {
        if (a->n == kZPadSteps || base < 2) return false;
        const int l = std::min(lo, base - 1), r = std::min(hi, base - 1);
        a->lo[a->n] = l; a->size[a->n] = size; ++a->n;
        size += l + r; lo -= l; hi -= r;
    }
    return true;
}
}  // namespace

struct nunif_zoedepth_head : DeviceOwner {
    int F = 256, n_attr[4] = {16, 8, 4, 1};
    float alpha = 1000.f, min_temp = 0.0212f, max_temp = 50.f;
    PackedLinear conv2, seed1, sproj1, sproj2, proj1[4], proj2[4], att1[4], e80;
    float *seed_w = nullptr, *seed_b = nullptr, *att_w[4] = {}, *att_b[4] = {}, *w1 = nullptr, *w2 = nullptr, *logbinom = nullptr;
    DeviceBuf x0, s1, t128, emb[2], xa, a1, cen[5], e80buf;
    int tap_h[5] = {}, tap_w[5] = {}, tap_b = 0;
};

namespace {
// a 1x1 conv as a token Linear; the output rows are N wide, padding included (e80: 80 of 96)
int zrun(const PackedLinear &L, const f16 *a, long M, int relu, f16 *out, hipStream_t s, const char *tag) {
    GemmArgs g = gemm_token_args(L, a, M, out);
    g.act = relu ? 2 : 0; g.ldo = L.N; g.n_real = L.N;
    return launch_gemm(g, s, tag);
}
unsigned zblocks(long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// Replaces the metric-bins head of the torch.hub net behind iw3/zoedepth_model.py:23-27 `_forward` (ZoeD_Any_N / ZoeD_Any_K).
// Tensors under HuggingFace's ZoeDepthMetricDepthEstimationHead names (conv2, seed_bin_regressor.conv1/2, seed_projector.conv1/2,
// projectors.N.conv1/2, attractors.N.conv1/2, conditional_log_binomial.mlp.0/2).
extern "C" int nunif_hip_zoedepth_head_create(const nunif_tensor_desc *tensors, int32_t n_tensors, float alpha, float min_temp,
                                              float max_temp, nunif_zoedepth_head **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "zoedepth_head_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_zoedepth_head *h = new nunif_zoedepth_head();
    h->alpha = alpha; h->min_temp = min_temp; h->max_temp = max_temp;
    int rc = NUNIF_HIP_OK;
    do {
        const HostTensor *w, *b;
        if ((rc = find(m, "conv2.bias", &b))) break;
        const int F = (int)b->numel;
        if (F != 256) { set_error("zoedepth_head: bottleneck width %d unsupported (256)", F); rc = NUNIF_HIP_EUNSUPPORTED; break; }
        h->F = F;
        if ((rc = linear_from(h, m, "conv2", F, F, 32, &h->conv2)) || (rc = linear_from(h, m, "seed_bin_regressor.conv1", 256, F, 32, &h->seed1)) ||
            (rc = linear_from(h, m, "seed_projector.conv1", kZEmb, F, 32, &h->sproj1)) ||
            (rc = linear_from(h, m, "seed_projector.conv2", kZEmb, kZEmb, 32, &h->sproj2)))
            break;
        if ((rc = find(m, "seed_bin_regressor.conv2.weight", &w)) || (rc = find(m, "seed_bin_regressor.conv2.bias", &b))) break;
        if (w->numel != (int64_t)kZBins * 256 || b->numel != kZBins) { set_error("zoedepth_head: 64 bins expected"); rc = NUNIF_HIP_EUNSUPPORTED; break; }
        if ((rc = h->upload_f32(w, &h->seed_w)) || (rc = h->upload_f32(b, &h->seed_b))) break;
        for (int i = 0; i < 4 && !rc; ++i) {
            const std::string p = "projectors." + std::to_string(i), a = "attractors." + std::to_string(i);
            if ((rc = linear_from(h, m, p + ".conv1", kZEmb, F, 32, &h->proj1[i])) ||
                (rc = linear_from(h, m, p + ".conv2", kZEmb, kZEmb, 32, &h->proj2[i])) ||
                (rc = linear_from(h, m, a + ".conv1", kZEmb, kZEmb, 32, &h->att1[i])))
                break;
            if ((rc = find(m, a + ".conv2.weight", &w)) || (rc = find(m, a + ".conv2.bias", &b))) break;
            const int na = (int)b->numel;
            if (na < 1 || na > 64 || w->numel != (int64_t)na * kZEmb) { set_error("%s.conv2: unexpected shape", a.c_str()); rc = NUNIF_HIP_EINVAL; break; }
            h->n_attr[i] = na;
            if ((rc = h->upload_f32(w, &h->att_w[i])) || (rc = h->upload_f32(b, &h->att_b[i]))) break;
        }
        if (rc) break;
        const std::string c = "conditional_log_binomial.mlp.";
        if ((rc = linear_from(h, m, c + "0", kZHid, kZEmb, 32, &h->e80, false, nullptr, kZRel, kZRel + kZEmb))) break;
        const HostTensor *w2, *b2;
        if ((rc = find(m, c + "0.weight", &w)) || (rc = find(m, c + "2.weight", &w2)) || (rc = find(m, c + "2.bias", &b2))) break;
        if (w2->numel != 4 * kZHid || b2->numel != 4) { set_error("%s2: unexpected shape", c.c_str()); rc = NUNIF_HIP_EINVAL; break; }
        std::vector<float> w1((size_t)kZHid * kZRel), wo(4 * kZHid + 4), lb(kZBins);
        for (int j = 0; j < kZHid; ++j)
            for (int k = 0; k < kZRel; ++k) w1[(size_t)j * kZRel + k] = w->data[(size_t)j * (kZRel + kZEmb) + k];
        for (int i = 0; i < 4 * kZHid; ++i) wo[i] = w2->data[i];
        for (int i = 0; i < 4; ++i) wo[4 * kZHid + i] = b2->data[i];
        for (int k = 0; k < kZBins; ++k) {            // log_binom(n = 63, k), Stirling form with the published eps
            const double e = 1e-7, n = (kZBins - 1) + e, kk = k + e;
            lb[k] = (float)(n * std::log(n) - kk * std::log(kk) - (n - kk) * std::log(n - kk + e));
        }
        if ((rc = h->upload(w1, &h->w1)) || (rc = h->upload(wo, &h->w2)) || (rc = h->upload(lb, &h->logbinom))) break;
    } while (0);
    if (rc) { nunif_hip_zoedepth_head_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_zoedepth_head_destroy(nunif_zoedepth_head *h) {
    if (!h) return;
    h->free_all();
    for (DeviceBuf *b : {&h->x0, &h->s1, &h->t128, &h->emb[0], &h->emb[1], &h->xa, &h->a1, &h->e80buf}) b->release();
    for (DeviceBuf &b : h->cen) b.release();
    delete h;
}

// f: the six maps of nunif_hip_depth_anything_forward_features; rel: [B,H,W] f32 (the relative depth, H x W = the activation's
// size); out: [B,H,W] f32 = nan_to_num(metric_depth)
extern "C" int nunif_hip_zoedepth_head_forward(nunif_zoedepth_head *h, const nunif_da_features *f, const float *rel, float *out,
                                               int32_t B, int32_t H, int32_t W, void *stream) {
    NUNIF_REQUIRE(h && f && rel && out && B > 0 && H > 0 && W > 0, "zoedepth_head_forward: bad argument");
    NUNIF_REQUIRE(f->channels == h->F && f->outconv && f->bottleneck && f->bh > 0 && f->bw > 0, "zoedepth_head_forward: %d-channel maps expected", h->F);
    for (int i = 0; i < 4; ++i) NUNIF_REQUIRE(f->blocks[i] && f->rh[i] > 0 && f->rw[i] > 0, "zoedepth_head_forward: feature block %d missing", i);
    hipStream_t s = (hipStream_t)stream;
    const size_t e2 = sizeof(f16);
    const long P0 = (long)B * f->bh * f->bw;
    long Pmax = P0;
    for (int i = 0; i < 4; ++i) Pmax = std::max(Pmax, (long)B * f->rh[i] * f->rw[i]);
    int rc;
    if ((rc = h->x0.ensure(P0 * h->F * e2)) || (rc = h->s1.ensure(P0 * 256 * e2)) || (rc = h->t128.ensure(Pmax * kZEmb * e2)) ||
        (rc = h->emb[0].ensure(Pmax * kZEmb * e2)) || (rc = h->emb[1].ensure(Pmax * kZEmb * e2)) || (rc = h->xa.ensure(Pmax * kZEmb * e2)) ||
        (rc = h->a1.ensure(Pmax * kZEmb * e2)) || (rc = h->e80buf.ensure((size_t)B * f->rh[3] * f->rw[3] * kZHidP * e2)) ||
        (rc = h->cen[0].ensure(P0 * kZBins * sizeof(float))))
        return rc;
    for (int i = 0; i < 4; ++i)
        if ((rc = h->cen[i + 1].ensure((size_t)B * f->rh[i] * f->rw[i] * kZBins * sizeof(float)))) return rc;
    f16 *x0 = (f16 *)h->x0.p, *s1 = (f16 *)h->s1.p, *t128 = (f16 *)h->t128.p, *xa = (f16 *)h->xa.p, *a1 = (f16 *)h->a1.p;
    // seed: x = conv2(bottleneck); centres = softplus(regressor(x)); embedding = seed_projector(x)
    if ((rc = zrun(h->conv2, (const f16 *)f->bottleneck, P0, 0, x0, s, "zoe_conv2")) || (rc = zrun(h->seed1, x0, P0, 1, s1, s, "zoe_seed1"))) return rc;
    {
        ProfScope ps("zoe_seed_kernel", s, 2.0 * P0 * kZBins * 256, (double)P0 * (256 * 2.0 + kZBins * 4.0));
        zoe_seed_kernel<<<zblocks(P0 * kZBins), 256, 0, s>>>(s1, h->seed_w, h->seed_b, (float *)h->cen[0].p, P0, 256);
        NUNIF_LAUNCH_CHECK();
    }
    f16 *eprev = (f16 *)h->emb[0].p, *ecur = (f16 *)h->emb[1].p;
    if ((rc = zrun(h->sproj1, x0, P0, 1, t128, s, "zoe_sproj1")) || (rc = zrun(h->sproj2, t128, P0, 0, eprev, s, "zoe_sproj2"))) return rc;
    int Hp = f->bh, Wp = f->bw;
    h->tap_b = B; h->tap_h[0] = Hp; h->tap_w[0] = Wp;
    for (int i = 0; i < 4; ++i) {
        const int Hc = f->rh[i], Wc = f->rw[i];
        const long P = (long)B * Hc * Wc;
        if ((rc = zrun(h->proj1[i], (const f16 *)f->blocks[i], P, 1, t128, s, "zoe_proj1")) || (rc = zrun(h->proj2[i], t128, P, 0, ecur, s, "zoe_proj2"))) return rc;
        {
            ProfScope ps("zoe_addup_kernel", s, 0.0, (double)P * kZEmb * 2.0 * 3.0);
            zoe_addup_kernel<<<zblocks(P * (kZEmb / 8)), 256, 0, s>>>(ecur, eprev, xa, B, Hc, Wc, Hp, Wp);
            NUNIF_LAUNCH_CHECK();
        }
        if ((rc = zrun(h->att1[i], xa, P, 1, a1, s, "zoe_att1"))) return rc;
        {
            ProfScope ps("zoe_attractor_kernel", s, (double)P * h->n_attr[i] * (2.0 * kZEmb + 6.0 * kZBins), (double)P * (kZEmb * 2.0 + kZBins * 8.0));
            zoe_attractor_kernel<<<(unsigned)((P + 3) / 4), 256, 0, s>>>(a1, h->att_w[i], h->att_b[i], (const float *)h->cen[i].p,
                                                                        (float *)h->cen[i + 1].p, B, Hc, Wc, Hp, Wp, h->n_attr[i], h->alpha);
            NUNIF_LAUNCH_CHECK();
        }
        std::swap(eprev, ecur);
        Hp = Hc; Wp = Wc;
        h->tap_h[i + 1] = Hc; h->tap_w[i + 1] = Wc;
    }
    if ((rc = zrun(h->e80, eprev, (long)B * Hp * Wp, 0, (f16 *)h->e80buf.p, s, "zoe_e80"))) return rc;
    ZoeFinalArgs g;
    g.act = (const f16 *)f->outconv; g.rel = rel; g.e80 = (const f16 *)h->e80buf.p; g.centres = (const float *)h->cen[4].p;
    g.w1 = h->w1; g.w2 = h->w2; g.logbinom = h->logbinom; g.out = out; g.B = B; g.H = H; g.W = W; g.Hp = Hp; g.Wp = Wp;
    g.min_temp = h->min_temp; g.max_temp = h->max_temp;
    {
        const double n = (double)B * H * W;
        ProfScope ps("zoe_final_kernel", s, n * (2.0 * kZHid * (kZRel + 4) + 8.0 * kZBins), n * (32 * 2.0 + 8.0 + 4 * (kZHid * 2.0 + kZBins * 4.0)));
        zoe_final_kernel<<<zblocks((long)B * H * W), 256, 0, s>>>(g);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}

// The bin centres of the last forward: tap 0 = the seed centres, 1 .. 4 = behind each attractor.  dst: [B,h,w,64] f32 (device),
// dims: {B, h, w} of that tap (host).  Either may be NULL.
extern "C" int nunif_hip_zoedepth_head_debug_taps(nunif_zoedepth_head *h, int32_t tap, float *dst, int32_t *dims, void *stream) {
    NUNIF_REQUIRE(h && tap >= 0 && tap < 5 && h->tap_b > 0, "zoedepth_head_debug_taps: tap 0..4 after a forward");
    if (dims) { dims[0] = h->tap_b; dims[1] = h->tap_h[tap]; dims[2] = h->tap_w[tap]; }
    if (dst)
        NUNIF_HIP_CHECK(hipMemcpyAsync(dst, h->cen[tap].p, (size_t)h->tap_b * h->tap_h[tap] * h->tap_w[tap] * kZBins * sizeof(float),
                                       hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return NUNIF_HIP_OK;
}

// Replaces the tail of batch_preprocess (iw3/zoedepth_model.py:66-83): reflection_pad2d_loop(x, [left, right, top, bottom]),
// clamp_(0, 1), (x - 0.5) / 0.5.  x: [planes,h,w] f32 -> y: [planes, h + top + bottom, w + left + right] f32.  A pad may exceed
// the map (the reference pads in steps of at most size - 1).
extern "C" int nunif_hip_zoedepth_pad_normalize(const float *x, float *y, int64_t planes, int32_t h, int32_t w, int32_t left,
                                                int32_t right, int32_t top, int32_t bottom, void *stream) {
    NUNIF_REQUIRE(x && y && planes > 0 && h > 0 && w > 0 && left >= 0 && right >= 0 && top >= 0 && bottom >= 0, "zoedepth_pad_normalize: bad argument");
    ZoePadAxis ay, ax;
    NUNIF_REQUIRE(pad_axis(h, top, bottom, &ay) && pad_axis(w, left, right, &ax), "zoedepth_pad_normalize: pad too large for a %d x %d map", h, w);
    const int H = h + top + bottom, W = w + left + right;
    zoe_prep_kernel<<<zblocks(planes * H * W), 256, 0, (hipStream_t)stream>>>(x, y, planes, h, w, H, W, ay, ax);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
