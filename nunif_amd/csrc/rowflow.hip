// iw3 "sbs.row_flow_v3" (the default --method) on gfx950: depth -> horizontal flow (delta) -> backward warp.
//
// Reference: iw3/models/row_flow_v3.py — RowFlowV3._forward :56-66 (replicate pad to multiples of 96 x 12,
// pixel_unshuffle (1,8), 1x1 conv 24->64, WABlock(4x4), WABlock(3x3), pixel_shuffle, crop, replicate-pad 3x3 conv 8->1),
// WABlock :14-30; nunif/modules/attention.py — WindowMHA2d :118-161, MHA :94-115, sliced_sdp :61-77 (2 heads of 32,
// float score bias), WindowScoreBias :375-419; iw3/backward_warp.py — backward_warp :67-83, make_grid :86-93,
// apply_divergence_nn_delta :191-236 (right eye = flipped inputs / flipped output).
//
// The net runs at DEPTH resolution (e.g. 392 x 686 -> 396 x 96 tokens of 64 channels, ~9 GFLOP per eye), so it is a
// handful of small launches; maps are NHWC fp16 like the other nets:
//   rf_input_kernel   pad + unshuffle + 1x1 conv 24->64                        (VALU, K = 24)
//   run_wa_blocks     the WABlocks (wa_block.hip): wmha_kernel<WS,C>, conv_mlp[0] 1x1 + GELU(erf), replicate-pad 3x3 +
//                     LeakyReLU + residual
//   rf_output_kernel  pixel_shuffle + crop + replicate-pad 3x3 conv 8->1 -> delta fp32
//   delta_warp_kernel grid = linspace + delta*scale, bilinear resize to the image size, grid_sample(border) + clamp
#include <string>
#include <vector>

#include "wa_block.h"

namespace nunif {

// ---------------------------------------------------------------------------------------------------------------------
struct RfInputArgs {
    const float *x;          // [B,3,h,w] planes: depth, divergence feature, convergence feature
    const float *w;          // [24][64] (k = c*8 + sw, transposed for broadcast reads) then bias[64]
    f16 *out;                // [B,Hp,Wq,64]
    int B, h, w_, Hp, Wq, flip;
};

__global__ void __launch_bounds__(256) rf_input_kernel(RfInputArgs a) {
    __shared__ float sw[25 * 64];
    for (int i = threadIdx.x; i < 25 * 64; i += 256) sw[i] = a.w[i];
    __syncthreads();
    const long total = (long)a.B * a.Hp * a.Wq;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int xq = (int)(id % a.Wq);
    const long t = id / a.Wq;
    const int y = (int)(t % a.Hp), b = (int)(t / a.Hp);
    const int yy = min(y, a.h - 1);                                   // replicate pad (bottom / right only)
    float in[24];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            int xx = min(xq * 8 + s, a.w_ - 1);
            if (a.flip) xx = a.w_ - 1 - xx;                            // the right eye runs on the mirrored depth
            in[c * 8 + s] = a.x[(((long)b * 3 + c) * a.h + yy) * a.w_ + xx];
        }
    f16 *o = a.out + id * 64;
    for (int c0 = 0; c0 < 64; c0 += 8) {
        f16x8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float acc = sw[24 * 64 + c0 + j];
#pragma unroll
            for (int k = 0; k < 24; ++k) acc = fmaf(in[k], sw[k * 64 + c0 + j], acc);
            ov[j] = (f16)acc;
        }
        *reinterpret_cast<f16x8 *>(o + c0) = ov;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct RfOutputArgs {
    const f16 *f;            // [B,Hp,Wq,64]
    const float *w;          // [8][3][3] then bias
    float *delta;            // [B,1,h,w]
    int B, h, w_, Hp, Wq;
};

__global__ void __launch_bounds__(256) rf_output_kernel(RfOutputArgs a) {
    __shared__ float sw[73];
    if (threadIdx.x < 73) sw[threadIdx.x] = a.w[threadIdx.x];
    __syncthreads();
    const long total = (long)a.B * a.h * a.w_;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int x = (int)(id % a.w_);
    const long t = id / a.w_;
    const int y = (int)(t % a.h), b = (int)(t / a.h);
    float acc = sw[72];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            // pixel_shuffle (1,8) + crop + ReplicationPad2d(1): shuffled[c][yy][xx] = f[yy][xx/8][c*8 + xx%8]
            const int yy = min(max(y + dy - 1, 0), a.h - 1), xx = min(max(x + dx - 1, 0), a.w_ - 1);
            const f16 *p = a.f + (((long)b * a.Hp + yy) * a.Wq + (xx >> 3)) * 64 + (xx & 7);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc = fmaf((float)p[c * 8], sw[(c * 3 + dy) * 3 + dx], acc);
        }
    a.delta[id] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
struct DeltaWarpArgs {
    const float *c;          // [B,C,H,W]
    const float *delta;      // [B,L,h,w] (horizontal flows at depth resolution, in the mirrored frame when flip)
    const float *weight;     // NULL (L = 1, weight 1) or [B,L,H,W] layer weights at IMAGE resolution (mirrored frame)
    float *out;              // [B,C,H,W]
    int B, C, H, W, h, w, flip, L;
    float delta_scale;
};

__device__ __forceinline__ float lin_pm1(int i, int n) {           // torch.linspace(-1, 1, n)[i]
    if (n <= 1) return -1.0f;
    const float step = 2.0f / (float)(n - 1);
    return i < n / 2 ? -1.0f + step * (float)i : 1.0f - step * (float)(n - 1 - i);
}

__global__ void __launch_bounds__(256) delta_warp_kernel(DeltaWarpArgs a) {
    const long total = (long)a.B * a.H * a.W;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int Xo = (int)(id % a.W);
    const long t = id / a.W;
    const int Y = (int)(t % a.H), b = (int)(t / a.H);
    const int X = a.flip ? a.W - 1 - Xo : Xo;                         // position in the (possibly mirrored) frame
    float accum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int layer = 0; layer < a.L; ++layer) {
    const float *dmap = a.delta + ((long)b * a.L + layer) * a.h * a.w;
    auto gx_at = [&](int yy, int xx) -> float { return lin_pm1(xx, a.w) + dmap[(long)yy * a.w + xx] * a.delta_scale; };
    float gx, gy;
    if (a.h == a.H && a.w == a.W) {
        gx = gx_at(Y, X);
        gy = lin_pm1(Y, a.h);
    } else {
        // F.interpolate(grid, size=(H,W), bilinear, align_corners=True)  (backward_warp.py:69-71)
        const float ry = a.H > 1 ? (float)(a.h - 1) / (float)(a.H - 1) : 0.f;
        const float rx = a.W > 1 ? (float)(a.w - 1) / (float)(a.W - 1) : 0.f;
        const float sy = ry * (float)Y, sx = rx * (float)X;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < a.h - 1 ? 1 : 0), x1 = x0 + (x0 < a.w - 1 ? 1 : 0);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        const float hy = 1.f - ly, hx = 1.f - lx;
        gx = hy * (hx * gx_at(y0, x0) + lx * gx_at(y0, x1)) + ly * (hx * gx_at(y1, x0) + lx * gx_at(y1, x1));
        const float g0 = lin_pm1(y0, a.h), g1 = lin_pm1(y1, a.h);
        gy = hy * (hx * g0 + lx * g0) + ly * (hx * g1 + lx * g1);
    }
    // grid_sampler_2d, align_corners=True, padding_mode=border
    float ix = ((gx + 1.f) / 2.f) * (float)(a.W - 1);
    float iy = ((gy + 1.f) / 2.f) * (float)(a.H - 1);
    ix = fminf(fmaxf(ix, 0.f), (float)(a.W - 1));
    iy = fminf(fmaxf(iy, 0.f), (float)(a.H - 1));
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float tx = ix - fx, ty = iy - fy;
    const float w_nw = (1.f - tx) * (1.f - ty), w_ne = tx * (1.f - ty), w_sw = (1.f - tx) * ty, w_se = tx * ty;
    const bool xin = x1 <= a.W - 1, yin = y1 <= a.H - 1;
    // the sampled image is the mirrored one when flip: column x of it is column W-1-x of c
    const int cx0 = a.flip ? a.W - 1 - x0 : x0, cx1 = a.flip ? a.W - 1 - x1 : x1;
    const float lw = a.weight ? a.weight[(((long)b * a.L + layer) * a.H + Y) * a.W + X] : 1.0f;
    for (int ch = 0; ch < a.C && ch < 4; ++ch) {
        const float *p = a.c + ((long)b * a.C + ch) * a.H * a.W;
        float v = p[(long)y0 * a.W + cx0] * w_nw;
        if (xin) v += p[(long)y0 * a.W + cx1] * w_ne;
        if (yin) v += p[(long)y1 * a.W + cx0] * w_sw;
        if (xin && yin) v += p[(long)y1 * a.W + cx1] * w_se;
        accum[ch] += fminf(fmaxf(v, 0.f), 1.f) * lw;                  // backward_warp clamps, then the layer weight
    }
    }
    for (int ch = 0; ch < a.C && ch < 4; ++ch)
        a.out[(((long)b * a.C + ch) * a.H + Y) * a.W + Xo] = fminf(fmaxf(accum[ch], 0.f), 1.f);
}

// ---------------------------------------------------------------------------------------------------------------------
// MLBW (iw3/models/mlbw.py): lv1_in = centred replicate pad to multiples of 32 x 4, ReplicationPad (4,4,0,0) + 1x9 conv
// 3 -> C/8 + LeakyReLU(0.2), written directly in the pixel_unshuffle (1,8) layout (channel c*8 + x%8 of token x/8).
struct MlbwInArgs {
    const float *x;          // [B,3,h,w]
    const float *w;          // [27][Cs] (k = ci*9 + tap) then bias[Cs]
    f16 *out, *x1;           // [B,Hp,Wq,C] twice: the working map and the preserved skip (x + x1 before lv1_out)
    int B, h, w_, Hp, Wp, ph1, pw1, Cs, flip;
};

__global__ void __launch_bounds__(256) mlbw_in_kernel(MlbwInArgs a) {
    __shared__ float sw[28 * 16];
    for (int i = threadIdx.x; i < 28 * a.Cs; i += 256) sw[i] = a.w[i];
    __syncthreads();
    const long total = (long)a.B * a.Hp * a.Wp;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int xp = (int)(id % a.Wp);
    const long t = id / a.Wp;
    const int yp = (int)(t % a.Hp), b = (int)(t / a.Hp);
    const int y = min(max(yp - a.ph1, 0), a.h - 1);
    float in[27];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int xs = min(max(xp + k - 4, 0), a.Wp - 1);              // lv1_in's own replicate pad, on the padded map
        int xx = min(max(xs - a.pw1, 0), a.w_ - 1);
        if (a.flip) xx = a.w_ - 1 - xx;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) in[ci * 9 + k] = a.x[(((long)b * 3 + ci) * a.h + y) * a.w_ + xx];
    }
    const int C = a.Cs * 8;
    const long base = (((long)b * a.Hp + yp) * (a.Wp >> 3) + (xp >> 3)) * C + (xp & 7);
    for (int co = 0; co < a.Cs; ++co) {
        float acc = sw[27 * a.Cs + co];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc = fmaf(in[k], sw[k * a.Cs + co], acc);
        acc = acc >= 0.f ? acc : acc * 0.2f;
        a.out[base + co * 8] = (f16)acc;
        a.x1[base + co * 8] = (f16)acc;
    }
}

// lv1_out: pixel_shuffle + (x + x1) + ReplicationPad (4,4,0,0) + 1x9 conv C/8 -> 2L, crop, softmax over the L logits
struct MlbwOutArgs {
    const f16 *f, *x1;       // [B,Hp,Wq,C]
    const float *w;          // [Cs*9][2L] (k = ci*9 + tap) then bias[2L]
    float *delta, *weight;   // [B,L,h,w] each
    float *mask;             // hole-mask variant (2L + 1 outputs): [B,1,h,w] logits in IMAGE coordinates, else NULL
    int B, h, w_, Hp, Wp, ph1, pw1, Cs, L, no, flip;
};

__global__ void __launch_bounds__(256) mlbw_out_kernel(MlbwOutArgs a) {
    __shared__ float sw[(16 * 9 + 1) * 8];
    const int no = a.no;         // 2L, or 2L + 1 with the hole-mask logit (mlbw.py:70-75, 104-106)
    for (int i = threadIdx.x; i < (a.Cs * 9 + 1) * no; i += 256) sw[i] = a.w[i];
    __syncthreads();
    const long total = (long)a.B * a.h * a.w_;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int x = (int)(id % a.w_);
    const long t = id / a.w_;
    const int y = (int)(t % a.h), b = (int)(t / a.h);
    const int yp = y + a.ph1, xp = x + a.pw1, C = a.Cs * 8;
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = o < no ? sw[a.Cs * 9 * no + o] : 0.f;
    for (int k = 0; k < 9; ++k) {
        const int xs = min(max(xp + k - 4, 0), a.Wp - 1);
        const long base = (((long)b * a.Hp + yp) * (a.Wp >> 3) + (xs >> 3)) * C + (xs & 7);
        for (int ci = 0; ci < a.Cs; ++ci) {
            const float v = (float)a.f[base + ci * 8] + (float)a.x1[base + ci * 8];
            const float *wr = sw + (ci * 9 + k) * no;
#pragma unroll
            for (int o = 0; o < 8; ++o) if (o < no) acc[o] = fmaf(v, wr[o], acc[o]);
        }
    }
    float mx = -3.0e38f;
    for (int i = 0; i < a.L; ++i) mx = fmaxf(mx, acc[a.L + i]);
    float e[4], sum = 0.f;
    for (int i = 0; i < a.L; ++i) { e[i] = expf(acc[a.L + i] - mx); sum += e[i]; }
    const long hw = (long)a.h * a.w_, o0 = (long)b * a.L * hw + (long)y * a.w_ + x;
    for (int i = 0; i < a.L; ++i) {
        a.delta[o0 + i * hw] = acc[i];
        a.weight[o0 + i * hw] = e[i] / sum;
    }
    // the reference flips the logits back for the right eye (backward_warp.py:325-327); delta / weight stay in model
    // coordinates because the warp kernel folds the flip
    if (a.mask) a.mask[((long)b * a.h + y) * a.w_ + (a.flip ? a.w_ - 1 - x : x)] = acc[2 * a.L];
}

}  // namespace nunif

using namespace nunif;

// =====================================================================================================================
// host side
// =====================================================================================================================
static const int kNoShift[2] = {0, 0};

struct nunif_row_flow : WaMaps {
    float *w_in = nullptr, *w_out = nullptr;
    WaBlock blk[2];
};

extern "C" int nunif_hip_row_flow_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_row_flow **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "row_flow_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_row_flow *h = new nunif_row_flow();
    int rc = NUNIF_HIP_OK;
    do {
        const HostTensor *w0, *b0, *wl, *bl;
        if ((rc = find(m, "blocks.0.weight", &w0)) || (rc = find(m, "blocks.0.bias", &b0)) ||
            (rc = find(m, "last_layer.1.weight", &wl)) || (rc = find(m, "last_layer.1.bias", &bl)))
            break;
        if (w0->numel != 64 * 24 || wl->numel != 72) { set_error("row_flow_v3: unexpected stem / head shape"); rc = NUNIF_HIP_EINVAL; break; }
        std::vector<float> win(25 * 64), wout(73);
        for (int k = 0; k < 24; ++k) for (int co = 0; co < 64; ++co) win[k * 64 + co] = w0->data[co * 24 + k];
        for (int co = 0; co < 64; ++co) win[24 * 64 + co] = b0->data[co];
        for (int i = 0; i < 72; ++i) wout[i] = wl->data[i];
        wout[72] = bl->data[0];
        if ((rc = h->upload(win, &h->w_in)) || (rc = h->upload(wout, &h->w_out))) break;
        if ((rc = make_wa_block(h, m, "blocks.1.", 4, 64, 32, &h->blk[0]))) break;
        if ((rc = make_wa_block(h, m, "blocks.2.", 3, 64, 32, &h->blk[1]))) break;
    } while (0);
    if (rc) { nunif_hip_row_flow_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_row_flow_destroy(nunif_row_flow *h) {
    if (!h) return;
    h->free_all();
    h->release_maps();
    delete h;
}

extern "C" int nunif_hip_row_flow_delta(nunif_row_flow *h, const float *x, float *delta, int32_t B, int32_t hh,
                                        int32_t ww, int32_t flip, void *stream) {
    NUNIF_REQUIRE(h && x && delta && B > 0 && hh > 0 && ww > 0, "row_flow_delta: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int Hp = hh + (12 - hh % 12), Wp = ww + (96 - ww % 96), Wq = Wp / 8;          // row_flow_v3.py:58-59
    const size_t tok = (size_t)B * Hp * Wq;
    int rc;
    if ((rc = h->ensure_maps(tok, 64))) return rc;
    {
        ProfScope ps("rf_input_kernel", s, 2.0 * 24 * 64 * (double)tok, (double)tok * (12.0 * 8 + 128.0));
        RfInputArgs a;
        a.x = x; a.w = h->w_in; a.out = (f16 *)h->f.p; a.B = B; a.h = hh; a.w_ = ww; a.Hp = Hp; a.Wq = Wq; a.flip = flip;
        rf_input_kernel<<<(unsigned)((tok + 255) / 256), 256, 0, s>>>(a);
        NUNIF_LAUNCH_CHECK();
    }
    f16 *cur;      // conv_mlp's 3x3 ends in LeakyReLU(0.1)
    if ((rc = run_wa_blocks(h, h->blk, 2, kNoShift, kNoShift, 64, B, Hp, Wq, 2, 0.1f, "rowflow_mlp0", s, &cur))) return rc;
    {
        const long px = (long)B * hh * ww;
        ProfScope ps("rf_output_kernel", s, 2.0 * 72 * (double)px, (double)px * (4.0 + 16.0));
        RfOutputArgs a;
        a.f = cur; a.w = h->w_out; a.delta = delta; a.B = B; a.h = hh; a.w_ = ww; a.Hp = Hp; a.Wq = Wq;
        rf_output_kernel<<<(unsigned)((px + 255) / 256), 256, 0, s>>>(a);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}

static int run_delta_warp(const float *c, const float *delta, const float *weight, float *out, int B, int C, int H,
                          int W, int dh, int dw, int L, double delta_scale, int flip, hipStream_t s) {
    DeltaWarpArgs a;
    a.c = c; a.delta = delta; a.weight = weight; a.out = out; a.B = B; a.C = C; a.H = H; a.W = W; a.h = dh; a.w = dw;
    a.flip = flip; a.L = L; a.delta_scale = (float)delta_scale;
    const long total = (long)B * H * W;
    ProfScope ps("delta_warp_kernel", s, 0.0, (double)total * (4.0 + 8.0 * C + (weight ? 4.0 * L : 0.0)));
    delta_warp_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(a);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_delta_warp(const float *c, const float *delta, float *out, int32_t B, int32_t C, int32_t H,
                                    int32_t W, int32_t dh, int32_t dw, double delta_scale, int32_t flip, void *stream) {
    NUNIF_REQUIRE(c && delta && out && B > 0 && C > 0 && C <= 4 && H > 0 && W > 0 && dh > 0 && dw > 0, "delta_warp: bad argument");
    return run_delta_warp(c, delta, nullptr, out, B, C, H, W, dh, dw, 1, delta_scale, flip, (hipStream_t)stream);
}

extern "C" int nunif_hip_delta_weight_warp(const float *c, const float *delta, const float *weight, float *out, int32_t B,
                                           int32_t C, int32_t H, int32_t W, int32_t dh, int32_t dw, int32_t L,
                                           double delta_scale, int32_t flip, void *stream) {
    NUNIF_REQUIRE(c && delta && weight && out && B > 0 && C > 0 && C <= 4 && H > 0 && W > 0 && dh > 0 && dw > 0 && L > 0 && L <= 4,
                  "delta_weight_warp: bad argument");
    return run_delta_warp(c, delta, weight, out, B, C, H, W, dh, dw, L, delta_scale, flip, (hipStream_t)stream);
}

// ---- MLBW --------------------------------------------------------------------------------------------------------------
struct nunif_mlbw : WaMaps {
    int L = 2, C = 64, n_blocks = 4, hole_mask = 0;
    float *w_in = nullptr, *w_out = nullptr;
    WaBlock blk[4];
    int sy[4] = {0, 0, 0, 0}, sx[4] = {0, 0, 0, 0};
    DeviceBuf x1;
};

extern "C" int nunif_hip_mlbw_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_mlbw **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "mlbw_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_mlbw *h = new nunif_mlbw();
    int rc = NUNIF_HIP_OK;
    do {
        const HostTensor *wi, *bi, *wo, *bo;
        if ((rc = find(m, "lv1_in.1.weight", &wi)) || (rc = find(m, "lv1_in.1.bias", &bi)) ||
            (rc = find(m, "lv1_out.1.weight", &wo)) || (rc = find(m, "lv1_out.1.bias", &bo)))
            break;
        const int Cs = (int)bi->numel;                  // C / 8
        h->C = Cs * 8; h->L = h->C / 32;
        h->hole_mask = bo->numel == 2 * h->L + 1 ? 1 : 0;             // sbs.mask_mlbw_l2 (mlbw.py:275-278)
        const int no = 2 * h->L + h->hole_mask;
        if ((Cs != 8 && Cs != 16) || wi->numel != (int64_t)Cs * 27 || bo->numel != no || no > 8 ||
            wo->numel != (int64_t)no * Cs * 9) {
            set_error("mlbw: unsupported shape (C/8 = %d, %lld outputs)", Cs,
                      (long long)bo->numel);
            rc = NUNIF_HIP_EUNSUPPORTED;
            break;
        }
        h->n_blocks = m.count("lv2.3.mha.mha.qkv_proj.weight") ? 4 : 2;
        // shifts (mlbw.py:57-68): full (T,T),(F,F),(T,T),(F,F); small (F,T),(F,F)
        if (h->n_blocks == 4) { h->sy[0] = h->sx[0] = 2; h->sy[2] = h->sx[2] = 2; }
        else { h->sx[0] = 2; }
        std::vector<float> win(28 * Cs), wout((size_t)(Cs * 9 + 1) * no);
        for (int k = 0; k < 27; ++k) for (int co = 0; co < Cs; ++co) win[k * Cs + co] = wi->data[co * 27 + k];
        for (int co = 0; co < Cs; ++co) win[27 * Cs + co] = bi->data[co];
        for (int k = 0; k < Cs * 9; ++k) for (int o = 0; o < no; ++o) wout[(size_t)k * no + o] = wo->data[(size_t)o * Cs * 9 + k];
        for (int o = 0; o < no; ++o) wout[(size_t)Cs * 9 * no + o] = bo->data[o];
        if ((rc = h->upload(win, &h->w_in)) || (rc = h->upload(wout, &h->w_out))) break;
        for (int i = 0; i < h->n_blocks && !rc; ++i)
            rc = make_wa_block(h, m, "lv2." + std::to_string(i) + ".", 4, h->C, 32, &h->blk[i]);
    } while (0);
    if (rc) { nunif_hip_mlbw_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_mlbw_destroy(nunif_mlbw *h) {
    if (!h) return;
    h->free_all();
    h->release_maps(); h->x1.release();
    delete h;
}

extern "C" int32_t nunif_hip_mlbw_num_layers(const nunif_mlbw *h) { return h ? h->L : 0; }
extern "C" int32_t nunif_hip_mlbw_has_hole_mask(const nunif_mlbw *h) { return h ? h->hole_mask : 0; }

extern "C" int nunif_hip_mlbw_delta(nunif_mlbw *h, const float *x, float *delta, float *weight, int32_t B, int32_t hh,
                                    int32_t ww, int32_t flip, void *stream) {
    return nunif_hip_mlbw_delta_mask(h, x, delta, weight, nullptr, B, hh, ww, flip, stream);
}

extern "C" int nunif_hip_mlbw_delta_mask(nunif_mlbw *h, const float *x, float *delta, float *weight, float *mask_logits,
                                         int32_t B, int32_t hh, int32_t ww, int32_t flip, void *stream) {
    NUNIF_REQUIRE(h && x && delta && weight && B > 0 && hh > 0 && ww > 0, "mlbw_delta: bad argument");
    NUNIF_REQUIRE(!mask_logits || h->hole_mask, "mlbw_delta_mask: this model has no hole-mask output");
    hipStream_t s = (hipStream_t)stream;
    const int pad_w = 32 - ww % 32, pad_h = 4 - hh % 4;                 // mlbw.py:78-93 (eval: centred)
    const int pw1 = pad_w / 2, ph1 = pad_h / 2;
    const int Hp = hh + pad_h, Wp = ww + pad_w, Wq = Wp / 8, C = h->C, Cs = C / 8;
    const size_t tok = (size_t)B * Hp * Wq;
    int rc;
    if ((rc = h->ensure_maps(tok, C)) || (rc = h->x1.ensure(tok * C * sizeof(f16)))) return rc;
    f16 *x1 = (f16 *)h->x1.p;
    {
        const long px = (long)B * Hp * Wp;
        ProfScope ps("mlbw_in_kernel", s, 2.0 * 27 * Cs * (double)px, (double)px * (12.0 + 4.0 * Cs));
        MlbwInArgs a;
        a.x = x; a.w = h->w_in; a.out = (f16 *)h->f.p; a.x1 = x1; a.B = B; a.h = hh; a.w_ = ww; a.Hp = Hp; a.Wp = Wp; a.ph1 = ph1;
        a.pw1 = pw1; a.Cs = Cs; a.flip = flip;
        mlbw_in_kernel<<<(unsigned)((px + 255) / 256), 256, 0, s>>>(a);
        NUNIF_LAUNCH_CHECK();
    }
    f16 *cur;      // MLBW's conv_mlp has no activation after the 3x3
    if ((rc = run_wa_blocks(h, h->blk, h->n_blocks, h->sy, h->sx, C, B, Hp, Wq, 0, 0.f, "mlbw_mlp0", s, &cur))) return rc;
    {
        const long px = (long)B * hh * ww;
        ProfScope ps("mlbw_out_kernel", s, 2.0 * 9 * Cs * 2 * h->L * (double)px, (double)px * (8.0 * h->L + 36.0 * Cs));
        MlbwOutArgs a;
        a.f = cur; a.x1 = x1; a.w = h->w_out; a.delta = delta; a.weight = weight; a.B = B; a.h = hh; a.w_ = ww; a.Hp = Hp;
        a.Wp = Wp; a.ph1 = ph1; a.pw1 = pw1; a.Cs = Cs; a.L = h->L; a.no = 2 * h->L + h->hole_mask; a.flip = flip;
        a.mask = mask_logits;
        mlbw_out_kernel<<<(unsigned)((px + 255) / 256), 256, 0, s>>>(a);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}
