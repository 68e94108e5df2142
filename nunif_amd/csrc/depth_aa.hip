// iw3 "iw3.depth_aa" (depth anti-aliasing net, --depth-aa) on gfx950.
//
// Reference: iw3/models/depth_aa.py — DepthAA.infer :46-56 (tensor-wide min-max normalise, forward(clamp=False),
// de-normalise), DepthAA.forward :59-85 (centred replicate pad to multiples of 16, pixel_unshuffle 2, proj_in 4->32,
// three WABlocks with zero-pad shift True/False/True, proj_out 32->4, pixel_shuffle 2, crop, residual), WABlock :11-26;
// nunif/modules/attention.py WindowMHA2d :118-161 (window 8x8 = 64 tokens, 2 heads of 16), WindowScoreBias :375-419.
//
// Maps are NHWC fp16 [B, H/2, W/2, 32].  Kernels:
//   daa_minmax_kernel  tensor-wide min / max (order-preserving uint keys + atomics)
//   daa_in_kernel      normalise + pad + unshuffle + proj_in                               (VALU, K = 4)
//   run_wa_blocks      the WABlocks (wa_block.hip): wmha8_kernel, conv_mlp[0] 1x1 + GELU(erf), replicate-pad 3x3 + LeakyReLU +
//                      residual
//   daa_out_kernel     proj_out + pixel_shuffle + crop + residual + de-normalise           (VALU)
#include <algorithm>
#include <string>
#include <vector>

#include "wa_block.h"

namespace nunif {

__global__ void daa_minmax_init_kernel(unsigned int *mm) { mm[0] = 0xFFFFFFFFu; mm[1] = 0u; }

__global__ void __launch_bounds__(256) daa_minmax_kernel(const float *__restrict__ x, unsigned int *mm, long n) {
    float mn = 3.0e38f, mx = -3.0e38f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = x[i];
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    __shared__ float smn[256], smx[256];
    smn[threadIdx.x] = mn; smx[threadIdx.x] = mx;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + st]);
            smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + st]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { atomicMin(mm, order_key(smn[0])); atomicMax(mm + 1, order_key(smx[0])); }
}

struct DaaInArgs {
    const float *x;           // [B,1,h,w]
    const unsigned int *mm;   // min / max keys, or NULL: no normalisation (plain forward)
    const float *w;           // [4][32] then bias[32]   (k = i*2 + j of the 2x2 unshuffle)
    f16 *out;                 // [B,Hq,Wq,32]
    int B, h, w_, Hq, Wq, ph1, pw1;
};

__global__ void __launch_bounds__(256) daa_in_kernel(DaaInArgs a) {
    __shared__ float sw[5 * 32];
    if (threadIdx.x < 160) sw[threadIdx.x] = a.w[threadIdx.x];
    __syncthreads();
    const long total = (long)a.B * a.Hq * a.Wq;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int xq = (int)(id % a.Wq);
    const long t = id / a.Wq;
    const int yq = (int)(t % a.Hq), b = (int)(t / a.Hq);
    float mn = 0.f, scale = 1.f;
    if (a.mm) { mn = key_value(a.mm[0]); scale = key_value(a.mm[1]) - mn; }
    float in[4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int y = min(max(yq * 2 + i - a.ph1, 0), a.h - 1), x = min(max(xq * 2 + j - a.pw1, 0), a.w_ - 1);
            float v = a.x[((long)b * a.h + y) * a.w_ + x];
            if (a.mm) {
                v = (v - mn) / scale;                                  // depth_aa.py:49-51, nan_to_num
                if (v != v) v = 0.f;
                else if (v > 3.4028235e38f) v = 3.4028235e38f;
                else if (v < -3.4028235e38f) v = -3.4028235e38f;
            }
            in[i * 2 + j] = v;
        }
    f16 *o = a.out + id * 32;
    for (int c0 = 0; c0 < 32; c0 += 8) {
        f16x8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float acc = sw[4 * 32 + c0 + j];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fmaf(in[k], sw[k * 32 + c0 + j], acc);
            ov[j] = (f16)acc;
        }
        *reinterpret_cast<f16x8 *>(o + c0) = ov;
    }
}

struct DaaOutArgs {
    const f16 *f;             // [B,Hq,Wq,32]
    const float *src;         // [B,1,h,w] the un-normalised input
    const unsigned int *mm;   // or NULL
    const float *w;           // [32][4] then bias[4]
    float *out;               // [B,1,h,w]
    int B, h, w_, Hq, Wq, ph1, pw1, clamp01;
};

__global__ void __launch_bounds__(256) daa_out_kernel(DaaOutArgs a) {
    __shared__ float sw[33 * 4];
    if (threadIdx.x < 132) sw[threadIdx.x] = a.w[threadIdx.x];
    __syncthreads();
    const long total = (long)a.B * a.h * a.w_;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int x = (int)(id % a.w_);
    const long t = id / a.w_;
    const int y = (int)(t % a.h), b = (int)(t / a.h);
    const int yp = y + a.ph1, xp = x + a.pw1;
    const int n = (yp & 1) * 2 + (xp & 1);                            // pixel_shuffle 2: channel i*2 + j
    const f16 *p = a.f + (((long)b * a.Hq + (yp >> 1)) * a.Wq + (xp >> 1)) * 32;
    float acc = sw[32 * 4 + n];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc = fmaf((float)p[k], sw[k * 4 + n], acc);
    float v = a.src[id];
    if (a.mm) {
        const float mn = key_value(a.mm[0]), scale = key_value(a.mm[1]) - mn;
        float z = (v - mn) / scale;
        if (z != z) z = 0.f;
        v = (z + acc) * scale + mn;                                   // forward(clamp=False) * scale + min
    } else {
        v = v + acc;
        if (a.clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
    }
    a.out[id] = v;
}

}  // namespace nunif

using namespace nunif;

struct nunif_depth_aa : WaMaps {
    float *w_in = nullptr, *w_out = nullptr;
    WaBlock blk[3];
    DeviceBuf mm;
};

extern "C" int nunif_hip_depth_aa_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_depth_aa **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "depth_aa_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_depth_aa *h = new nunif_depth_aa();
    int rc = NUNIF_HIP_OK;
    do {
        const HostTensor *wi, *bi, *wo, *bo;
        if ((rc = find(m, "proj_in.weight", &wi)) || (rc = find(m, "proj_in.bias", &bi)) ||
            (rc = find(m, "proj_out.weight", &wo)) || (rc = find(m, "proj_out.bias", &bo)))
            break;
        if (wi->numel != 32 * 4 || wo->numel != 4 * 32) { set_error("depth_aa: unexpected proj shapes"); rc = NUNIF_HIP_EINVAL; break; }
        std::vector<float> win(5 * 32), wout(33 * 4);
        for (int k = 0; k < 4; ++k) for (int co = 0; co < 32; ++co) win[k * 32 + co] = wi->data[co * 4 + k];
        for (int co = 0; co < 32; ++co) win[4 * 32 + co] = bi->data[co];
        for (int k = 0; k < 32; ++k) for (int n = 0; n < 4; ++n) wout[k * 4 + n] = wo->data[n * 32 + k];
        for (int n = 0; n < 4; ++n) wout[32 * 4 + n] = bo->data[n];
        if ((rc = h->upload(win, &h->w_in)) || (rc = h->upload(wout, &h->w_out))) break;
        for (int i = 0; i < 3 && !rc; ++i) rc = make_wa_block(h, m, "blocks." + std::to_string(i) + ".", 8, 32, 16, &h->blk[i]);
    } while (0);
    if (rc) { nunif_hip_depth_aa_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_depth_aa_destroy(nunif_depth_aa *h) {
    if (!h) return;
    h->free_all();
    h->release_maps(); h->mm.release();
    delete h;
}

extern "C" int nunif_hip_depth_aa_forward(nunif_depth_aa *h, const float *x, float *y, int32_t B, int32_t hh, int32_t ww,
                                          int32_t mode, void *stream) {
    NUNIF_REQUIRE(h && x && y && B > 0 && hh > 0 && ww > 0 && mode >= 0 && mode <= 2, "depth_aa_forward: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int pad_w = 16 - ww % 16, pad_h = 16 - hh % 16;               // depth_aa.py:61-66
    const int pw1 = pad_w / 2, ph1 = pad_h / 2;
    const int Hq = (hh + pad_h) / 2, Wq = (ww + pad_w) / 2;
    const size_t tok = (size_t)B * Hq * Wq;
    int rc;
    if ((rc = h->ensure_maps(tok, 32)) || (rc = h->mm.ensure(16))) return rc;
    unsigned int *mm = mode == 2 ? (unsigned int *)h->mm.p : nullptr;
    const long px = (long)B * hh * ww;
    if (mm) {
        daa_minmax_init_kernel<<<1, 1, 0, s>>>(mm);
        daa_minmax_kernel<<<(unsigned)std::min<long>((px + 255) / 256, 1024), 256, 0, s>>>(x, mm, px);
        NUNIF_LAUNCH_CHECK();
    }
    {
        ProfScope ps("daa_in_kernel", s, 2.0 * 4 * 32 * (double)tok, (double)tok * (16.0 + 64.0));
        DaaInArgs a;
        a.x = x; a.mm = mm; a.w = h->w_in; a.out = (f16 *)h->f.p; a.B = B; a.h = hh; a.w_ = ww; a.Hq = Hq; a.Wq = Wq; a.ph1 = ph1; a.pw1 = pw1;
        daa_in_kernel<<<(unsigned)((tok + 255) / 256), 256, 0, s>>>(a);
        NUNIF_LAUNCH_CHECK();
    }
    static const int shift[3] = {4, 0, 4};                               // shift True / False / True
    f16 *cur;      // conv_mlp's 3x3 ends in LeakyReLU(0.1)
    if ((rc = run_wa_blocks(h, h->blk, 3, shift, shift, 32, B, Hq, Wq, 2, 0.1f, "depth_aa_mlp0", s, &cur))) return rc;
    {
        ProfScope ps("daa_out_kernel", s, 2.0 * 32 * (double)px, (double)px * (8.0 + 64.0));
        DaaOutArgs a;
        a.f = cur; a.src = x; a.mm = mm; a.w = h->w_out; a.out = y; a.B = B; a.h = hh; a.w_ = ww; a.Hq = Hq; a.Wq = Wq;
        a.ph1 = ph1; a.pw1 = pw1; a.clamp01 = mode == 1 ? 1 : 0;
        daa_out_kernel<<<(unsigned)((px + 255) / 256), 256, 0, s>>>(a);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}
