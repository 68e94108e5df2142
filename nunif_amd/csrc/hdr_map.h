// The HDR -> SDR map of one pixel and the three output forms, shared by hdr.hip (rgb48 frame in) and hdr_planes.hip (yuv420p10le
// planes in): the constants, the device functions and the stores of a lane's 8 pixels / 1 pixel.  hdr.hip's header comment states
// the arithmetic and why the powers are evaluated as they are; both files are built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace nunif {

enum { HDR_PQ = 16, HDR_HLG = 18 };                      // AVCOL_TRC_SMPTE2084 / AVCOL_TRC_ARIB_STD_B67 (video.py:24-25)
enum { HDR_FORM_U16 = 0, HDR_FORM_CHW = 1, HDR_FORM_DEBUG = 2 };

struct HdrConst {
    float m[9];            // BT.2020 -> bt709 / bt601, row major (:373-383)
    float exposure;        // pq_exposure / hlg_exposure as fp32
    float hable_white;     // hable_map(white) in the reference's fp32 expressions
    float cb, de, df, ef;  // C * B, D * E, D * F, E / F: Python float products, then fp32 (:357-358)
    float gain, one_minus_gain;
    int mix;               // HLG with saturation_gain < 1
};

// the reference's Python-float scalars become fp32 when they meet an fp32 tensor
static const double kA = 0.15, kB = 0.50, kC = 0.10, kD = 0.20, kF = 0.30;

static inline float hable_host(float v, const HdrConst &k) {
    const float a = (float)kA, b = (float)kB;
    return ((v * (a * v + k.cb) + k.de) / (v * (a * v + b) + k.df)) - k.ef;
}

static inline bool make_const(int trc, int colorspace, const nunif_hdr2sdr_params *p, HdrConst *k) {
    static const float m709[9] = {1.6605f, -0.5876f, -0.0728f, -0.1246f, 1.1329f, -0.0083f, -0.0182f, -0.1006f, 1.1187f};
    static const float m601[9] = {1.5540f, -0.5143f, -0.0397f, -0.1017f, 1.1147f, -0.0130f, -0.0163f, -0.0886f, 1.1049f};
    if ((trc != HDR_PQ && trc != HDR_HLG) || (colorspace != 709 && colorspace != 601) || !p) return false;
    const double E = trc == HDR_HLG ? 0.01 : 0.02;
    for (int i = 0; i < 9; ++i) k->m[i] = colorspace == 709 ? m709[i] : m601[i];
    k->exposure = (float)p->exposure;
    k->cb = (float)(kC * kB); k->de = (float)(kD * E); k->df = (float)(kD * kF); k->ef = (float)(E / kF);
    k->hable_white = hable_host((float)p->white_point, *k);
    k->gain = (float)p->saturation_gain; k->one_minus_gain = (float)(1.0 - p->saturation_gain);
    k->mix = trc == HDR_HLG && p->saturation_gain < 1.0;
    return true;
}

// x ** g for x >= 0, g > 0 (0 ** g = 0).  y = g * log2 x is rounded once; r is that rounding error (exact, by FMA), and
// 2 ** (y + r) = 2 ** y * (1 + r ln 2) to first order — what is left is the 1 ulp of each of the two instructions.
__device__ __forceinline__ float pow_pos(float x, float g) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (!(x > 0.f)) return 0.f;
    const float l = __builtin_amdgcn_logf(x), y = g * l, r = __builtin_fmaf(g, l, -y);
    const float e = __builtin_amdgcn_exp2f(y);
    return __builtin_fmaf(e, r * 0.6931471805599453f, e);
#else
    return 0.f;                    // host pass of the single-source compile only parses this
#endif
}

__device__ __forceinline__ float exp_acc(float t) {      // e ** t, |t| < 4
#if defined(__HIP_DEVICE_COMPILE__)
    const float L = 1.4426950408889634f, Llo = 1.9259629911266175e-8f;       // log2 e = L + Llo
    const float y = t * L, r = __builtin_fmaf(t, L, -y) + t * Llo;
    const float e = __builtin_amdgcn_exp2f(y);
    return __builtin_fmaf(e, r * 0.6931471805599453f, e);
#else
    return 0.f;
#endif
}

// PQ code value x in [0, 1] -> linear light (:330-333), by the cancellation-free form described at the top of hdr.hip
__device__ __forceinline__ float pq_linear(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float K = 0.1640625f, c3 = 18.6875f;                                // 21 / 128 = 1 - c1 = c2 - c3; 2392 / 4096 * 32
    const float ln2_over_m2 = (float)(0.6931471805599453 / (2523.0 / 4096.0 * 128.0));
    // code 0 (log2 = -inf) and anything below code 1 lands on -0.2, where 21/128 + p < 0 and the clamp of :333 gives 0
    const float z = fmaxf(__builtin_amdgcn_logf(x) * ln2_over_m2, -0.2f);
    float p = 1.0f / 5040.0f;
    p = __builtin_fmaf(p, z, 1.0f / 720.0f);
    p = __builtin_fmaf(p, z, 1.0f / 120.0f);
    p = __builtin_fmaf(p, z, 1.0f / 24.0f);
    p = __builtin_fmaf(p, z, 1.0f / 6.0f);
    p = __builtin_fmaf(p, z, 0.5f);
    p = __builtin_fmaf(p, z, 1.0f);
    p = p * z;                                                                // expm1(z) = x ** (1 / m2) - 1
    const float q = fmaxf(K + p, 0.f) / __builtin_fmaf(-c3, p, K);
    return pow_pos(q, (float)(1.0 / (2610.0 / 16384.0)));
#else
    return 0.f;
#endif
}

__device__ __forceinline__ float hlg_linear(float x) {                        // :338-344
    const float a = 0.17883277f, b = 0.28466892f, c = 0.55991073f;
    return x <= 0.5f ? (x * x) / 3.0f : (exp_acc((x - c) / a) + b) / 12.0f;
}

__device__ __forceinline__ float hable(float v, const HdrConst &k) {          // :356-358
    const float a = (float)0.15, b = (float)0.50;
    return ((v * (a * v + k.cb) + k.de) / (v * (a * v + b) + k.df)) - k.ef;
}

__device__ __forceinline__ float oetf(float v) {                              // :388-395 and the clamp of :398
    v = fminf(fmaxf(v, 0.f), 1.f);
    const float g = v < 0.018f ? v * 4.5f : 1.099f * pow_pos(v, 0.45f) - 0.099f;
    return fminf(fmaxf(g, 0.f), 1.f);
}

// one pixel: three 16-bit codes -> the three values before `* 65535`
template <int TRC>
__device__ __forceinline__ void map_pixel(unsigned r, unsigned g, unsigned b, const HdrConst &k, float out[3]) {
    float s[3] = {(float)r / 65535.0f, (float)g / 65535.0f, (float)b / 65535.0f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lin = TRC == HDR_PQ ? pq_linear(s[c]) : hlg_linear(s[c]);
        s[c] = hable(lin * k.exposure, k) / k.hable_white;
    }
    if (TRC == HDR_HLG && k.mix) {
        const float luma = s[0] * 0.2126f + s[1] * 0.7152f + s[2] * 0.0722f;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = (s[c] * k.gain) + (luma * k.one_minus_gain);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = oetf(k.m[3 * c] * s[0] + k.m[3 * c + 1] * s[1] + k.m[3 * c + 2] * s[2]);
}

__device__ __forceinline__ unsigned quant16(float v) { return (unsigned)(v * 65535.0f); }      // .to(torch.uint16) truncates

// ---- the three output forms ---------------------------------------------------------------------------------------------------
// 8 consecutive pixels, v[3 * pixel + channel], the first of them pixel p of the frame taken as a flat array of n pixels, in
// 16-byte stores: three (u16), six (chw, debug).  The caller has checked the alignment: dst % 16 == 0 and p % 8 == 0 (u16),
// p % 4 == 0 (debug), p % 4 == 0 and n % 4 == 0 (chw).
template <int FORM>
__device__ __forceinline__ void store_pixels8(void *__restrict__ dst, long p, long n, const float *v) {
    if (FORM == HDR_FORM_U16) {
        u32x4 *o = (u32x4 *)((uint16_t *)dst + p * 3);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            u32x4 ow;
#pragma unroll
            for (int e = 0; e < 4; ++e) ow[e] = quant16(v[8 * t + 2 * e]) | (quant16(v[8 * t + 2 * e + 1]) << 16);
            o[t] = ow;
        }
    } else if (FORM == HDR_FORM_CHW) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4 *o = (f32x4 *)((float *)dst + c * n + p);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = (float)quant16(v[3 * (4 * t + e) + c]) / 65535.0f;
                o[t] = ov;
            }
        }
    } else {
        f32x4 *o = (f32x4 *)((float *)dst + p * 3);
#pragma unroll
        for (int t = 0; t < 6; ++t) o[t] = (f32x4){v[4 * t], v[4 * t + 1], v[4 * t + 2], v[4 * t + 3]};
    }
}

// pixel p alone, v[channel]
template <int FORM>
__device__ __forceinline__ void store_pixel(void *__restrict__ dst, long p, long n, const float *v) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (FORM == HDR_FORM_U16) ((uint16_t *)dst)[p * 3 + c] = (uint16_t)quant16(v[c]);
        else if (FORM == HDR_FORM_CHW) ((float *)dst)[c * n + p] = (float)quant16(v[c]) / 65535.0f;
        else ((float *)dst)[p * 3 + c] = v[c];
    }
}

}  // namespace nunif
