// HDR (BT.2020, PQ or HLG) -> SDR (BT.709 / BT.601) tone mapping of one rgb48 frame on gfx950: one kernel, one pass.
//
// Reference: nunif/utils/video.py hdr2sdr :309-416, called once per decoded frame by process_video's input_reformatter
// (:1025-1036): upload, x / 65535 (:325), the inverse EOTF (PQ :330-333, HLG :338-344), exposure (:354), the Hable map over the
// Hable map of the white point (:356-369), for HLG the luma mix (:363-367), the 3 x 3 matrix (:372-387), clamp (:388), the OETF
// with its linear toe (:391-395), clamp, * 65535 and truncation to uint16 (:398), download; VU.to_tensor (:218-223) then uploads
// the frame again and divides by 65535.  About thirty fp32 passes over 3 x H x W and three PCIe crossings; here the frame is read
// once (from the device or zero-copy from pinned host memory) and written once, in the form the next step wants.
//
// Every step from the Hable map on is the reference's fp32 expression, operation by operation, in its order (-ffp-contract=off:
// no FMA where the reference has a multiply and an add), so those steps carry the reference's own rounding and nothing else.
// Divisions are IEEE divisions as in the reference.  The powers are where the two differ ("HDR to SDR"):
//   * x ** g is exp2(g * log2 x) on the 1-ulp v_log_f32 / v_exp_f32, with the rounding error of the product g * log2 x carried
//     into the result by one FMA; exp likewise.  powf costs ~250 instructions a call and there are up to nine per pixel.
//   * the PQ curve is NOT evaluated as the reference writes it.  With xp = x ** (1 / m2) the reference forms xp - c1 and
//     c2 - c3 * xp: both cancel (c2 - c3 * xp is 18.85 - 18.69 at xp = 1: an error of 1 ulp of 18 over 0.16, then raised to the
//     6.28th power — the 5 counts of 65535 by which the reference's fp32 differs from float64).  Since 1 - c1 = c2 - c3 = 21 / 128
//     exactly, with p = xp - 1 = expm1(ln x / m2) both are sums without that cancellation: xp - c1 = 21/128 + p and
//     c2 - c3 * xp = 21/128 - c3 * p (p <= 0).  |ln x / m2| <= 0.1407 for every code >= 1, where the degree-7 Taylor polynomial of
//     expm1 is exact to 4e-12.
//
// A lane owns 8 consecutive pixels of the frame taken as a flat array (the map is pointwise): 48 B of rgb48 = three 16-byte
// loads; the u16 form stores three 16-byte pieces, the planar and debug forms six.  Pixels beyond the last whole group of 8, or the
// whole frame when a pointer or the plane stride does not allow 16-byte accesses, go through the one-pixel-per-lane kernel: the same
// device function, the same bits.
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

static float hable_host(float v, const HdrConst &k) {
    const float a = (float)kA, b = (float)kB;
    return ((v * (a * v + k.cb) + k.de) / (v * (a * v + b) + k.df)) - k.ef;
}

static bool make_const(int trc, int colorspace, const nunif_hdr2sdr_params *p, HdrConst *k) {
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

// PQ code value x in [0, 1] -> linear light (:330-333), by the cancellation-free form described at the top
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

// 8 pixels per lane, flat over the first `groups * 8` pixels of the frame.  n: pixels of the whole frame (the plane stride).
template <int TRC, int FORM>
__global__ void __launch_bounds__(256)
hdr2sdr_vec_kernel(const u32x4 *__restrict__ src, void *__restrict__ dst, long groups, long n, HdrConst k) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= groups) return;
    const u32x4 w0 = src[i * 3], w1 = src[i * 3 + 1], w2 = src[i * 3 + 2];
    const unsigned w[12] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3]};
    float v[24];                                                             // HWC: v[3 * pixel + channel]
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned c[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) { const int h = 3 * j + e; c[e] = (w[h >> 1] >> (16 * (h & 1))) & 0xffffu; }
        map_pixel<TRC>(c[0], c[1], c[2], k, v + 3 * j);
    }
    if (FORM == HDR_FORM_U16) {
        u32x4 *o = (u32x4 *)dst + i * 3;
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
            f32x4 *o = (f32x4 *)((float *)dst + c * n + i * 8);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = (float)quant16(v[3 * (4 * t + e) + c]) / 65535.0f;
                o[t] = ov;
            }
        }
    } else {
        f32x4 *o = (f32x4 *)dst + i * 6;
#pragma unroll
        for (int t = 0; t < 6; ++t) o[t] = (f32x4){v[4 * t], v[4 * t + 1], v[4 * t + 2], v[4 * t + 3]};
    }
}

// one pixel per lane over pixels [first, n)
template <int TRC, int FORM>
__global__ void __launch_bounds__(256)
hdr2sdr_px_kernel(const uint16_t *__restrict__ src, void *__restrict__ dst, long first, long n, HdrConst k) {
    const long i = first + (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[3];
    map_pixel<TRC>(src[i * 3], src[i * 3 + 1], src[i * 3 + 2], k, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (FORM == HDR_FORM_U16) ((uint16_t *)dst)[i * 3 + c] = (uint16_t)quant16(v[c]);
        else if (FORM == HDR_FORM_CHW) ((float *)dst)[c * n + i] = (float)quant16(v[c]) / 65535.0f;
        else ((float *)dst)[i * 3 + c] = v[c];
    }
}

template <int TRC, int FORM>
static void launch(const void *src, void *dst, long n, bool vec, const HdrConst &k, hipStream_t s) {
    const long groups = vec ? n / 8 : 0, rest = n - groups * 8;
    if (groups)
        hdr2sdr_vec_kernel<TRC, FORM><<<(unsigned)((groups + 255) / 256), 256, 0, s>>>((const u32x4 *)src, dst, groups, n, k);
    if (rest)
        hdr2sdr_px_kernel<TRC, FORM><<<(unsigned)((rest + 255) / 256), 256, 0, s>>>((const uint16_t *)src, dst, groups * 8, n, k);
}

template <int TRC>
static void launch_form(int form, const void *src, void *dst, long n, bool vec, const HdrConst &k, hipStream_t s) {
    if (form == HDR_FORM_U16) launch<TRC, HDR_FORM_U16>(src, dst, n, vec, k, s);
    else if (form == HDR_FORM_CHW) launch<TRC, HDR_FORM_CHW>(src, dst, n, vec, k, s);
    else launch<TRC, HDR_FORM_DEBUG>(src, dst, n, vec, k, s);
}

}  // namespace nunif

using namespace nunif;

extern "C" int nunif_hip_hdr2sdr_constants(int32_t trc, int32_t colorspace, const nunif_hdr2sdr_params *params, float *matrix,
                                           float *hable_white) {
    HdrConst k;
    NUNIF_REQUIRE(matrix && hable_white, "hdr2sdr_constants: bad argument");
    NUNIF_REQUIRE(make_const(trc, colorspace, params, &k),
                  "hdr2sdr_constants: trc must be 16 (PQ) or 18 (HLG) and colorspace 709 or 601");
    for (int i = 0; i < 9; ++i) matrix[i] = k.m[i];
    *hable_white = k.hable_white;
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_hdr2sdr(const void *src, void *dst, int32_t H, int32_t W, int32_t trc, int32_t colorspace,
                                 const nunif_hdr2sdr_params *params, int32_t form, void *stream) {
    HdrConst k;
    NUNIF_REQUIRE(src && dst && H > 0 && W > 0 && form >= HDR_FORM_U16 && form <= HDR_FORM_DEBUG, "hdr2sdr: bad argument");
    NUNIF_REQUIRE(H <= 8192 && W <= 8192, "hdr2sdr: H and W must not exceed 8192");
    NUNIF_REQUIRE(make_const(trc, colorspace, params, &k), "hdr2sdr: trc must be 16 (PQ) or 18 (HLG) and colorspace 709 or 601");
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)H * W;
    // 16-byte accesses: both pointers aligned, and for the planar form a plane stride of whole 16-byte pieces
    const bool vec = ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0) && (form != HDR_FORM_CHW || n % 4 == 0);
    ProfScope ps("hdr2sdr_kernel", s, 0.0, (double)n * (6.0 + (form == HDR_FORM_U16 ? 6.0 : 12.0)));
    if (trc == HDR_PQ) launch_form<HDR_PQ>(form, src, dst, n, vec, k, s);
    else launch_form<HDR_HLG>(form, src, dst, n, vec, k, s);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
