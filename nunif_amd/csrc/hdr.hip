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
//
// The map itself (map_pixel and what it calls, the constants) and the stores of the three forms live in hdr_map.h, shared with
// hdr_planes.hip, which feeds the same map from the decoder's yuv420p10le planes.
#include "hdr_map.h"

namespace nunif {

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
    store_pixels8<FORM>(dst, i * 8, n, v);
}

// one pixel per lane over pixels [first, n)
template <int TRC, int FORM>
__global__ void __launch_bounds__(256)
hdr2sdr_px_kernel(const uint16_t *__restrict__ src, void *__restrict__ dst, long first, long n, HdrConst k) {
    const long i = first + (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[3];
    map_pixel<TRC>(src[i * 3], src[i * 3 + 1], src[i * 3 + 2], k, v);
    store_pixel<FORM>(dst, i, n, v);
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
