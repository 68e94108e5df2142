// HDR video enters as YUV planes: yuv420p10le planes (BT.2020 non-constant luminance, PQ or HLG) -> the tone-mapped SDR frame on
// gfx950, one kernel, one pass over the planes.
//
// Reference: nunif/utils/video.py hdr2sdr :309-416.  Its first step is frame.to_ndarray(format="rgb48le") (:322-325) — host
// libswscale on one thread turns the decoder's planes into a 6 B/px rgb48 frame (the reference asserts colorspace == BT2020, :318)
// — then the map of :327-398, then to_tensor (:218-223).  hdr.hip does the map from that rgb48 frame; this file does it from the
// planes the decoder holds (3 B/px), so the rgb48 frame is neither made on the host, nor carried across PCIe, nor written and read
// again on the device.
//
// Nothing here is new arithmetic.  Per pixel, in this order:
//   1. linear chroma upsampling, then rgb = M (yuv - off) with the bt2020 constants of nunif_hip_pixfmt_constants (called for
//      them, not copied), each row (m0 a + m1 b) + m2 c without FMA, clamped to [0, 1]: what
//      yuv_to_tensor_kernel<PF_420P10, chw> of pixfmt.hip computes;
//   2. code = (unsigned)rintf(v * 65535.0f): the rgb48 code that kernel's side frame holds, and the intermediate the reference's
//      route has too;
//   3. map_pixel<TRC> of hdr_map.h, as hdr.hip calls it;
//   4. the three output forms of nunif_hip_hdr2sdr through the stores of hdr_map.h: u16 HWC trunc(v * 65535), chw fp32
//      float(trunc(v * 65535)) / 65535, debug HWC fp32 v.
// So the launch is bit-equal to nunif_hip_yuv_to_tensor(frame = rgb48) followed by nunif_hip_hdr2sdr (tests/test_gpu_hdr_planes.py
// holds it to that over every case), and each half stays pinned against float64 by its own tests.
//
// Steps 3 and 4 are shared code: the map and the stores were moved out of hdr.hip into hdr_map.h.  Step 1, THE PLANE GATHER, IS
// RESTATED here (namespace hdr_planes, for the one 16-bit 4:2:0 format) and not shared with pixfmt.hip: moving it into a header
// that both include changed the register allocation of pixfmt.hip's own kernels (66 -> 80 VGPRs for yuv420p, 71 -> 90 with the
// side frame, past the budget of tests/test_isa_pixfmt.py) although the source was the same.  The bit-equality test above is
// what guards the restatement.
//
// Shape: that of yuv_to_tensor_kernel.  Block (64, 4); a lane owns 8 luma pixels of one row pair and the 3 x 5 chroma neighbourhood
// of each chroma plane; no LDS, no atomics, fp32.  16-byte luma loads, 8-byte chroma runs plus the one neighbour, 16-byte stores.
// One row of the pair at a time: the live state is the chroma neighbourhood plus the row's 24 values.  A run that crosses the right
// edge, or the whole frame when a pointer / pitch does not allow the wide loads, takes clamped one-sample loads into the same
// registers; likewise one-pixel stores where the destination or W does not allow the 16-byte ones.  The arithmetic between is
// shared, so the bits are too.  Planes are read where they are — device memory or pinned host memory, zero-copy — at their own
// byte pitch; padding is never read past a row's samples and nothing but the H x W pixels of dst is written.
#include "hdr_map.h"

namespace nunif {

enum { HP_VEC_IN = 1, HP_VEC_OUT = 2 };

struct PlanesConst {
    float m[9];            // yuv codes -> rgb in [0, 1], row major
    float off[3];          // code offsets, subtracted before M
};

namespace hdr_planes {

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// N consecutive uint16 samples at p (N = 4 or 8) in one access of 2 N bytes
template <int N>
__device__ __forceinline__ void load_run(const uint8_t *p, float *v) {
    unsigned w[4];
    if (N == 8) { const u32x4 t = *(const u32x4 *)p; w[0] = t[0]; w[1] = t[1]; w[2] = t[2]; w[3] = t[3]; }
    else { const u32x2 t = *(const u32x2 *)p; w[0] = t[0]; w[1] = t[1]; }
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (float)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
}

__device__ __forceinline__ float load_one(const uint8_t *row, int x) { return (float)((const uint16_t *)row)[x]; }

}  // namespace hdr_planes

template <int TRC, int FORM>
__global__ void __launch_bounds__(256)
yuv_hdr_to_tensor_kernel(const uint8_t *__restrict__ Y, const uint8_t *__restrict__ U, const uint8_t *__restrict__ V, long py, long pu,
                         long pv, void *__restrict__ dst, int H, int W, int flags, PlanesConst k, HdrConst hk) {
    using namespace hdr_planes;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8, rp = blockIdx.y * 4 + threadIdx.y, y0 = rp * 2;
    if (x0 >= W || y0 >= H) return;
    const bool whole = x0 + 8 <= W, fast_in = (flags & HP_VEC_IN) && whole, fast_out = (flags & HP_VEC_OUT) && whole;
    const int CW = (W + 1) >> 1, CH = (H + 1) >> 1;
    const int rows = imin(2, H - y0);

    // chroma neighbourhood: rows rp - 1, rp, rp + 1 and columns cx0 .. cx0 + 4, clamped
    float cu[3][5], cv[3][5];
    {
        const int cx0 = x0 >> 1, cr[3] = {imax(rp - 1, 0), rp, imin(rp + 1, CH - 1)};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint8_t *ur = U + (long)cr[i] * pu, *vr = V + (long)cr[i] * pv;
            if (fast_in) {
                load_run<4>(ur + cx0 * 2, cu[i]);
                load_run<4>(vr + cx0 * 2, cv[i]);
                const int xe = imin(cx0 + 4, CW - 1);
                cu[i][4] = load_one(ur, xe);
                cv[i][4] = load_one(vr, xe);
            } else {
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int xe = imin(cx0 + j, CW - 1);
                    cu[i][j] = load_one(ur, xe);
                    cv[i][j] = load_one(vr, xe);
                }
            }
        }
    }
    const long hw = (long)H * W;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (i >= rows) break;
        const int y = y0 + i;
        float ly[8], u8[8], v8[8];
        const uint8_t *yr = Y + (long)y * py;
        if (fast_in) load_run<8>(yr + x0 * 2, ly);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) ly[j] = load_one(yr, imin(x0 + j, W - 1));
        }
        const int o = i == 0 ? 0 : 2;
        float uvert[5], vvert[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            uvert[j] = 0.75f * cu[1][j] + 0.25f * cu[o][j];
            vvert[j] = 0.75f * cv[1][j] + 0.25f * cv[o][j];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            u8[2 * t] = uvert[t];
            v8[2 * t] = vvert[t];
            u8[2 * t + 1] = 0.5f * uvert[t] + 0.5f * uvert[t + 1];
            v8[2 * t + 1] = 0.5f * vvert[t] + 0.5f * vvert[t + 1];
        }
        float v[24];                                                         // HWC: v[3 * pixel + channel]
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = ly[j] - k.off[0], b = u8[j] - k.off[1], d = v8[j] - k.off[2];
            unsigned q[3];                                                   // the rgb48 codes of the two-launch chain
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float c = (k.m[3 * e] * a + k.m[3 * e + 1] * b) + k.m[3 * e + 2] * d;
                q[e] = (unsigned)rintf(fminf(fmaxf(c, 0.f), 1.f) * 65535.0f);
            }
            map_pixel<TRC>(q[0], q[1], q[2], hk, v + 3 * j);
        }
        const long p = (long)y * W + x0;
        if (fast_out) store_pixels8<FORM>(dst, p, hw, v);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < W) store_pixel<FORM>(dst, p + j, hw, v + 3 * j);
        }
    }
}

static bool aligned(const void *p, long pitch, long n) { return (uintptr_t)p % n == 0 && pitch % n == 0; }

// every plane there, aligned for uint16 samples, and its pitch not shorter than its row
static bool planes_valid(const nunif_pixfmt_planes *p, int W) {
    for (int i = 0; i < 3; ++i) {
        if (!p->data[i] || p->pitch[i] < (long)(i == 0 ? W : (W + 1) / 2) * 2) return false;
        if (!aligned(p->data[i], p->pitch[i], 2)) return false;
    }
    return true;
}

template <int TRC, int FORM>
static void launch(const nunif_pixfmt_planes *p, void *dst, int H, int W, int flags, const PlanesConst &k, const HdrConst &hk,
                   hipStream_t s) {
    yuv_hdr_to_tensor_kernel<TRC, FORM><<<dim3((unsigned)cdiv(cdiv(W, 8), 64), (unsigned)cdiv(cdiv(H, 2), 4)), dim3(64, 4), 0, s>>>(
        (const uint8_t *)p->data[0], (const uint8_t *)p->data[1], (const uint8_t *)p->data[2], p->pitch[0], p->pitch[1], p->pitch[2],
        dst, H, W, flags, k, hk);
}

template <int TRC>
static void launch_form(int form, const nunif_pixfmt_planes *p, void *dst, int H, int W, int flags, const PlanesConst &k,
                        const HdrConst &hk, hipStream_t s) {
    if (form == HDR_FORM_U16) launch<TRC, HDR_FORM_U16>(p, dst, H, W, flags, k, hk, s);
    else if (form == HDR_FORM_CHW) launch<TRC, HDR_FORM_CHW>(p, dst, H, W, flags, k, hk, s);
    else launch<TRC, HDR_FORM_DEBUG>(p, dst, H, W, flags, k, hk, s);
}

}  // namespace nunif

using namespace nunif;

extern "C" int nunif_hip_yuv_hdr_to_tensor(const nunif_pixfmt_planes *src, int32_t format, int32_t H, int32_t W, int32_t full_range,
                                           int32_t trc, int32_t colorspace, const nunif_hdr2sdr_params *params, int32_t form,
                                           void *dst, void *stream) {
    PlanesConst k;
    HdrConst hk;
    NUNIF_REQUIRE(src && dst && H > 0 && W > 0 && form >= HDR_FORM_U16 && form <= HDR_FORM_DEBUG, "yuv_hdr_to_tensor: bad argument");
    NUNIF_REQUIRE(H <= 8192 && W <= 8192, "yuv_hdr_to_tensor: H and W must not exceed 8192");
    NUNIF_REQUIRE(format == 2, "yuv_hdr_to_tensor: format must be 2 (yuv420p10le)");
    NUNIF_REQUIRE(make_const(trc, colorspace, params, &hk),
                  "yuv_hdr_to_tensor: trc must be 16 (PQ) or 18 (HLG) and colorspace 709 or 601");
    NUNIF_REQUIRE(planes_valid(src, W), "yuv_hdr_to_tensor: a plane is null, misaligned for its sample size, or its pitch is "
                                        "smaller than its row");
    // the matrix is bt2020 by definition (video.py:318); the constants are pixfmt.hip's own
    if (nunif_hip_pixfmt_constants(2020, full_range, 10, 0, k.m, k.off) != NUNIF_HIP_OK) return NUNIF_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // the wide loads: 8 luma samples (16 bytes) and 4 chroma samples (8 bytes) per access
    int flags = aligned(src->data[0], src->pitch[0], 16) && aligned(src->data[1], src->pitch[1], 8) &&
                        aligned(src->data[2], src->pitch[2], 8) ? HP_VEC_IN : 0;
    // 16-byte stores: a row's first pixel of a run lands on a 16-byte boundary of dst (hdr_map.h, store_pixels8)
    if ((uintptr_t)dst % 16 == 0 && W % (form == HDR_FORM_U16 ? 8 : 4) == 0) flags |= HP_VEC_OUT;
    const double n = (double)H * W, planes = 2.0 * (n + 2.0 * (double)((H + 1) / 2) * ((W + 1) / 2));
    ProfScope ps("yuv_hdr_to_tensor_kernel", s, 0.0, planes + (form == HDR_FORM_U16 ? 6.0 : 12.0) * n);
    if (trc == HDR_PQ) launch_form<HDR_PQ>(form, src, dst, H, W, flags, k, hk, s);
    else launch_form<HDR_HLG>(form, src, dst, H, W, flags, k, hk, s);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
