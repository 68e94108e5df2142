// Planar YUV <-> the model's CHW fp32 tensor on gfx950: the two pixel-format conversions of the video loop, one launch each.
//
// Reference: nunif/utils/video.py process_video.  Going in, input_reformatter :1025-1041 calls frame.reformat(**rgb24_options)
// :1038-1039 (options from guess_rgb24_options :621-640, source matrix / range from guess_colorspace :610-618 and
// guess_color_range :596-607) and to_tensor :218-223 uploads the rgb frame and divides by its maximum.  Coming out, to_frame
// :259-269 clamps and quantises to rgb24 / rgb48le and reformatter(new_frame) :1084 (built by configure_colorspace :763-854) turns
// that into --pix-fmt.  Both reformat calls are host libswscale on one thread, and the frame crosses PCIe as 3 (6) bytes per pixel
// each way where the decoder holds and the encoder wants 1.5 (3).  Here the planes are read (written) where they are — device
// memory or pinned host memory, zero-copy — at their own byte pitch, and the tensor is written (read) once.
//
// Formats: yuv420p, yuv444p (uint8) and yuv420p10le (uint16, 10 significant bits); a yuvj* format is the same layout with full
// range.  Matrix bt601 / bt709 / bt2020 non-constant-luminance, range limited or full.
//
// THIS IS NOT swscale'S ARITHMETIC, on purpose (as jpeg.hip is not libjpeg's): the coefficients are the ITU definitions in fp32,
// not fixed-point tables, and chroma is resampled for the MPEG-2 / H.264 default position (horizontally on the even luma column,
// vertically midway between the two rows) with the linear kernels that follow from it:
//   up    horizontally c[k] at x = 2k, 1/2 c[k] + 1/2 c[k+1] at x = 2k + 1; vertically 3/4 c[r] + 1/4 c[r-1] on row 2r and
//         3/4 c[r] + 1/4 c[r+1] on row 2r + 1; indices clamped at the edges.  Every weight is a power of two times 1 or 3 and the
//         codes have at most 16 bits, so the upsampled chroma is exact in fp32 whatever the order.
//   down  [1 2 1] / 4 horizontally, centred on the even column, then the mean of the two rows; indices clamped at the edges.
//   odd sizes have ceil(W / 2) x ceil(H / 2) chroma samples.
// In:  rgb = M (yuv - off), M and off from nunif_hip_pixfmt_constants, each row evaluated (m0 a + m1 b) + m2 c without FMA
//      (-ffp-contract=off), then clamped to [0, 1] (not in the debug form).
// Out: x clamped to [0, 1] as to_frame does; Y = ((m0 r + m1 g) + m2 b) + off; U, V likewise without the offset, filtered
//      (1/4 a + 1/2 b) + 1/4 c, 1/2 (row0 + row1), + off; code = floor(v + 1/2) (round half up), clamped to [0, 2^bits - 1].
// tests/pixfmt_ref.py restates exactly this, in float64 and in fp32.
//
// Shape: a lane owns 8 luma pixels of one row pair (2 x 8 luma, 4 chroma per plane at 4:2:0), so 4:2:0 is one pass.  Block
// (64, 4): 64 runs along x, 4 row pairs.  No LDS: the only reuse between lanes is the chroma neighbourhood on the way in (one
// column to the right, one row above and below) and one tensor column to the left on the way out — a few bytes next to lines
// the lane or its neighbour fetches anyway, served by the vector L1; staging a row pair in LDS would add a barrier and a second
// trip for nothing.  Luma moves as 8-byte (uint8) or 16-byte (uint16) accesses, the tensor as 16-byte ones.  A run that crosses
// the right edge, or the whole frame when a pointer / pitch / W does not allow the wide accesses, takes clamped one-sample
// accesses into the same registers: the arithmetic after the loads is shared, so the bits are too.  Pitch padding is never written.
#include "common.h"

namespace nunif {

enum { PF_420P8 = 0, PF_444P8 = 1, PF_420P10 = 2 };
enum { PF_FORM_CHW = 0, PF_FORM_DEBUG = 1 };
enum { PF_VEC = 1, PF_VEC_FRAME = 2 };

struct PixConst {
    float m[9];            // row major
    float off[3];          // code offsets: subtracted before M on the way in, added after M on the way out
    float maxc;            // 2^bits - 1
};

static bool make_const(int matrix, int full_range, int bits, int direction, PixConst *k) {
    double Kr, Kb;
    if (matrix == 601) { Kr = 0.299; Kb = 0.114; }
    else if (matrix == 709) { Kr = 0.2126; Kb = 0.0722; }
    else if (matrix == 2020) { Kr = 0.2627; Kb = 0.0593; }
    else return false;
    if ((bits != 8 && bits != 10) || (full_range != 0 && full_range != 1) || (direction != 0 && direction != 1)) return false;
    const double Kg = 1.0 - Kr - Kb, step = (double)(1 << (bits - 8)), top = (double)((1 << bits) - 1);
    const double sy = full_range ? top : 219.0 * step, sc = full_range ? top : 224.0 * step;
    const double yoff = full_range ? 0.0 : 16.0 * step, coff = 128.0 * step;
    double m[9];
    if (direction == 0) {                                   // yuv codes -> rgb in [0, 1]
        m[0] = 1.0 / sy; m[1] = 0.0;                                    m[2] = 2.0 * (1.0 - Kr) / sc;
        m[3] = 1.0 / sy; m[4] = -(2.0 * (1.0 - Kb) * Kb / Kg) / sc;     m[5] = -(2.0 * (1.0 - Kr) * Kr / Kg) / sc;
        m[6] = 1.0 / sy; m[7] = 2.0 * (1.0 - Kb) / sc;                  m[8] = 0.0;
    } else {                                                // rgb in [0, 1] -> yuv codes
        const double du = 2.0 * (1.0 - Kb), dv = 2.0 * (1.0 - Kr);
        m[0] = Kr * sy;              m[1] = Kg * sy;         m[2] = Kb * sy;
        m[3] = -Kr / du * sc;        m[4] = -Kg / du * sc;   m[5] = (1.0 - Kb) / du * sc;
        m[6] = (1.0 - Kr) / dv * sc; m[7] = -Kg / dv * sc;   m[8] = -Kb / dv * sc;
    }
    for (int i = 0; i < 9; ++i) k->m[i] = (float)m[i];
    k->off[0] = (float)yoff; k->off[1] = k->off[2] = (float)coff;
    k->maxc = (float)top;
    return true;
}

template <int FMT> struct Fmt {
    typedef uint8_t T;
    static constexpr bool SUB = FMT != PF_444P8;
    static constexpr int BITS = 8;
};
template <> struct Fmt<PF_420P10> {
    typedef uint16_t T;
    static constexpr bool SUB = true;
    static constexpr int BITS = 10;
};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// N consecutive samples at p (N = 4 or 8) in one access of N * sizeof(T) bytes
template <typename T, int N>
__device__ __forceinline__ void load_run(const uint8_t *p, float *v) {
    if (sizeof(T) == 1) {
        unsigned w[2];
        if (N == 8) { const u32x2 t = *(const u32x2 *)p; w[0] = t[0]; w[1] = t[1]; }
        else w[0] = *(const unsigned *)p;
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = (float)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
    } else {
        unsigned w[4];
        if (N == 8) { const u32x4 t = *(const u32x4 *)p; w[0] = t[0]; w[1] = t[1]; w[2] = t[2]; w[3] = t[3]; }
        else { const u32x2 t = *(const u32x2 *)p; w[0] = t[0]; w[1] = t[1]; }
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = (float)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
    }
}

template <typename T, int N>
__device__ __forceinline__ void store_run(uint8_t *p, const unsigned *c) {
    if (sizeof(T) == 1) {
        unsigned w[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < N; ++j) w[j >> 2] |= c[j] << (8 * (j & 3));
        if (N == 8) *(u32x2 *)p = (u32x2){w[0], w[1]};
        else *(unsigned *)p = w[0];
    } else {
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < N; ++j) w[j >> 1] |= c[j] << (16 * (j & 1));
        if (N == 8) *(u32x4 *)p = (u32x4){w[0], w[1], w[2], w[3]};
        else *(u32x2 *)p = (u32x2){w[0], w[1]};
    }
}

template <typename T>
__device__ __forceinline__ float load_one(const uint8_t *row, int x) { return (float)((const T *)row)[x]; }

// ---- planes -> tensor -----------------------------------------------------------------------------------------------------
// out [3][H][W] fp32.  frame (or null): HWC rgb24 (8-bit formats) / rgb48 (10-bit), rint(v * max) of the clamped value — what
// to_frame makes of `out`.  flags: PF_VEC the wide accesses on planes and tensor, PF_VEC_FRAME on the frame.
template <int FMT, int FORM, bool FRAME>
__global__ void __launch_bounds__(256)
yuv_to_tensor_kernel(const uint8_t *__restrict__ Y, const uint8_t *__restrict__ U, const uint8_t *__restrict__ V, long py, long pu,
                     long pv, float *__restrict__ out, uint8_t *__restrict__ frame, int H, int W, int flags, PixConst k) {
    typedef typename Fmt<FMT>::T T;
    constexpr bool SUB = Fmt<FMT>::SUB;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8, rp = blockIdx.y * 4 + threadIdx.y, y0 = rp * 2;
    if (x0 >= W || y0 >= H) return;
    const bool fast = (flags & PF_VEC) && x0 + 8 <= W;
    const int CW = SUB ? (W + 1) >> 1 : W, CH = SUB ? (H + 1) >> 1 : H;
    const int rows = imin(2, H - y0);

    // chroma neighbourhood at 4:2:0: rows rp - 1, rp, rp + 1 and columns cx0 .. cx0 + 4, clamped
    float cu[3][5], cv[3][5];
    if (SUB) {
        const int cx0 = x0 >> 1, cr[3] = {imax(rp - 1, 0), rp, imin(rp + 1, CH - 1)};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint8_t *ur = U + (long)cr[i] * pu, *vr = V + (long)cr[i] * pv;
            if (fast) {
                load_run<T, 4>(ur + cx0 * sizeof(T), cu[i]);
                load_run<T, 4>(vr + cx0 * sizeof(T), cv[i]);
                const int xe = imin(cx0 + 4, CW - 1);
                cu[i][4] = load_one<T>(ur, xe);
                cv[i][4] = load_one<T>(vr, xe);
            } else {
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const int xe = imin(cx0 + j, CW - 1);
                    cu[i][j] = load_one<T>(ur, xe);
                    cv[i][j] = load_one<T>(vr, xe);
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
        if (fast) load_run<T, 8>(yr + x0 * sizeof(T), ly);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) ly[j] = load_one<T>(yr, imin(x0 + j, W - 1));
        }
        if (SUB) {
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
        } else {
            const uint8_t *ur = U + (long)y * pu, *vr = V + (long)y * pv;
            if (fast) {
                load_run<T, 8>(ur + x0 * sizeof(T), u8);
                load_run<T, 8>(vr + x0 * sizeof(T), v8);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int xe = imin(x0 + j, W - 1);
                    u8[j] = load_one<T>(ur, xe);
                    v8[j] = load_one<T>(vr, xe);
                }
            }
        }
        float c[3][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = ly[j] - k.off[0], b = u8[j] - k.off[1], d = v8[j] - k.off[2];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                float v = (k.m[3 * e] * a + k.m[3 * e + 1] * b) + k.m[3 * e + 2] * d;
                if (FORM != PF_FORM_DEBUG) v = fminf(fmaxf(v, 0.f), 1.f);
                c[e][j] = v;
            }
        }
        float *o = out + (long)y * W + x0;
        if (fast) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                f32x4 *d = (f32x4 *)(o + e * hw);
                d[0] = (f32x4){c[e][0], c[e][1], c[e][2], c[e][3]};
                d[1] = (f32x4){c[e][4], c[e][5], c[e][6], c[e][7]};
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < W) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) o[e * hw + j] = c[e][j];
                }
        }
        if (FRAME) {
            const float maxv = sizeof(T) == 1 ? 255.0f : 65535.0f;
            unsigned q[24];                                                  // HWC
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int e = 0; e < 3; ++e) q[3 * j + e] = (unsigned)rintf(fminf(fmaxf(c[e][j], 0.f), 1.f) * maxv);
            uint8_t *f = frame + ((long)y * W + x0) * 3 * sizeof(T);
            if (fast && (flags & PF_VEC_FRAME)) {
#pragma unroll
                for (int t = 0; t < 3; ++t) store_run<T, 8>(f + t * 8 * sizeof(T), q + 8 * t);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (x0 + j < W) {
#pragma unroll
                        for (int e = 0; e < 3; ++e) ((T *)f)[3 * j + e] = (T)q[3 * j + e];
                    }
            }
        }
    }
}

// ---- tensor -> planes -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned quant_code(float v, float maxc) { return (unsigned)fminf(fmaxf(floorf(v + 0.5f), 0.f), maxc); }

template <int FMT>
__global__ void __launch_bounds__(256)
tensor_to_yuv_kernel(const float *__restrict__ x, uint8_t *__restrict__ Y, uint8_t *__restrict__ U, uint8_t *__restrict__ V, long py,
                     long pu, long pv, int H, int W, int flags, PixConst k) {
    typedef typename Fmt<FMT>::T T;
    constexpr bool SUB = Fmt<FMT>::SUB;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8, rp = blockIdx.y * 4 + threadIdx.y, y0 = rp * 2;
    if (x0 >= W || y0 >= H) return;
    const bool fast = (flags & PF_VEC) && x0 + 8 <= W;
    const long hw = (long)H * W;
    float hu[2][4], hv[2][4];                                                // 4:2:0: the horizontally filtered chroma of each row
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int y = imin(y0 + i, H - 1);                                   // odd H: the last pair is the last row twice
        const bool live = y0 + i < H;
        // columns x0 - 1 .. x0 + 7 (index j <-> column x0 - 1 + j), clamped
        float c[3][9];
        const float *r = x + (long)y * W;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float *re = r + e * hw;
            c[e][0] = re[imax(x0 - 1, 0)];
            if (fast) {
                const f32x4 a = *(const f32x4 *)(re + x0), b = *(const f32x4 *)(re + x0 + 4);
                c[e][1] = a[0]; c[e][2] = a[1]; c[e][3] = a[2]; c[e][4] = a[3];
                c[e][5] = b[0]; c[e][6] = b[1]; c[e][7] = b[2]; c[e][8] = b[3];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) c[e][1 + j] = re[imin(x0 + j, W - 1)];
            }
#pragma unroll
            for (int j = 0; j < 9; ++j) c[e][j] = fminf(fmaxf(c[e][j], 0.f), 1.f);
        }
        unsigned yq[8], uq[8], vq[8];
        float up[9], vp[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            up[j] = (k.m[3] * c[0][j] + k.m[4] * c[1][j]) + k.m[5] * c[2][j];
            vp[j] = (k.m[6] * c[0][j] + k.m[7] * c[1][j]) + k.m[8] * c[2][j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float yv = ((k.m[0] * c[0][j + 1] + k.m[1] * c[1][j + 1]) + k.m[2] * c[2][j + 1]) + k.off[0];
            yq[j] = quant_code(yv, k.maxc);
            if (!SUB) {
                uq[j] = quant_code(up[j + 1] + k.off[1], k.maxc);
                vq[j] = quant_code(vp[j + 1] + k.off[2], k.maxc);
            }
        }
        if (SUB) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                hu[i][t] = (0.25f * up[2 * t] + 0.5f * up[2 * t + 1]) + 0.25f * up[2 * t + 2];
                hv[i][t] = (0.25f * vp[2 * t] + 0.5f * vp[2 * t + 1]) + 0.25f * vp[2 * t + 2];
            }
        }
        if (live) {
            uint8_t *yr = Y + (long)y * py;
            if (fast) {
                store_run<T, 8>(yr + x0 * sizeof(T), yq);
                if (!SUB) {
                    store_run<T, 8>(U + (long)y * pu + x0 * sizeof(T), uq);
                    store_run<T, 8>(V + (long)y * pv + x0 * sizeof(T), vq);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (x0 + j < W) {
                        ((T *)yr)[x0 + j] = (T)yq[j];
                        if (!SUB) {
                            ((T *)(U + (long)y * pu))[x0 + j] = (T)uq[j];
                            ((T *)(V + (long)y * pv))[x0 + j] = (T)vq[j];
                        }
                    }
            }
        }
    }
    if (SUB) {
        const int cx0 = x0 >> 1, CW = (W + 1) >> 1;
        unsigned uq[4], vq[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uq[t] = quant_code(0.5f * (hu[0][t] + hu[1][t]) + k.off[1], k.maxc);
            vq[t] = quant_code(0.5f * (hv[0][t] + hv[1][t]) + k.off[2], k.maxc);
        }
        uint8_t *ur = U + (long)rp * pu, *vr = V + (long)rp * pv;
        if (fast) {
            store_run<T, 4>(ur + cx0 * sizeof(T), uq);
            store_run<T, 4>(vr + cx0 * sizeof(T), vq);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (cx0 + t < CW) {
                    ((T *)ur)[cx0 + t] = (T)uq[t];
                    ((T *)vr)[cx0 + t] = (T)vq[t];
                }
        }
    }
}

static bool aligned(const void *p, long pitch, long n) { return (uintptr_t)p % n == 0 && pitch % n == 0; }

// the wide accesses of one plane set: 8 luma samples and, at 4:2:0, 4 chroma samples per access
template <int FMT>
static bool planes_allow_vec(const nunif_pixfmt_planes *p) {
    const long s = sizeof(typename Fmt<FMT>::T), c = Fmt<FMT>::SUB ? 4 * s : 8 * s;
    return aligned(p->data[0], p->pitch[0], 8 * s) && aligned(p->data[1], p->pitch[1], c) && aligned(p->data[2], p->pitch[2], c);
}

template <int FMT>
static bool planes_valid(const nunif_pixfmt_planes *p, int W) {
    const long s = sizeof(typename Fmt<FMT>::T), cw = Fmt<FMT>::SUB ? (W + 1) / 2 : W;
    for (int i = 0; i < 3; ++i) {
        if (!p->data[i] || p->pitch[i] < (i == 0 ? W : cw) * s) return false;
        if ((uintptr_t)p->data[i] % s != 0 || p->pitch[i] % s != 0) return false;
    }
    return true;
}

static dim3 grid_for(int H, int W) { return dim3((unsigned)cdiv(cdiv(W, 8), 64), (unsigned)cdiv(cdiv(H, 2), 4)); }

template <int FMT>
static int launch_in(const nunif_pixfmt_planes *p, int H, int W, int form, float *dst, void *frame, const PixConst &k, hipStream_t s) {
    typedef typename Fmt<FMT>::T T;
    NUNIF_REQUIRE(planes_valid<FMT>(p, W), "yuv_to_tensor: a plane is null, misaligned for its sample size, or its pitch is "
                                           "smaller than its row");
    int flags = 0;
    if (planes_allow_vec<FMT>(p) && (uintptr_t)dst % 16 == 0 && W % 4 == 0) flags |= PF_VEC;
    if (frame && (uintptr_t)frame % (8 * sizeof(T)) == 0 && W % 8 == 0) flags |= PF_VEC_FRAME;
    const uint8_t *y = (const uint8_t *)p->data[0], *u = (const uint8_t *)p->data[1], *v = (const uint8_t *)p->data[2];
    const long py = p->pitch[0], pu = p->pitch[1], pv = p->pitch[2];
    const dim3 g = grid_for(H, W), b(64, 4);
    if (form == PF_FORM_DEBUG)
        yuv_to_tensor_kernel<FMT, PF_FORM_DEBUG, false><<<g, b, 0, s>>>(y, u, v, py, pu, pv, dst, nullptr, H, W, flags, k);
    else if (frame)
        yuv_to_tensor_kernel<FMT, PF_FORM_CHW, true><<<g, b, 0, s>>>(y, u, v, py, pu, pv, dst, (uint8_t *)frame, H, W, flags, k);
    else
        yuv_to_tensor_kernel<FMT, PF_FORM_CHW, false><<<g, b, 0, s>>>(y, u, v, py, pu, pv, dst, nullptr, H, W, flags, k);
    return NUNIF_HIP_OK;
}

template <int FMT>
static int launch_out(const float *src, int H, int W, const nunif_pixfmt_planes *p, const PixConst &k, hipStream_t s) {
    NUNIF_REQUIRE(planes_valid<FMT>(p, W), "tensor_to_yuv: a plane is null, misaligned for its sample size, or its pitch is "
                                           "smaller than its row");
    const int flags = planes_allow_vec<FMT>(p) && (uintptr_t)src % 16 == 0 && W % 4 == 0 ? PF_VEC : 0;
    tensor_to_yuv_kernel<FMT><<<grid_for(H, W), dim3(64, 4), 0, s>>>(src, (uint8_t *)p->data[0], (uint8_t *)p->data[1],
                                                                     (uint8_t *)p->data[2], p->pitch[0], p->pitch[1], p->pitch[2],
                                                                     H, W, flags, k);
    return NUNIF_HIP_OK;
}

static double plane_bytes(int format, int H, int W) {
    const double s = format == PF_420P10 ? 2.0 : 1.0, n = (double)H * W;
    return s * (format == PF_444P8 ? 3.0 * n : n + 2.0 * (double)((H + 1) / 2) * ((W + 1) / 2));
}

}  // namespace nunif

using namespace nunif;

extern "C" int nunif_hip_pixfmt_constants(int32_t matrix, int32_t full_range, int32_t bits, int32_t direction, float *coefficients,
                                          float *offsets) {
    PixConst k;
    NUNIF_REQUIRE(coefficients && offsets, "pixfmt_constants: bad argument");
    NUNIF_REQUIRE(make_const(matrix, full_range, bits, direction, &k),
                  "pixfmt_constants: matrix must be 601, 709 or 2020, full_range 0 or 1, bits 8 or 10, direction 0 or 1");
    for (int i = 0; i < 9; ++i) coefficients[i] = k.m[i];
    for (int i = 0; i < 3; ++i) offsets[i] = k.off[i];
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_yuv_to_tensor(const nunif_pixfmt_planes *src, int32_t format, int32_t H, int32_t W, int32_t matrix,
                                       int32_t full_range, int32_t form, float *dst, void *frame, void *stream) {
    PixConst k;
    NUNIF_REQUIRE(src && dst && H > 0 && W > 0, "yuv_to_tensor: bad argument");
    NUNIF_REQUIRE(H <= 8192 && W <= 8192, "yuv_to_tensor: H and W must not exceed 8192");
    NUNIF_REQUIRE(format >= PF_420P8 && format <= PF_420P10, "yuv_to_tensor: format must be 0 (yuv420p), 1 (yuv444p) or 2 (yuv420p10le)");
    NUNIF_REQUIRE(form == PF_FORM_CHW || (form == PF_FORM_DEBUG && !frame), "yuv_to_tensor: form must be 0 (chw) or 1 (debug, no frame)");
    NUNIF_REQUIRE(make_const(matrix, full_range, format == PF_420P10 ? 10 : 8, 0, &k),
                  "yuv_to_tensor: matrix must be 601, 709 or 2020 and full_range 0 or 1");
    hipStream_t s = (hipStream_t)stream;
    const double n = (double)H * W;
    ProfScope ps("yuv_to_tensor_kernel", s, 0.0, plane_bytes(format, H, W) + 12.0 * n + (frame ? (format == PF_420P10 ? 6.0 : 3.0) * n : 0.0));
    int rc;
    if (format == PF_420P8) rc = launch_in<PF_420P8>(src, H, W, form, dst, frame, k, s);
    else if (format == PF_444P8) rc = launch_in<PF_444P8>(src, H, W, form, dst, frame, k, s);
    else rc = launch_in<PF_420P10>(src, H, W, form, dst, frame, k, s);
    if (rc != NUNIF_HIP_OK) return rc;
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_tensor_to_yuv(const float *src, int32_t H, int32_t W, int32_t format, int32_t matrix, int32_t full_range,
                                       const nunif_pixfmt_planes *dst, void *stream) {
    PixConst k;
    NUNIF_REQUIRE(src && dst && H > 0 && W > 0, "tensor_to_yuv: bad argument");
    NUNIF_REQUIRE(H <= 8192 && W <= 8192, "tensor_to_yuv: H and W must not exceed 8192");
    NUNIF_REQUIRE(format >= PF_420P8 && format <= PF_420P10, "tensor_to_yuv: format must be 0 (yuv420p), 1 (yuv444p) or 2 (yuv420p10le)");
    NUNIF_REQUIRE(make_const(matrix, full_range, format == PF_420P10 ? 10 : 8, 1, &k),
                  "tensor_to_yuv: matrix must be 601, 709 or 2020 and full_range 0 or 1");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps("tensor_to_yuv_kernel", s, 0.0, plane_bytes(format, H, W) + 12.0 * (double)H * W);
    int rc;
    if (format == PF_420P8) rc = launch_out<PF_420P8>(src, H, W, dst, k, s);
    else if (format == PF_444P8) rc = launch_out<PF_444P8>(src, H, W, dst, k, s);
    else rc = launch_out<PF_420P10>(src, H, W, dst, k, s);
    if (rc != NUNIF_HIP_OK) return rc;
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
