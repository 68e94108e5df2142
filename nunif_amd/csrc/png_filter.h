// The first launch of the PNG frame encoder (png.hip): quantise a row and filter it.  One template, instantiated per pixel form:
// png.hip holds the forms with one source pointer (0..2), png_planes.hip those that take their colour and alpha planes apart
// (4..6), each file with the launcher of its own instantiations.
#pragma once
#include "common.h"
#include "png_host.h"

namespace nunif {
namespace png_dev {

using namespace png;

constexpr int kThreads = 256;

struct Frame {
    int B, H, W, form, bpp, stripe_rows, stripes;
    long row, stripe_stride;
};

// ---- quantise, filter ----------------------------------------------------------------------------------------------------------------
struct Px {
    int c[4];
};

// The planar fp32 sources of forms 4..6: colour [B][channels][H][W] (channels 1 or 3) and alpha [B][1][H][W], each with its own
// distance between frames (in floats), so that a caller's two tensors and one tensor that holds both are the same to the kernel.
struct Planes {
    const float *alpha;
    long colour_stride, alpha_stride;
    int channels;
};

// quantize256 (nunif/transforms/functional.py:9-12, reference): x 255, round half to even, clamp
__device__ __forceinline__ int quantise8(float v) { return (int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

template <int FORM>
__device__ __forceinline__ Px load_px(const void *src, const Planes &pl, long b, int y, int x, int H, int W) {
    Px p;
    if (x < 0 || y < 0) {
        p.c[0] = p.c[1] = p.c[2] = p.c[3] = 0;
        return p;
    }
    p.c[3] = 0;
    if (FORM == kRgba8F32 || FORM == kGray8F32 || FORM == kGrayA8F32) {
        const long at = (long)y * W + x, plane = (long)H * W;
        const float *f = static_cast<const float *>(src) + b * pl.colour_stride + at;
        if (FORM == kRgba8F32) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p.c[k] = quantise8(f[k * plane]);
        } else {
            // three planes: the bytes first, then PIL's Image.convert("L") on them (pil_io.py:287-291 save_image, reference)
            if (pl.channels == 3) {
                const int r = quantise8(f[0]), g = quantise8(f[plane]), bl = quantise8(f[2 * plane]);
                p.c[0] = (19595 * r + 38470 * g + 7471 * bl + 0x8000) >> 16;
            } else {
                p.c[0] = quantise8(f[0]);
            }
            p.c[1] = p.c[2] = 0;
        }
        if (FORM == kRgba8F32) p.c[3] = quantise8(pl.alpha[b * pl.alpha_stride + at]);
        if (FORM == kGrayA8F32) p.c[1] = quantise8(pl.alpha[b * pl.alpha_stride + at]);
    } else if (FORM == kRgb8F32) {
        const float *f = static_cast<const float *>(src) + (b * 3 * H + y) * (long)W + x;
#pragma unroll
        for (int k = 0; k < 3; ++k) p.c[k] = (int)rintf(fminf(fmaxf(f[(long)k * H * W], 0.f), 1.f) * 255.f);
    } else if (FORM == kRgb8U8) {
        const uint8_t *u = static_cast<const uint8_t *>(src) + ((b * H + y) * (long)W + x) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) p.c[k] = u[k];
    } else {
        const float d = static_cast<const float *>(src)[(b * H + y) * (long)W + x];
        const unsigned v = (unsigned)(65535.f * fminf(fmaxf(d, 0.f), 1.f));
        p.c[0] = (int)(v >> 8);
        p.c[1] = (int)(v & 255u);
        p.c[2] = 0;
    }
    return p;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int filtered(int type, int x, int a, int b, int c) {
    int pred = 0;
    if (type == 1) pred = a;
    else if (type == 2) pred = b;
    else if (type == 3) pred = (a + b) >> 1;
    else if (type == 4) pred = paeth(a, b, c);
    return (x - pred) & 255;
}
__device__ __forceinline__ int signed_abs(int v) { return v < 128 ? v : 256 - v; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// out: the filtered bytes; row r of frame b at out + b * frame_stride + (r / stripe_rows) * stripe_stride + (r % stripe_rows) * row
template <int FORM>
__global__ void __launch_bounds__(kThreads) png_filter_kernel(const void *__restrict__ src, const Planes pl,
                                                               uint8_t *__restrict__ out, uint32_t *__restrict__ rowsum,
                                                               const Frame f, long frame_stride) {
    constexpr int BPP = FORM == kRgba8F32 ? 4 : FORM == kGray8F32 ? 1 : (FORM == kGray16F32 || FORM == kGrayA8F32) ? 2 : 3;
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const long b = blockIdx.y;
    if (r >= f.H) return;
    int cost[5] = {0, 0, 0, 0, 0};
    for (int x = lane; x < f.W; x += 64) {
        const Px cur = load_px<FORM>(src, pl, b, r, x, f.H, f.W), left = load_px<FORM>(src, pl, b, r, x - 1, f.H, f.W);
        const Px up = load_px<FORM>(src, pl, b, r - 1, x, f.H, f.W);
        const Px ul = load_px<FORM>(src, pl, b, r - 1, r > 0 ? x - 1 : -1, f.H, f.W);
#pragma unroll
        for (int k = 0; k < BPP; ++k)
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += signed_abs(filtered(t, cur.c[k], left.c[k], up.c[k], ul.c[k]));
    }
    int best = 0, best_cost = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int c = wave_sum(cost[t]);
        if (t == 0 || c < best_cost) {                           // the lowest type on a tie
            best = t;
            best_cost = c;
        }
    }
    uint8_t *dst = out + b * frame_stride + (long)(r / f.stripe_rows) * f.stripe_stride + (long)(r % f.stripe_rows) * f.row;
    unsigned long long sa = 0, sb = 0;                           // sum of d[i] and of (row - i) d[i]
    if (lane == 0) {
        dst[0] = (uint8_t)best;
        sa = (unsigned)best;
        sb = (unsigned long long)f.row * (unsigned)best;
    }
    for (int x = lane; x < f.W; x += 64) {
        const Px cur = load_px<FORM>(src, pl, b, r, x, f.H, f.W), left = load_px<FORM>(src, pl, b, r, x - 1, f.H, f.W);
        const Px up = load_px<FORM>(src, pl, b, r - 1, x, f.H, f.W);
        const Px ul = load_px<FORM>(src, pl, b, r - 1, r > 0 ? x - 1 : -1, f.H, f.W);
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < BPP; ++k) {
            const long i = 1 + (long)x * BPP + k;
            const int v = filtered(best, cur.c[k], left.c[k], up.c[k], ul.c[k]);
            if (BPP == 4) word |= (uint32_t)v << (8 * k);
            else dst[i] = (uint8_t)v;
            sa += (unsigned)v;
            sb += (unsigned long long)(f.row - i) * (unsigned)v;
        }
        // a pixel of four bytes is one store; it starts behind the row's filter type, so it is aligned to a byte only
        if (BPP == 4) __builtin_memcpy(dst + 1 + (long)x * 4, &word, 4);
    }
    if (rowsum) {
        sa = wave_sum64(sa);
        sb = wave_sum64(sb);
        if (lane == 0) {
            rowsum[(b * f.H + r) * 2] = (uint32_t)(sa % 65521u);
            rowsum[(b * f.H + r) * 2 + 1] = (uint32_t)(sb % 65521u);
        }
    }
}

// png_planes.hip: the filter launch of forms 4..6
int launch_filter_planes(const void *src, const Planes &pl, const Frame &f, uint8_t *filt, uint32_t *rowsum, long frame_stride,
                         hipStream_t s);

}  // namespace png_dev
}  // namespace nunif
