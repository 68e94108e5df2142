// What the fp32 implicit-GEMM kernels (tn_gemm of transnetv2.hip, sp_gemm of superpoint.hip) and the fp32 MFMA helpers of
// outpaint.hip share: C = A * B on v_mfma_f32_32x32x2_f32 with exact fp32 operands, a k-ordered fmaf chain per output element
// that tn_gemm / sp_gemm close every kFlush k.  Device-only.
//
// The main loop itself (two LDS stages, the MFMA inner loop, the acc / tot chain) is NOT here: it is written out in tn_gemm and
// in sp_gemm, the same statements twice.  As a shared __forceinline__ function hipcc compiled it differently in every kernel
// and TransNetV2's window ran 2 % slower (profiles/gemm_f32_core_timing.txt).  A change to the chain is made in both kernels.
#pragma once
#include "common.h"

#if defined(__HIPCC__)
namespace nunif {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBK = 16;          // k per LDS stage
constexpr int kPad = 4;          // LDS row padding (floats)
constexpr int kFlush = 128;      // k per accumulation chain

__device__ __forceinline__ f32x16 zero16() {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
    return v;
}

// The accumulator map of a 32 x 32 tile: register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
// Registers 4g .. 4g + 3 of a lane are therefore four consecutive rows.
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ---- rows of the A tile ---------------------------------------------------------------------------------------------------------

// One row of the A tile as its loader thread sees it; a row past M loads zeros (ok == 0).
struct RowInfo { long long base; int h, w, ok; };

// row m of a row-major matrix: base = offset of its first float
__device__ __forceinline__ RowInfo row_plain(int m, int M, int lda) {
    RowInfo r;
    r.ok = m < M;
    if (!r.ok) m = 0;
    r.base = (long long)m * lda; r.h = 0; r.w = 0;
    return r;
}

// rows ordered (image, h, w) over H x W images: base = image
__device__ __forceinline__ RowInfo row_conv(int m, int M, int H, int W) {
    RowInfo r;
    r.ok = m < M;
    if (!r.ok) m = 0;
    const int hw = H * W, b = m / hw, p = m - b * hw;
    r.h = p / W; r.w = p - r.h * W; r.base = b;
    return r;
}

// ---- the tile ----------------------------------------------------------------------------------------------------------------

// 4 waves as WM x WN, each TM x TN tiles of 32 x 32.  LDS holds both operand tiles k-major ([k][row], rows padded by kPad) so that
// an MFMA operand is one conflict-free ds_read_b32.  A loader thread owns row (tid >> 2) + 64 pass and 4 k; BM == 32 has one pass
// that only the first 128 threads take part in.
template <int WM, int WN, int TM, int TN>
struct GemmTile {
    static constexpr int BM = WM * TM * 32, BN = WN * TN * 32, LDA = BM + kPad, LDB = BN + kPad;
    static_assert(WM * WN == 4 && (BM % 64 == 0 || BM == 32), "tile shape");
    static constexpr int APASS = BM >= 64 ? BM / 64 : 1, BVEC = kBK * BN / 4, BPASS = (BVEC + 255) / 256;
    static constexpr int A_STAGE = kBK * LDA, B_STAGE = kBK * LDB;       // floats of one LDS stage of each operand
};

}  // namespace nunif
#endif
