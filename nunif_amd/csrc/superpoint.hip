// SuperPoint (nunif/utils/superpoint.py, reference) for gfx950: the network, keypoint extraction, descriptor sampling, descriptor
// matching and the stabiliser's affine warp, fp32 throughout.
//
// stlizer thresholds the score map and takes an argmax over descriptor similarities, so operands and accumulation stay fp32: the
// 3x3 and 1x1 convolutions are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32 inputs, a k-ordered fmaf chain per output
// element, closed every 128 k as DESIGN.md 4.24 found necessary for TransNetV2).
//
// Activations are channels-last [image][h][w][c].  A VGG block is conv -> ReLU -> BatchNorm (superpoint.py:55-71), so the BN of
// the eight backbone and two 3x3 head convs is a per-channel scale / shift AFTER the ReLU (epilogue), not a fold.  A conv that is
// followed by MaxPool2d(2, 2) orders its rows (image, pooled pixel, 2x2 corner): registers 4g..4g+3 of a lane are the four corners
// of one window, the max is the epilogue and the rows the floor drops are never computed.  The two 1x1 head convs have no ReLU,
// their BN is folded on the host; the detector's softmax + dustbin drop + depth-to-space and the descriptor's L2 norm are their
// epilogues (through an LDS tile that re-uses the operand stages).
#include <string>
#include <vector>

#include "gemm_f32.h"
#include "host_weights.h"

namespace nunif {
namespace {

constexpr int kCell = 8;         // stride of the net: one 65-way softmax per 8 x 8 cell

enum { A_PLAIN = 0, A_CONV = 1, A_CONV_POOL = 2 };
enum { E_BN = 0, E_BN_POOL = 1, E_DET = 2, E_DESC = 3 };

struct GemmArgs {
    const float *A, *Bm, *bias, *scale, *shift;
    float *out;
    int M, N, K;                 // valid rows / output columns / k (B is zero padded to a multiple of BN columns)
    int lda, ldb, ldo;           // A_PLAIN: floats per row of A; row strides of B and out
    int H, W, C;                 // conv: input image and channels; E_DET: cells per image (h, w)
    int Hp, Wp;                  // pooled geometry
};

template <int AMODE>
__device__ __forceinline__ RowInfo row_info(const GemmArgs &g, int m) {
    if (AMODE == A_PLAIN) return row_plain(m, g.M, g.lda);
    if (AMODE == A_CONV) return row_conv(m, g.M, g.H, g.W);
    // rows ordered (image, pooled pixel, 2x2 corner): (h, w) is the full-resolution pixel of corner m & 3
    RowInfo r;
    r.ok = m < g.M;
    if (!r.ok) m = 0;
    const int q = m & 3, mp = m >> 2, pp = g.Hp * g.Wp, b = mp / pp, p = mp - b * pp, ph = p / g.Wp, pw = p - ph * g.Wp;
    r.h = 2 * ph + (q >> 1); r.w = 2 * pw + (q & 1); r.base = b;
    return r;
}

// Four consecutive k of row r starting at k (k % 4 == 0; C % 4 == 0, so the four lie inside one tap).  B is not zero padded
// in k here, so k >= K loads zeros.
template <int AMODE>
__device__ __forceinline__ f32x4 load_a(const GemmArgs &g, const RowInfo &r, int k) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!r.ok || k >= g.K) return v;
    if (AMODE == A_PLAIN) {
        v = *reinterpret_cast<const f32x4 *>(g.A + r.base + k);
    } else {
        const int tap = k / g.C, c = k - tap * g.C, dh = tap / 3, hh = r.h + dh - 1, ww = r.w + (tap - dh * 3) - 1;
        if (hh >= 0 && hh < g.H && ww >= 0 && ww < g.W)
            v = *reinterpret_cast<const f32x4 *>(g.A + ((r.base * g.H + hh) * g.W + ww) * g.C + c);
    }
    return v;
}

// C[M][N] = A[M][K] * B[K][N] on v_mfma_f32_32x32x2_f32.  4 waves as WM x WN, each TM x TN tiles of 32 x 32.  A comes through
// load_a (implicit im2col), B is a plain row-major matrix.  LDS holds both tiles k-major so that an MFMA operand is one
// conflict-free ds_read_b32; two LDS stages and a register stage hide the global loads.  tn_gemm of transnetv2.hip holds the same
// loop (gemm_f32.h says why it is written twice): change both.
template <int AMODE, int EMODE, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void sp_gemm(const GemmArgs g) {
    typedef GemmTile<WM, WN, TM, TN> Tile;
    constexpr int BM = Tile::BM, BN = Tile::BN, LDA = Tile::LDA, LDB = Tile::LDB;
    constexpr int AP = Tile::APASS, BVEC = Tile::BVEC, BPASS = Tile::BPASS;
    constexpr int STAGES = 2 * (Tile::A_STAGE + Tile::B_STAGE), TILE = (EMODE == E_DET || EMODE == E_DESC) ? BM * (BN + 1) : 0;
    constexpr int SMEM = STAGES > TILE ? STAGES : TILE;
    static_assert(SMEM * 4 <= 65536, "LDS");
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    __shared__ float rown[BM];
    float *As = smem, *Bs = smem + 2 * Tile::A_STAGE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    // A loader: thread -> (row arow, 4 k starting at kq); BM == 32 uses the first 128 threads only
    const int kq = (tid & 3) * 4, arow = tid >> 2;
    const bool aload = BM >= 64 || arow < BM;
    RowInfo rows[AP];
#pragma unroll
    for (int p = 0; p < AP; ++p) rows[p] = row_info<AMODE>(g, m0 + p * 64 + arow);

    f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; tot[i][j][r] = 0.f; }

    f32x4 ra[AP], rb[BPASS];
    const int nk = (g.K + kBK - 1) / kBK;

    auto gload = [&](int kt) {
#pragma unroll
        for (int p = 0; p < AP; ++p)
            if (aload) ra[p] = load_a<AMODE>(g, rows[p], kt * kBK + kq);
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + p * 256;
            if (BVEC % 256 == 0 || idx < BVEC) {
                const int kr = idx / (BN / 4), nc = (idx - kr * (BN / 4)) * 4;
                rb[p] = *reinterpret_cast<const f32x4 *>(g.Bm + (long long)(kt * kBK + kr) * g.ldb + n0 + nc);
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int p = 0; p < AP; ++p)
            if (aload)
#pragma unroll
                for (int i = 0; i < 4; ++i) As[buf * kBK * LDA + (kq + i) * LDA + p * 64 + arow] = ra[p][i];
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + p * 256;
            if (BVEC % 256 == 0 || idx < BVEC) {
                const int kr = idx / (BN / 4), nc = (idx - kr * (BN / 4)) * 4;
                *reinterpret_cast<f32x4 *>(&Bs[buf * kBK * LDB + kr * LDB + nc]) = rb[p];
            }
        }
    };

    gload(0);
    lstore(0);
    __syncthreads();
    const int lk = lane >> 5, lr = lane & 31;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
        for (int kk = 0; kk < kBK; kk += 2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[cur * kBK * LDA + (kk + lk) * LDA + (wm * TM + i) * 32 + lr];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[cur * kBK * LDB + (kk + lk) * LDB + (wn * TN + j) * 32 + lr];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if ((kt + 1) % (kFlush / kBK) == 0 || kt + 1 == nk) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                }
        }
        if (kt + 1 < nk) lstore(cur ^ 1);
        __syncthreads();
    }

    // acc_row() of gemm_f32.h, spelled out (through the function the epilogues compile to other code): registers 4 q4 .. 4 q4 + 3
    // of a lane are rows 8 q4 + 4 lk .. + 3 of the 32 x 32 tile
    if (EMODE == E_BN || EMODE == E_BN_POOL) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + (wn * TN + j) * 32 + lr;
                if (n >= g.N) continue;
                const int mb = m0 + (wm * TM + i) * 32 + 4 * lk;
                const float bias = g.bias[n], sc = g.scale[n], sh = g.shift[n];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int m = mb + 8 * q4;                     // rows m .. m+3 are registers 4 q4 .. 4 q4 + 3
                    if (EMODE == E_BN_POOL) {
                        if (m >= g.M) continue;                    // M % 4 == 0: a window is inside or outside as a whole
                        float v = -INFINITY;
#pragma unroll
                        for (int q = 0; q < 4; ++q) v = fmaxf(v, fmaf(fmaxf(tot[i][j][4 * q4 + q] + bias, 0.f), sc, sh));
                        g.out[(long long)(m >> 2) * g.ldo + n] = v;
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (m + q >= g.M) continue;
                            g.out[(long long)(m + q) * g.ldo + n] = fmaf(fmaxf(tot[i][j][4 * q4 + q] + bias, 0.f), sc, sh);
                        }
                    }
                }
            }
    } else {
        // the K loop ended on a barrier: the operand stages are dead, the tile of logits takes their place
        float *tile = smem;
        constexpr int LDT = BN + 1;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int nl = (wn * TN + j) * 32 + lr;
                const float bias = g.bias[n0 + nl];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ml = (wm * TM + i) * 32 + 4 * lk + (r & 3) + 8 * (r >> 2);
                    tile[ml * LDT + nl] = tot[i][j][r] + bias;
                }
            }
        __syncthreads();
        if (EMODE == E_DET) {
            // softmax over the 65 logits of a cell, the dustbin dropped, channel c = 8 i + j to pixel (8 hc + i, 8 wc + j)
            // (superpoint.py:122-128)
            const int m = m0 + tid;
            if (tid < BM && m < g.M) {
                float *row = tile + tid * LDT;
                float mx = row[0];
                for (int c = 1; c < g.N; ++c) mx = fmaxf(mx, row[c]);
                float s = 0.f;
                for (int c = 0; c < g.N; ++c) { const float e = expf(row[c] - mx); row[c] = e; s += e; }
                const int hw = g.H * g.W, b = m / hw, p = m - b * hw, hc = p / g.W, wc = p - hc * g.W;
                const int Ws = g.W * kCell;
                float *o = g.out + ((long long)b * g.H * kCell + hc * kCell) * Ws + wc * kCell;
                for (int c = 0; c < kCell * kCell; ++c) o[(c >> 3) * Ws + (c & 7)] = row[c] / s;
            }
        } else {
            // F.normalize(p=2, dim=1) (superpoint.py:117): v / max(||v||, 1e-12); 8 threads per row
            static_assert(EMODE != E_DESC || BM == 32, "E_DESC: 32 rows x 8 threads");
            const int row = tid >> 3, part = tid & 7;
            float ss = 0.f;
            for (int c = part; c < g.N; c += 8) { const float v = tile[row * LDT + c]; ss = fmaf(v, v, ss); }
            ss += __shfl_xor(ss, 1, 64);
            ss += __shfl_xor(ss, 2, 64);
            ss += __shfl_xor(ss, 4, 64);
            if (part == 0) rown[row] = fmaxf(sqrtf(ss), 1e-12f);
            __syncthreads();
            for (int idx = tid; idx < BM * BN; idx += 256) {
                const int r = idx / BN, c = idx - r * BN;
                if (m0 + r < g.M && c < g.N) g.out[(long long)(m0 + r) * g.ldo + c] = tile[r * LDT + c] / rown[r];
            }
        }
    }
}

// The first VGG block's first conv, Cin = 1 (superpoint.py:93), direct: 16 threads per pixel, 4 output channels each.  A 3-channel
// input is reduced to gray (0.299 / 0.587 / 0.114, :112-114) inside the gather; a 1-channel input is taken as it is.
__global__ __launch_bounds__(256) void sp_conv_first(const float *img, int C, long long npix, int H, int W, const float *w,
                                                      const float *bias, const float *scale, const float *shift, float *out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, pix = idx >> 4;
    if (pix >= npix) return;
    const int cg = ((int)idx & 15) * 4;
    const int hw = H * W, b = (int)(pix / hw), p = (int)(pix - (long long)b * hw), y = p / W, x = p - y * W;
    const float *im = img + (long long)b * C * hw;
    float gy[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int hh = y + t / 3 - 1, ww = x + t % 3 - 1;
        float v = 0.f;
        if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
            const float *q = im + hh * W + ww;
            v = C == 3 ? (q[0] * 0.299f + q[hw] * 0.587f) + q[2 * hw] * 0.114f : q[0];
        }
        gy[t] = v;
    }
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const f32x4 wt = *reinterpret_cast<const f32x4 *>(w + t * 64 + cg);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = fmaf(gy[t], wt[i], a[i]);
    }
    const f32x4 bs = *reinterpret_cast<const f32x4 *>(bias + cg), sc = *reinterpret_cast<const f32x4 *>(scale + cg),
                sh = *reinterpret_cast<const f32x4 *>(shift + cg);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = fmaf(fmaxf(a[i] + bs[i], 0.f), sc[i], sh[i]);
    *reinterpret_cast<f32x4 *>(out + pix * 64 + cg) = o;
}

// ---- keypoints (superpoint.py:30-45, :129-149) ------------------------------------------------------------------------------------

constexpr int kNmsW = 64, kNmsH = 16, kNmsR = 8;      // output tile of one workgroup; largest radius

// One (2r+1)^2 max-pool of batched_nms with the comparisons around it; cells outside the image are -inf, as in max_pool2d.
//   MODE 0: mask  = scores == pool(scores)                                   (:39)
//   MODE 1: supp  = pool(mask) > 0;  ss = supp ? 0 : scores                  (:41-42)
//   MODE 2: mask |= (ss == pool(ss)) & ~supp                                 (:43-44); the last round also writes
//           out = mask ? scores : 0 (:45) and the remove_borders band = -1 (:132-137)
template <int MODE>
__global__ __launch_bounds__(256) void sp_nms_step(const float *scores, float *ss, unsigned char *mask, unsigned char *supp,
                                                    float *out, int H, int W, int r, int borders) {
    __shared__ float t0[kNmsH + 2 * kNmsR][kNmsW + 2 * kNmsR + 1];
    __shared__ float t1[kNmsH + 2 * kNmsR][kNmsW + 1];
    const int tid = threadIdx.x, x0 = blockIdx.x * kNmsW, y0 = blockIdx.y * kNmsH, th = kNmsH + 2 * r, tw = kNmsW + 2 * r;
    const long long img = (long long)blockIdx.z * H * W;
    for (int idx = tid; idx < th * tw; idx += 256) {
        const int ty = idx / tw, tx = idx - ty * tw, y = y0 + ty - r, x = x0 + tx - r;
        float v = -INFINITY;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const long long gi = img + (long long)y * W + x;
            v = MODE == 0 ? scores[gi] : MODE == 1 ? (float)mask[gi] : ss[gi];
        }
        t0[ty][tx] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < th * kNmsW; idx += 256) {
        const int ty = idx / kNmsW, x = idx - ty * kNmsW;
        float m = t0[ty][x];
        for (int d = 1; d <= 2 * r; ++d) m = fmaxf(m, t0[ty][x + d]);
        t1[ty][x] = m;
    }
    __syncthreads();
    for (int idx = tid; idx < kNmsH * kNmsW; idx += 256) {
        const int y = idx / kNmsW, x = idx - y * kNmsW, gy = y0 + y, gx = x0 + x;
        if (gy >= H || gx >= W) continue;
        float m = t1[y][x];
        for (int d = 1; d <= 2 * r; ++d) m = fmaxf(m, t1[y + d][x]);
        const float c = t0[y + r][x + r];
        const long long gi = img + (long long)gy * W + gx;
        if (MODE == 0) {
            mask[gi] = c == m;
        } else if (MODE == 1) {
            const bool sp = m > 0.f;
            supp[gi] = sp;
            ss[gi] = sp ? 0.f : scores[gi];
        } else {
            const bool nm = mask[gi] || (c == m && !supp[gi]);
            mask[gi] = nm;
            if (out) {
                float v = nm ? scores[gi] : 0.f;
                if (borders > 0 && (gy < borders || gx < borders || gy >= H - borders || gx >= W - borders)) v = -1.f;
                out[gi] = v;
            }
        }
    }
}

// nms_radius == 0 (every pixel is its own maximum): only the border band
__global__ void sp_border_only(const float *scores, float *out, int H, int W, int borders, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = (int)(i % ((long long)H * W)), gy = p / W, gx = p - gy * W;
    out[i] = (borders > 0 && (gy < borders || gx < borders || gy >= H - borders || gx >= W - borders)) ? -1.f : scores[i];
}

// rows of one image are compacted in order: count per row, exclusive scan over the rows, then one wave per row writes its
// keypoints behind the rows above it: the row-major order of torch.where (:141-149)
__global__ __launch_bounds__(64) void sp_row_count(const float *nms, int W, float thr, int *rowcnt) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float *p = nms + (long long)row * W;
    int n = 0;
    for (int x = lane; x < W; x += 64) n += p[x] > thr;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) rowcnt[row] = n;
}

__global__ __launch_bounds__(256) void sp_row_scan(const int *rowcnt, int H, int *rowoff, int *counts) {
    __shared__ int buf[256];
    __shared__ int carry;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int y0 = 0; y0 < H; y0 += 256) {
        const int y = y0 + tid, v = y < H ? rowcnt[b * H + y] : 0;
        buf[tid] = v;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const int add = tid >= s ? buf[tid - s] : 0;
            __syncthreads();
            buf[tid] += add;
            __syncthreads();
        }
        const int base = carry;
        if (y < H) rowoff[b * H + y] = base + buf[tid] - v;
        __syncthreads();
        if (tid == 255) carry = base + buf[255];
        __syncthreads();
    }
    if (tid == 0) counts[b] = carry;
}

__global__ __launch_bounds__(64) void sp_compact(const float *nms, int H, int W, float thr, const int *rowoff, long long cap,
                                                 float *kp, float *kps) {
    const int row = blockIdx.x, b = row / H, y = row - b * H, lane = threadIdx.x;
    const float *p = nms + (long long)row * W;
    int base = rowoff[row];
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const float v = x < W ? p[x] : -INFINITY;
        const bool on = v > thr;
        const unsigned long long bal = __ballot(on);
        if (on) {
            const long long o = b * cap + base + __popcll(bal & ((1ull << lane) - 1ull));
            kp[2 * o] = (float)x;
            kp[2 * o + 1] = (float)y;
            kps[o] = v;
        }
        base += __popcll(bal);
    }
}

// sample_descriptors (superpoint.py:16-27): bilinear grid_sample (align_corners=False, zeros padding) of the channels-last dense
// map at (kp + 0.5) / (s * [w, h]), then the L2 norm over channels; one wave per keypoint, 16-byte accesses along the channels
__global__ __launch_bounds__(256) void sp_sample(const float *kp, int n, const float *dense, int h, int w, int C, int s,
                                                 float *out) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    float gx = (kp[2 * k] + 0.5f) / ((float)w * (float)s), gy = (kp[2 * k + 1] + 0.5f) / ((float)h * (float)s);
    gx = gx * 2.f - 1.f;
    gy = gy * 2.f - 1.f;
    const float ix = ((gx + 1.f) * (float)w - 1.f) / 2.f, iy = ((gy + 1.f) * (float)h - 1.f) / 2.f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
    const float wt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
    f32x4 v[4];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane * 4 + i * 256;
        v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < C) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
                if (xx >= 0 && xx < w && yy >= 0 && yy < h) {
                    const f32x4 d = *reinterpret_cast<const f32x4 *>(dense + ((long long)yy * w + xx) * C + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[i][e] = fmaf(d[e], wt[t], v[i][e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) ss = fmaf(v[i][e], v[i][e], ss);
        }
    }
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < C) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = v[i][e] / nrm;
            *reinterpret_cast<f32x4 *>(out + (long long)k * C + c) = o;
        }
    }
}

// ---- matching (find_match_index, superpoint.py:206-223) ---------------------------------------------------------------------------

constexpr int kMT = 64, kMK = 32;     // tile of the similarity matrix per step; k per LDS stage and per accumulation chain

// best[i] = max over j of (order_key(<d1[i], d2[j]>) << 32 | ~j): the larger similarity wins, on equal similarities the lower j,
// as torch.argmax.  A workgroup owns 64 rows of d1 and walks every gridDim.y-th 64-column tile of d2; the N1 x N2 matrix exists
// only as 4 x 4 register tiles.
__global__ __launch_bounds__(256) void sp_match(const float *d1, int n1, const float *d2, int n2, int D,
                                                unsigned long long *best) {
    __shared__ __attribute__((aligned(16))) float As[kMK][kMT + 4];
    __shared__ __attribute__((aligned(16))) float Bs[kMK][kMT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, r0 = blockIdx.x * kMT;
    float bv[4];
    int bi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { bv[i] = -INFINITY; bi[i] = 0x7fffffff; }
    for (int ct = blockIdx.y; ct * kMT < n2; ct += gridDim.y) {
        const int c0 = ct * kMT;
        float tot[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[i][j] = 0.f;
        for (int k0 = 0; k0 < D; k0 += kMK) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int idx = tid + p * 256, row = idx >> 3, kq = (idx & 7) * 4;
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
                if (k0 + kq < D) {
                    if (r0 + row < n1) a = *reinterpret_cast<const f32x4 *>(d1 + (long long)(r0 + row) * D + k0 + kq);
                    if (c0 + row < n2) b = *reinterpret_cast<const f32x4 *>(d2 + (long long)(c0 + row) * D + k0 + kq);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) { As[kq + i][row] = a[i]; Bs[kq + i][row] = b[i]; }
            }
            __syncthreads();
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
#pragma unroll 8
            for (int k = 0; k < kMK; ++k) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(&As[k][ty * 4]), b = *reinterpret_cast<const f32x4 *>(&Bs[k][tx * 4]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) tot[i][j] += acc[i][j];
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = c0 + tx * 4 + j;
                if (col < n2 && tot[i][j] > bv[i]) { bv[i] = tot[i][j]; bi[i] = col; }      // columns ascend: strict >
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v = bv[i];
        int c = bi[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oc = __shfl_xor(c, o, 64);
            if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
        }
        const int row = r0 + ty * 4 + i;
        if (tx == 0 && row < n1 && c != 0x7fffffff) {
            const unsigned long long key = ((unsigned long long)order_key(v + 0.f) << 32) | (unsigned)(0xffffffffu - (unsigned)c);
            atomicMax(best + row, key);
        }
    }
}

__global__ void sp_match_decode(const unsigned long long *best, int n1, long long *index, float *sim) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n1) return;
    const unsigned long long k = best[i];
    // k == 0: no similarity of this row compared greater than -inf (a NaN descriptor); index 0 keeps later gathers in bounds
    index[i] = k ? (long long)(0xffffffffu - (unsigned)(k & 0xffffffffu)) : 0;
    sim[i] = k ? key_value((unsigned)(k >> 32)) : NAN;
}

// ---- the stabilising warp (apply_transform, superpoint.py:330-378) ---------------------------------------------------------------

// params per image: shift x, shift y, scale, angle (degrees), center x, center y.  The inverse rotation / scale / shift about the
// center and the normalisation to [-1, 1] are the reference's fp32 operations in its order (:350-371), followed by grid_sample's
// own un-normalisation (align_corners=False), the border clip, and four taps that are always multiplied and added when they lie
// inside the image, so that a NaN texel with weight 0 still gives NaN, as in torch.
template <bool VEC>
__global__ __launch_bounds__(256) void sp_affine_warp(const float *x, const float *params, float *out, int C, int H, int W,
                                                      int border) {
#pragma clang fp contract(off)
    const int xg = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (xg >= W || y >= H) return;
    const float *p = params + b * 6;
    const float cx = p[4], cy = p[5], sx = -p[0], sy = -p[1], inv = 1.0f / p[2];
    const float ang = -(p[3] * (float)(3.14159265358979323846 / 180.0));
    const float sn = sinf(ang), cs = cosf(ang);
    const float tx = sx + cx, ty = sy + cy, ax = (float)(W - 1) * 0.5f, ay = (float)(H - 1) * 0.5f;
    const long long hw = (long long)H * W;
    const float *xb = x + (long long)b * C * hw;
    float *ob = out + (long long)b * C * hw + (long long)y * W + xg;
    int i00[4];
    float w4[4][4];
    unsigned ok = 0;
    const float py = (float)y - cy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float px = (float)(xg + i) - cx;
        float gx = px * cs - py * sn, gy = px * sn + py * cs;
        gx = gx * inv; gy = gy * inv;
        gx = gx + tx; gy = gy + ty;
        gx = gx / ax - 1.0f; gy = gy / ay - 1.0f;
        float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f, iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
        if (border) {
            ix = fminf((float)(W - 1), fmaxf(ix, 0.f));
            iy = fminf((float)(H - 1), fmaxf(iy, 0.f));
        }
        const float fx = floorf(ix), fy = floorf(iy);
        // a coordinate far outside (or NaN) has no tap inside: keep the int conversion defined
        const bool far = !(fx >= -2.f && fx <= (float)W && fy >= -2.f && fy <= (float)H);
        const int x0 = far ? -2 : (int)fx, y0 = far ? -2 : (int)fy;
        const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
        w4[i][0] = wx0 * wy0; w4[i][1] = wx1 * wy0; w4[i][2] = wx0 * wy1; w4[i][3] = wx1 * wy1;
        i00[i] = y0 * W + x0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
            if (xx >= 0 && xx < W && yy >= 0 && yy < H) ok |= 1u << (i * 4 + t);
        }
    }
    for (int c = 0; c < C; ++c) {
        const float *xc = xb + c * hw;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float a = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (ok & (1u << (i * 4 + t))) a = a + xc[i00[i] + (t >> 1) * W + (t & 1)] * w4[i][t];
            o[i] = a;
        }
        if (VEC) {
            *reinterpret_cast<f32x4 *>(ob + c * hw) = (f32x4){o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (xg + i < W) ob[c * hw + i] = o[i];
        }
    }
}

struct Conv { float *w = nullptr, *bias = nullptr, *scale = nullptr, *shift = nullptr; int cin = 0, cout = 0, npad = 0; };

template <int AMODE, int EMODE, int WM, int WN, int TM, int TN>
void launch(const GemmArgs &g, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    dim3 grid(cdiv(g.M, BM), cdiv(g.N, BN));
    hipLaunchKernelGGL((sp_gemm<AMODE, EMODE, WM, WN, TM, TN>), grid, dim3(256), 0, s, g);
}

struct Tap { const char *name; float *p; long long shape[4]; };

long long keypoints_work_floats(long long B, long long H, long long W) {
    const long long n = B * H * W;
    return n + (2 * n + 3) / 4 + 2 * B * H + 8;
}

// NMS + border + threshold + ordered compaction of [B][H][W] score maps; the keypoint outputs are optional
int run_keypoints(const float *scores, int B, int H, int W, int radius, int borders, float thr, float *work, float *nms_out,
                  float *kp, float *kps, int *counts, hipStream_t s) {
    const long long n = (long long)B * H * W;
    float *ss = work;
    unsigned char *mask = reinterpret_cast<unsigned char *>(work + n), *supp = mask + n;
    int *rowcnt = reinterpret_cast<int *>(work + n + (2 * n + 3) / 4), *rowoff = rowcnt + B * H;
    float *nms = nms_out;
    if (radius == 0) {
        hipLaunchKernelGGL(sp_border_only, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scores, nms, H, W, borders, n);
        NUNIF_LAUNCH_CHECK();
    } else {
        dim3 grid(cdiv(W, kNmsW), cdiv(H, kNmsH), B);
        hipLaunchKernelGGL(sp_nms_step<0>, grid, dim3(256), 0, s, scores, ss, mask, supp, (float *)nullptr, H, W, radius, 0);
        NUNIF_LAUNCH_CHECK();
        for (int round = 0; round < 2; ++round) {
            hipLaunchKernelGGL(sp_nms_step<1>, grid, dim3(256), 0, s, scores, ss, mask, supp, (float *)nullptr, H, W, radius, 0);
            NUNIF_LAUNCH_CHECK();
            hipLaunchKernelGGL(sp_nms_step<2>, grid, dim3(256), 0, s, scores, ss, mask, supp, round == 1 ? nms : (float *)nullptr,
                               H, W, radius, borders);
            NUNIF_LAUNCH_CHECK();
        }
    }
    if (!kp) return NUNIF_HIP_OK;
    hipLaunchKernelGGL(sp_row_count, dim3(B * H), dim3(64), 0, s, nms, W, thr, rowcnt);
    NUNIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_row_scan, dim3(B), dim3(256), 0, s, rowcnt, H, rowoff, counts);
    NUNIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_compact, dim3(B * H), dim3(64), 0, s, nms, H, W, thr, rowoff, (long long)H * W, kp, kps);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

}  // namespace
}  // namespace nunif

using namespace nunif;

struct nunif_superpoint : DeviceOwner {
    Conv conv[8], heads, det, desc;
    // the launch plan of one input shape: buffer sizes and offsets into `work`; rebuilt when (B, H, W) changes
    int B = 0, H = 0, W = 0;
    int h = 0, w = 0;
    DeviceBuf work;
    float *scratch = nullptr, *blk[4] = {}, *hidden = nullptr, *dense = nullptr, *scores = nullptr, *nms = nullptr, *kwork = nullptr;
    std::vector<Tap> taps;                     // what debug_taps may read: names and shapes of the buffers above
};

namespace {

int fetch_conv(nunif_superpoint *h, const TensorMap &m, const std::string &p, int cin, int cout, int npad, int k, bool affine,
               Conv *c) {
    const HostTensor *t = nullptr;
    int rc;
    c->cin = cin; c->cout = cout; c->npad = npad;
    struct { const char *suffix; size_t n; float **dst; bool need; } parts[] = {
        {".w", (size_t)k * npad, &c->w, true}, {".bias", (size_t)npad, &c->bias, true},
        {".scale", (size_t)npad, &c->scale, affine}, {".shift", (size_t)npad, &c->shift, affine}};
    for (auto &q : parts) {
        if (!q.need) continue;
        if ((rc = find(m, p + q.suffix, &t))) return rc;
        NUNIF_REQUIRE((size_t)t->numel == q.n, "superpoint_create: '%s%s' has %lld elements, expected %zu", p.c_str(), q.suffix,
                      (long long)t->numel, q.n);
        if ((rc = h->upload_f32(t, q.dst))) return rc;
    }
    return NUNIF_HIP_OK;
}

const int kChan[5] = {1, 64, 64, 128, 128};

}  // namespace

extern "C" void nunif_hip_superpoint_destroy(nunif_superpoint *h) {
    if (!h) return;
    h->free_all();
    h->work.release();
    delete h;
}

extern "C" int nunif_hip_superpoint_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_superpoint **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "superpoint_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    nunif_superpoint *h = new nunif_superpoint();
    int rc = NUNIF_HIP_OK;
    for (int i = 0; i < 8 && rc == NUNIF_HIP_OK; ++i) {
        const int blk = i / 2, cout = kChan[blk + 1], cin = (i & 1) ? cout : kChan[blk];
        rc = fetch_conv(h, m, "backbone." + std::to_string(blk) + "." + std::to_string(i & 1), cin, cout, cout, 9 * cin, true,
                        &h->conv[i]);
    }
    if (rc == NUNIF_HIP_OK) rc = fetch_conv(h, m, "heads", 128, 512, 512, 9 * 128, true, &h->heads);
    if (rc == NUNIF_HIP_OK) rc = fetch_conv(h, m, "detector", 256, 65, 96, 256, false, &h->det);
    if (rc == NUNIF_HIP_OK) rc = fetch_conv(h, m, "descriptor", 256, 256, 256, 256, false, &h->desc);
    if (rc != NUNIF_HIP_OK) { nunif_hip_superpoint_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" int64_t nunif_hip_superpoint_keypoints_work_floats(int32_t B, int32_t H, int32_t W) {
    return keypoints_work_floats(B, H, W);
}

extern "C" int nunif_hip_superpoint_keypoints(const float *scores, int32_t B, int32_t H, int32_t W, int32_t nms_radius,
                                              int32_t remove_borders, float threshold, float *work, float *nms_out,
                                              float *keypoints, float *kp_scores, int32_t *counts, void *stream) {
    NUNIF_REQUIRE(scores && work && nms_out && B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1LL << 30),
                  "superpoint_keypoints: bad argument (B = %d, H = %d, W = %d)", B, H, W);
    NUNIF_REQUIRE(nms_radius >= 0 && nms_radius <= kNmsR, "superpoint_keypoints: nms_radius %d (0 .. %d are built)", nms_radius, kNmsR);
    NUNIF_REQUIRE(remove_borders >= 0, "superpoint_keypoints: remove_borders %d", remove_borders);
    NUNIF_REQUIRE(!keypoints || (kp_scores && counts), "superpoint_keypoints: keypoints without kp_scores / counts");
    return run_keypoints(scores, B, H, W, nms_radius, remove_borders, threshold, work, nms_out, keypoints, kp_scores, counts,
                         (hipStream_t)stream);
}

extern "C" int nunif_hip_superpoint_forward(nunif_superpoint *h, const float *image, int32_t B, int32_t C, int32_t H, int32_t W,
                                            int32_t nms_radius, int32_t remove_borders, float threshold, float *keypoints,
                                            float *kp_scores, int32_t *counts, void *stream) {
    NUNIF_REQUIRE(h && image, "superpoint_forward: NULL argument");
    NUNIF_REQUIRE((C == 1 || C == 3) && B >= 1 && H >= 8 && W >= 8 && (long long)B * H * W < (1LL << 24),
                  "superpoint_forward: B = %d, C = %d, H = %d, W = %d (need C in {1, 3}, H, W >= 8, B * H * W < 2^24)", B, C, H, W);
    NUNIF_REQUIRE(nms_radius >= 0 && nms_radius <= kNmsR, "superpoint_forward: nms_radius %d (0 .. %d are built)", nms_radius, kNmsR);
    NUNIF_REQUIRE(remove_borders >= 0, "superpoint_forward: remove_borders %d", remove_borders);
    NUNIF_REQUIRE(!keypoints || (kp_scores && counts), "superpoint_forward: keypoints without kp_scores / counts");
    hipStream_t s = (hipStream_t)stream;
    const int H2 = H / 2, W2 = W / 2, H4 = H2 / 2, W4 = W2 / 2, hc = H4 / 2, wc = W4 / 2, Hs = hc * kCell, Ws = wc * kCell;
    if (B != h->B || H != h->H || W != h->W) {
        // the plan: [conv scratch][block 0][block 1][block 2][block 3][heads][dense descriptors][scores][nms][keypoint work]
        const long long n[] = {(long long)B * H * W * 64, (long long)B * H2 * W2 * 64, (long long)B * H4 * W4 * 64,
                               (long long)B * hc * wc * 128, (long long)B * hc * wc * 128, (long long)B * hc * wc * 512,
                               (long long)B * hc * wc * 256, (long long)B * Hs * Ws, (long long)B * Hs * Ws,
                               keypoints_work_floats(B, Hs, Ws)};
        long long off[11] = {0};
        for (int i = 0; i < 10; ++i) off[i + 1] = off[i] + ((n[i] + 3) & ~3LL);
        if ((size_t)off[10] * sizeof(float) > h->work.cap) NUNIF_HIP_CHECK(hipDeviceSynchronize());
        int rc = h->work.ensure((size_t)off[10] * sizeof(float));
        if (rc) { h->B = 0; return rc; }
        float *base = (float *)h->work.p;
        h->scratch = base + off[0];
        for (int i = 0; i < 4; ++i) h->blk[i] = base + off[1 + i];
        h->hidden = base + off[5]; h->dense = base + off[6]; h->scores = base + off[7]; h->nms = base + off[8];
        h->kwork = base + off[9];
        h->taps = {{"backbone.0", h->blk[0], {B, H2, W2, 64}}, {"backbone.1", h->blk[1], {B, H4, W4, 64}},
                   {"backbone.2", h->blk[2], {B, hc, wc, 128}}, {"backbone.3", h->blk[3], {B, hc, wc, 128}},
                   {"heads", h->hidden, {B, hc, wc, 512}}, {"descriptors", h->dense, {B, hc, wc, 256}},
                   {"scores", h->scores, {B, 1, Hs, Ws}}, {"nms", h->nms, {B, 1, Hs, Ws}}};
        h->B = B; h->H = H; h->W = W; h->h = hc; h->w = wc;
    }
    float *scratch = h->scratch, *const *blk = h->blk, *heads = h->hidden, *dense = h->dense, *scores = h->scores, *nms = h->nms;

    {
        const Conv &c = h->conv[0];
        const long long npix = (long long)B * H * W;
        ProfScope prof("superpoint_conv_first", s, 2.0 * npix * 9 * 64, 0.0);
        hipLaunchKernelGGL(sp_conv_first, dim3((unsigned)((npix * 16 + 255) / 256)), dim3(256), 0, s, image, C, npix, H, W, c.w, c.bias,
                           c.scale, c.shift, scratch);
        NUNIF_LAUNCH_CHECK();
    }
    const float *in = scratch;
    int ih = H, iw = W;
    for (int i = 1; i < 8; ++i) {
        const Conv &c = h->conv[i];
        const bool second = i & 1, pool = second && i < 7;
        GemmArgs g = {};
        g.A = in; g.Bm = c.w; g.bias = c.bias; g.scale = c.scale; g.shift = c.shift;
        g.out = second ? blk[i / 2] : scratch;
        g.N = c.cout; g.K = 9 * c.cin; g.ldb = c.npad; g.ldo = c.cout; g.H = ih; g.W = iw; g.C = c.cin;
        g.Hp = ih / 2; g.Wp = iw / 2;
        g.M = pool ? B * g.Hp * g.Wp * 4 : B * ih * iw;
        ProfScope prof("superpoint_conv3", s, 2.0 * g.M * g.K * g.N, 0.0);
        if (c.cout == 64) {
            if (pool) launch<A_CONV_POOL, E_BN_POOL, 4, 1, 1, 2>(g, s);
            else launch<A_CONV, E_BN, 4, 1, 1, 2>(g, s);
        } else {
            if (pool) launch<A_CONV_POOL, E_BN_POOL, 2, 2, 2, 2>(g, s);
            else launch<A_CONV, E_BN, 2, 2, 2, 2>(g, s);
        }
        NUNIF_LAUNCH_CHECK();
        in = g.out;
        if (pool) { ih = g.Hp; iw = g.Wp; }
    }
    {
        const Conv &c = h->heads;
        GemmArgs g = {};
        g.A = blk[3]; g.Bm = c.w; g.bias = c.bias; g.scale = c.scale; g.shift = c.shift; g.out = heads;
        g.M = B * hc * wc; g.N = 512; g.K = 9 * 128; g.ldb = 512; g.ldo = 512; g.H = hc; g.W = wc; g.C = 128;
        ProfScope prof("superpoint_heads", s, 2.0 * g.M * g.K * g.N, 0.0);
        launch<A_CONV, E_BN, 2, 2, 2, 2>(g, s);
        NUNIF_LAUNCH_CHECK();
        GemmArgs d = {};
        d.A = heads; d.Bm = h->det.w; d.bias = h->det.bias; d.out = scores;
        d.M = B * hc * wc; d.N = 65; d.K = 256; d.lda = 512; d.ldb = 96; d.H = hc; d.W = wc;
        launch<A_PLAIN, E_DET, 4, 1, 1, 3>(d, s);
        NUNIF_LAUNCH_CHECK();
        GemmArgs e = {};
        e.A = heads + 256; e.Bm = h->desc.w; e.bias = h->desc.bias; e.out = dense;
        e.M = B * hc * wc; e.N = 256; e.K = 256; e.lda = 512; e.ldb = 256; e.ldo = 256;
        launch<A_PLAIN, E_DESC, 1, 4, 1, 2>(e, s);
        NUNIF_LAUNCH_CHECK();
    }
    ProfScope prof("superpoint_keypoints", s, 0.0, 0.0);
    return run_keypoints(scores, B, Hs, Ws, nms_radius, remove_borders, threshold, h->kwork, nms, keypoints, kp_scores,
                         counts, s);
}

extern "C" int nunif_hip_superpoint_debug_taps(nunif_superpoint *h, const char *name, float *out, int64_t capacity,
                                               int64_t *shape4, void *stream) {
    NUNIF_REQUIRE(h && name && out && shape4, "superpoint_debug_taps: NULL argument");
    NUNIF_REQUIRE(h->B > 0, "superpoint_debug_taps: no forward has run on this handle");
    const Tap *found = nullptr;
    for (const Tap &c : h->taps)
        if (std::string(name) == c.name) found = &c;
    NUNIF_REQUIRE(found, "superpoint_debug_taps: no tap named %s", name);
    const Tap &t = *found;
    const int64_t n = t.shape[0] * t.shape[1] * t.shape[2] * t.shape[3];
    NUNIF_REQUIRE(capacity >= n, "superpoint_debug_taps: %s needs %lld floats", name, (long long)n);
    for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
    NUNIF_HIP_CHECK(hipMemcpyAsync(out, t.p, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_sample_descriptors(const float *keypoints, int32_t n, const float *dense, int32_t h, int32_t w,
                                            int32_t C, int32_t stride, float *out, void *stream) {
    NUNIF_REQUIRE(n >= 0 && h >= 1 && w >= 1 && stride >= 1 && C >= 4 && C % 4 == 0 && C <= 1024,
                  "sample_descriptors: n = %d, h = %d, w = %d, C = %d, stride = %d (need C %% 4 == 0, C <= 1024)", n, h, w, C, stride);
    if (n == 0) return NUNIF_HIP_OK;
    NUNIF_REQUIRE(keypoints && dense && out, "sample_descriptors: NULL argument");
    hipLaunchKernelGGL(sp_sample, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, keypoints, n, dense, h, w, C, stride, out);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_superpoint_sample(nunif_superpoint *h, int32_t b, const float *keypoints, int32_t n, float *out,
                                           void *stream) {
    NUNIF_REQUIRE(h && h->B > 0 && b >= 0 && b < h->B, "superpoint_sample: image %d of a batch of %d", b, h ? h->B : 0);
    return nunif_hip_sample_descriptors(keypoints, n, h->dense + (long long)b * h->h * h->w * 256, h->h, h->w, 256, kCell, out, stream);
}

extern "C" int nunif_hip_superpoint_match(const float *d1, int32_t n1, const float *d2, int32_t n2, int32_t D, void *work,
                                          int64_t *index, float *max_similarity, void *stream) {
    NUNIF_REQUIRE(d1 && d2 && work && index && max_similarity && n1 >= 1 && n2 >= 1 && D >= 4 && D % 4 == 0,
                  "superpoint_match: n1 = %d, n2 = %d, D = %d (need n1, n2 >= 1, D %% 4 == 0)", n1, n2, D);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *best = (unsigned long long *)work;
    NUNIF_HIP_CHECK(hipMemsetAsync(best, 0, (size_t)n1 * sizeof(unsigned long long), s));
    const int rows = cdiv(n1, kMT), cols = cdiv(n2, kMT);
    int split = cdiv(512, rows);                    // about two workgroups per CU when d1 alone does not fill the device
    if (split > cols) split = cols;
    ProfScope prof("superpoint_match", s, 2.0 * n1 * n2 * D, 0.0);
    hipLaunchKernelGGL(sp_match, dim3(rows, split), dim3(256), 0, s, d1, n1, d2, n2, D, best);
    NUNIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_match_decode, dim3(cdiv(n1, 256)), dim3(256), 0, s, best, n1, (long long *)index, max_similarity);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_affine_warp(const float *x, const float *params, float *out, int32_t B, int32_t C, int32_t H, int32_t W,
                                     int32_t padding_mode, void *stream) {
    NUNIF_REQUIRE(x && params && out && x != out && B >= 1 && C >= 1 && H >= 1 && W >= 1 && B <= 65535 &&
                  (long long)B * C * H * W < (1LL << 40) && (long long)C * H * W < (1LL << 31),
                  "affine_warp: bad argument (B = %d, C = %d, H = %d, W = %d)", B, C, H, W);
    if (padding_mode != 0 && padding_mode != 1) {
        set_error("affine_warp: padding_mode %d (0 zeros and 1 border are built; reflection is not)", padding_mode);
        return NUNIF_HIP_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(cdiv(W, 256), cdiv(H, 4), B);
    ProfScope prof("affine_warp", s, 0.0, 8.0 * B * C * H * W);
    if (W % 4 == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(sp_affine_warp<true>, grid, dim3(256), 0, s, x, params, out, C, H, W, padding_mode);
    else
        hipLaunchKernelGGL(sp_affine_warp<false>, grid, dim3(256), 0, s, x, params, out, C, H, W, padding_mode);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
