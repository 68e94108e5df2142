// LightOutpaintV1 (stlizer/models/light_outpaint_v1.py, reference) for gfx950: the coarse outpaint network of stlizer's
// --border outpaint / expand_outpaint, its infer() wrapper and the EMA frame buffer of pass 4, fp32 throughout.
//
// The net is tiny (a 640 x 640 frame is an 80 x 80 x 64 map = 100 windows) and bound by launches and occupancy, not by FLOPs, so
// every GEMM runs on v_mfma_f32_32x32x2_f32 with exact fp32 operands (K <= 64: one k-ordered fmaf chain per output element) and a
// window / tile is ONE workgroup whose four waves split its 32 x 32 output tiles.  Activations are channels-last [image][y][x][c].
//
//   op_entry    both resizes of infer (:180-193), the 3x3 mask dilation and threshold, the zeroing, OutpaintBase's pad to a
//               multiple of 64 (:142-148) and the 4-channel cat (:116)
//   op_down     a 3x3 stride-2 conv over a replicate pad of 1 + LeakyReLU 0.2 (Downsampling :54-71), direct
//   op_mha      one MHABlock (:35-51) per 8 x 8 window: qkv -> scores + bias table -> softmax -> PV -> head_proj -> residual ->
//               GLU MLP -> residual, the window's 64 tokens in LDS
//   op_pool     one PoolBlock (:12-32) per 8 x 8 tile: 5x5 average of the in-image taps minus x on the tile + 1, 1x1 conv, LeakyReLU,
//               replicate pad, depthwise 3x3, GLU, 1x1 conv, residual
//   op_pw       proj_mid / proj_out (+ the skip add, :119)
//   op_proj3    the 64 -> 3 projection of ToImageBilinaer (:81-84) on the map
//   op_exit     the x8 bilinear upsample, the crop of the pad, infer's resize back (:198-199: a second gather over the first, not
//               merged with it) and the composite / raw / forward (:164-173, :201-206) output
//   op_buffer   lines 452-453 and 460-471 of stlizer/multipass_pipeline.py for a batch
#include <cmath>
#include <string>
#include <vector>

#include "gemm_f32.h"
#include "host_weights.h"

namespace nunif {
namespace {

constexpr int kWin = 8;                  // window side = stride of the net
constexpr int kTok = kWin * kWin;        // tokens per window / pixels per pool tile
constexpr int kHead = 32;                // channels per attention head
constexpr int kUnit = 64;                // OutpaintBase pads to a multiple of mod * downscaling_factor

enum { MODE_COMPOSITE = 0, MODE_RAW = 1, MODE_FORWARD = 2 };

// acc += A[32 rows][K] * B[K][32 columns]; A in LDS with element (i, k) at A[i * sa + k], B in global memory row-major with
// element (k, j) at B[k * ldb + j].  Lane l feeds A[l & 31][k + (l >> 5)] and B[k + (l >> 5)][l & 31].
template <int K>
__device__ __forceinline__ f32x16 mm_lg(const float *A, int sa, const float *B, int ldb, f32x16 acc, int lane) {
    const int lr = lane & 31, lk = lane >> 5;
    float b[K / 2];
#pragma unroll
    for (int k = 0; k < K; k += 2) b[k / 2] = B[(k + lk) * ldb + lr];
#pragma unroll
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[lr * sa + k + lk], b[k / 2], acc, 0, 0, 0);
    return acc;
}

// both operands in LDS: A element (i, k) at A[i * sa + k], B element (k, j) at B[k * sbk + j * sbj]
template <int K>
__device__ __forceinline__ f32x16 mm_ll(const float *A, int sa, const float *B, int sbk, int sbj, f32x16 acc, int lane) {
    const int lr = lane & 31, lk = lane >> 5;
#pragma unroll
    for (int k = 0; k < K; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[lr * sa + k + lk], B[(k + lk) * sbk + lr * sbj], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.2f * v; }
__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// ---- bilinear, align_corners=False, as torch's upsample_bilinear2d -------------------------------------------------------------

struct Lerp { int i0, i1; float l0, l1; };

__device__ __forceinline__ Lerp lerp_index(int dst, float scale, int in_size) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    int i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    Lerp r;
    r.i0 = i0;
    r.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    r.l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
    r.l0 = 1.f - r.l1;
    return r;
}

__device__ __forceinline__ float lerp2(const Lerp &ly, const Lerp &lx, float v00, float v01, float v10, float v11) {
    return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}

struct Geo {
    int B, H, W;           // the frames
    int nh, nw;            // the size the net sees before its pad (H, W unless max(H, W) > max_size)
    int Hp, Wp;            // padded to a multiple of 64
    int resized, padded;
    float sy, sx;          // source-index scales of the resize in (H / nh, W / nw)
    float ry, rx;          // and of the resize back (nh / H, nw / W)
};

// the float mask resized to (nh, nw) at (y, x) (:188)
__device__ __forceinline__ float mask_resized(const unsigned char *m, const Geo &g, int y, int x) {
    const Lerp ly = lerp_index(y, g.sy, g.H), lx = lerp_index(x, g.sx, g.W);
    const unsigned char *r0 = m + (long long)ly.i0 * g.W, *r1 = m + (long long)ly.i1 * g.W;
    return lerp2(ly, lx, r0[lx.i0] ? 1.f : 0.f, r0[lx.i1] ? 1.f : 0.f, r1[lx.i0] ? 1.f : 0.f, r1[lx.i1] ? 1.f : 0.f);
}

// [B][Hp][Wp][4] = (x, mask) as _forward's cat sees them
__global__ __launch_bounds__(256) void op_entry(const float *x, const unsigned char *mask, float *out, const Geo g) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, npix = (long long)g.B * g.Hp * g.Wp;
    if (idx >= npix) return;
    const int hw = g.Hp * g.Wp, b = (int)(idx / hw), p = (int)(idx - (long long)b * hw), y = p / g.Wp, xx = p - y * g.Wp;
    const int ys = min(y, g.nh - 1), xs = min(xx, g.nw - 1);            // the replicate pad (right / bottom only)
    const long long plane = (long long)g.H * g.W;
    const unsigned char *mb = mask + b * plane;
    const float *xb = x + 3 * b * plane;
    bool m;
    float v[3];
    if (g.resized) {
        float pooled = -INFINITY;                                        // max_pool2d(3, 1, 1): cells outside do not count
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = ys + dy, xc = xs + dx;
                if (yy >= 0 && yy < g.nh && xc >= 0 && xc < g.nw) pooled = fmaxf(pooled, mask_resized(mb, g, yy, xc));
            }
        m = pooled > 0.5f;
        const Lerp ly = lerp_index(ys, g.sy, g.H), lx = lerp_index(xs, g.sx, g.W);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *r0 = xb + c * plane + (long long)ly.i0 * g.W, *r1 = xb + c * plane + (long long)ly.i1 * g.W;
            v[c] = m ? 0.f : lerp2(ly, lx, r0[lx.i0], r0[lx.i1], r1[lx.i0], r1[lx.i1]);
        }
    } else {
        const long long o = (long long)ys * g.W + xs;
        m = mb[o] != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = xb[c * plane + o];
    }
    const float mf = (y >= g.nh || xx >= g.nw || m) ? 1.f : 0.f;
    if (g.padded) {                                                      // only a padded input is masked (:145-148)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] * (1.f - mf);
    }
    *reinterpret_cast<f32x4 *>(out + idx * 4) = (f32x4){v[0], v[1], v[2], mf};
}

// 3x3 stride-2 conv over a replicate pad of 1, LeakyReLU 0.2; w [9 * CIN][COUT] (row = tap * CIN + c); 4 output channels a thread
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void op_down(const float *in, const float *w, const float *bias, float *out, long long nout,
                                               int Hi, int Wi) {
    constexpr int G = COUT / 4;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nout * G) return;
    const long long pix = idx / G;
    const int cg = (int)(idx - pix * G) * 4;
    const int Ho = Hi / 2, Wo = Wi / 2, hw = Ho * Wo, b = (int)(pix / hw), p = (int)(pix - (long long)b * hw), y = p / Wo, x = p - y * Wo;
    const float *ib = in + (long long)b * Hi * Wi * CIN;
    f32x4 acc = *reinterpret_cast<const f32x4 *>(bias + cg);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = min(max(2 * y - 1 + t / 3, 0), Hi - 1), xx = min(max(2 * x - 1 + t % 3, 0), Wi - 1);
        const float *ip = ib + ((long long)yy * Wi + xx) * CIN;
#pragma unroll
        for (int c4 = 0; c4 < CIN; c4 += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(ip + c4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 wt = *reinterpret_cast<const f32x4 *>(w + (t * CIN + c4 + i) * COUT + cg);
#pragma unroll
                for (int o = 0; o < 4; ++o) acc[o] = fmaf(v[i], wt[o], acc[o]);
            }
        }
    }
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = leaky(acc[i]);
    *reinterpret_cast<f32x4 *>(out + pix * COUT + cg) = o;
}

struct MhaW { const float *qkv, *qkv_b, *table, *proj, *proj_b, *mlp1, *mlp1_b, *mlp2, *mlp2_b; };

// One MHABlock on one window.  qkv [C][3C] with the columns of head h at h * 96 + (q | k | v) * 32; table [64][64]; proj / mlp2
// [C][C] and mlp1 [C][2C] are input-major.  LDS: the window X [64][C + 1], one head's q | k | v [64][97] (q's columns later hold
// that head's attention output, the whole region the block's first residual sum), the head's scores [64][65] (later the GLU
// output).  The head projection is accumulated over the heads in registers.
template <int C>
__global__ __launch_bounds__(256) void op_mha(const float *x, float *out, const MhaW w, int hm, int wm) {
    constexpr int NH = C / kHead, NCT = C / 32, NT = 2 * NCT, LX = C + 1, LQ = 3 * kHead + 1, LS = kTok + 1;
    __shared__ float sm[kTok * (LX + LQ + LS)];
    float *X = sm, *Q = sm + kTok * LX, *S = Q + kTok * LQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31;
    const int wpr = wm / kWin, wpi = (hm / kWin) * wpr, b = blockIdx.x / wpi, wi = blockIdx.x - b * wpi, wy = wi / wpr, wx = wi - wy * wpr;
    const long long base = (((long long)b * hm + wy * kWin) * wm + wx * kWin) * C;          // token t: + ((t >> 3) * wm + (t & 7)) * C
    for (int i = tid; i < kTok * C / 4; i += 256) {
        const int t = i / (C / 4), c = (i - t * (C / 4)) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(x + base + ((long long)(t >> 3) * wm + (t & 7)) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) X[t * LX + c + e] = v[e];
    }
    __syncthreads();
    const bool own = wave < NT;                    // the [64][C] outputs are NT tiles of 32 x 32: one a wave
    const int ort = wave / NCT, oct = wave % NCT;
    const float scale = 0.17677669529663687f;      // 1 / sqrt(32)
    f32x16 yacc = zero16();
    for (int hd = 0; hd < NH; ++hd) {
        for (int t = wave; t < 6; t += 4) {
            const int rt = t / 3, ct = t - rt * 3, col = hd * 3 * kHead + ct * 32;
            const f32x16 a = mm_lg<C>(X + rt * 32 * LX, LX, w.qkv + col, 3 * C, zero16(), lane);
            const float bs = w.qkv_b[col + lr];
#pragma unroll
            for (int r = 0; r < 16; ++r) Q[(rt * 32 + acc_row(r, lane)) * LQ + ct * 32 + lr] = a[r] + bs;
        }
        __syncthreads();
        {
            const int rt = wave >> 1, ct = wave & 1;
            const f32x16 a = mm_ll<kHead>(Q + rt * 32 * LQ, LQ, Q + ct * 32 * LQ + kHead, 1, LQ, zero16(), lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt * 32 + acc_row(r, lane), col = ct * 32 + lr;
                S[row * LS + col] = fmaf(a[r], scale, w.table[row * kTok + col]);
            }
        }
        __syncthreads();
        {
            float *row = S + (tid >> 2) * LS + (tid & 3) * 16;
            float mx = row[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, row[i]);
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            float e[16], s = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { e[i] = expf(row[i] - mx); s += e[i]; }
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
#pragma unroll
            for (int i = 0; i < 16; ++i) row[i] = e[i] / s;
        }
        __syncthreads();
        if (wave < 2) {                            // P [64][64] * V [64][32]: two tiles
            const f32x16 a = mm_ll<kTok>(S + wave * 32 * LS, LS, Q + 2 * kHead, LQ, 1, zero16(), lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) Q[(wave * 32 + acc_row(r, lane)) * LQ + lr] = a[r];
        }
        __syncthreads();
        if (own) yacc = mm_lg<kHead>(Q + ort * 32 * LQ, LQ, w.proj + hd * kHead * C + oct * 32, C, yacc, lane);
        __syncthreads();
    }
    float *Y = Q, *G = S;                          // [64][LX] each
    if (own) {
        const float bs = w.proj_b[oct * 32 + lr];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int at = (ort * 32 + acc_row(r, lane)) * LX + oct * 32 + lr;
            Y[at] = X[at] + (yacc[r] + bs);
        }
    }
    __syncthreads();
    if (own) {
        const f32x16 a = mm_lg<C>(Y + ort * 32 * LX, LX, w.mlp1 + oct * 32, 2 * C, zero16(), lane);
        const f32x16 g = mm_lg<C>(Y + ort * 32 * LX, LX, w.mlp1 + C + oct * 32, 2 * C, zero16(), lane);
        const float ba = w.mlp1_b[oct * 32 + lr], bg = w.mlp1_b[C + oct * 32 + lr];
#pragma unroll
        for (int r = 0; r < 16; ++r) G[(ort * 32 + acc_row(r, lane)) * LX + oct * 32 + lr] = (a[r] + ba) * sigmoidf(g[r] + bg);
    }
    __syncthreads();
    if (own) {
        const f32x16 a = mm_lg<C>(G + ort * 32 * LX, LX, w.mlp2 + oct * 32, C, zero16(), lane);
        const float bs = w.mlp2_b[oct * 32 + lr];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = ort * 32 + acc_row(r, lane), c = oct * 32 + lr;
            out[base + ((long long)(t >> 3) * wm + (t & 7)) * C + c] = Y[t * LX + c] + (a[r] + bs);
        }
    }
}

struct PoolW { const float *pw1, *pw1_b, *dw, *dw_b, *pw2, *pw2_b; };

// One PoolBlock on one 8 x 8 tile of the map.  The depthwise conv needs the 1x1 conv's output on the tile + 1 (a 10 x 10 region,
// 100 GEMM rows), that needs the pooled map there, and the pool reaches 2 further: a halo of 3, read from global memory (the map
// is L2 resident).  Border rules are the MAP's: the average divides by the number of in-image taps, and a region pixel outside
// the map is never computed, the depthwise conv reads the clamped pixel instead (the replicate pad).  pw1 [C][2C] with the columns
// of chunk j at 64 j: GLU values 32 j .. 32 j + 31, then their gates; dw [9][2C] and dw_b in the reference's channel order.
// LDS: x1 [100][C + 1] | (row sums [14][10][C], then per chunk hidden [100][65] and GLU output [64][33]).
template <int C>
__global__ __launch_bounds__(256) void op_pool(const float *x, float *out, const PoolW w, int hm, int wm) {
    constexpr int NCT = C / 32, NT = 2 * NCT, LX = C + 1, LH = 65, LG = 33, R = kWin + 2, NR = R * R;
    constexpr int NX1 = NR * LX, NHS = (kWin + 6) * R * C, NHG = NR * LH + kTok * LG, NREST = NHS > NHG ? NHS : NHG;
    static_assert(NX1 + NREST >= 128 * LX, "the A operand reads 128 rows");
    static_assert((NX1 + NREST) * 4 <= 65536, "LDS");
    __shared__ float sm[NX1 + NREST];
    float *X1 = sm, *HS = sm + NX1, *Hd = sm + NX1, *G = Hd + NR * LH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31;
    const int tpr = wm / kWin, tpi = (hm / kWin) * tpr, b = blockIdx.x / tpi, ti = blockIdx.x - b * tpi, y0 = (ti / tpr) * kWin,
              x0 = (ti % tpr) * kWin;
    const float *xb = x + (long long)b * hm * wm * C;
    for (int i = tid; i < (kWin + 6) * R * C; i += 256) {
        const int c = i % C, p = i / C, rx = p % R, ry = p / R, y = y0 - 3 + ry, xx = x0 - 1 + rx;
        float s = 0.f;
        if (y >= 0 && y < hm && xx >= 0 && xx < wm) {
            const float *row = xb + (long long)y * wm * C + c;
#pragma unroll
            for (int d = -2; d <= 2; ++d)
                if (xx + d >= 0 && xx + d < wm) s += row[(xx + d) * C];
        }
        HS[i] = s;
    }
    __syncthreads();
    for (int i = tid; i < NR * C; i += 256) {
        const int c = i % C, p = i / C, rx = p % R, ry = p / R, y = y0 - 1 + ry, xx = x0 - 1 + rx;
        float v = 0.f;
        if (y >= 0 && y < hm && xx >= 0 && xx < wm) {
            float s = 0.f;
#pragma unroll
            for (int d = -2; d <= 2; ++d)
                if (y + d >= 0 && y + d < hm) s += HS[((ry + 2 + d) * R + rx) * C + c];
            const int ny = min(y + 2, hm - 1) - max(y - 2, 0) + 1, nx = min(xx + 2, wm - 1) - max(xx - 2, 0) + 1;
            v = s / (float)(ny * nx) - xb[((long long)y * wm + xx) * C + c];
        }
        X1[p * LX + c] = v;
    }
    __syncthreads();
    const bool own = wave < NT;
    const int ort = wave / NCT, oct = wave % NCT;
    f32x16 oacc = zero16();
    for (int j = 0; j < NCT; ++j) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {           // rows 32 wave .. 32 wave + 31 of the region, GLU values then gates
            const int col = j * 64 + ct * 32;
            const f32x16 a = mm_lg<C>(X1 + wave * 32 * LX, LX, w.pw1 + col, 2 * C, zero16(), lane);
            const float bs = w.pw1_b[col + lr];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wave * 32 + acc_row(r, lane);
                if (row < NR) Hd[row * LH + ct * 32 + lr] = leaky(a[r] + bs);
            }
        }
        __syncthreads();
        {
            const int px = tid >> 2, py = px >> 3, pxx = px & 7, cg = (tid & 3) * 8;
            int at[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ry = min(max(y0 + py + t / 3 - 1, 0), hm - 1) - (y0 - 1), rx = min(max(x0 + pxx + t % 3 - 1, 0), wm - 1) - (x0 - 1);
                at[t] = (ry * R + rx) * LH;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = cg + i, ca = j * 32 + c, cb = C + j * 32 + c;
                float a = w.dw_b[ca], g = w.dw_b[cb];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    a = fmaf(Hd[at[t] + c], w.dw[t * 2 * C + ca], a);
                    g = fmaf(Hd[at[t] + 32 + c], w.dw[t * 2 * C + cb], g);
                }
                G[px * LG + c] = a * sigmoidf(g);
            }
        }
        __syncthreads();
        if (own) oacc = mm_lg<32>(G + ort * 32 * LG, LG, w.pw2 + j * 32 * C + oct * 32, C, oacc, lane);
        __syncthreads();
    }
    if (own) {
        const float bs = w.pw2_b[oct * 32 + lr];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = ort * 32 + acc_row(r, lane);
            const long long o = ((long long)(y0 + (t >> 3)) * wm + x0 + (t & 7)) * C + oct * 32 + lr;
            out[(long long)b * hm * wm * C + o] = xb[o] + (oacc[r] + bs);
        }
    }
}

// out [M][COUT] = A [M][CIN] * W [CIN][COUT] + bias (+ skip [M][COUT]); 64 rows a workgroup, M % 64 == 0
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void op_pw(const float *A, const float *W, const float *bias, const float *skip, float *out) {
    constexpr int NCT = COUT / 32, NT = 2 * NCT, LX = CIN + 1;
    __shared__ float X[kTok * LX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31;
    const long long m0 = (long long)blockIdx.x * kTok;
    for (int i = tid; i < kTok * CIN / 4; i += 256) {
        const int t = i / (CIN / 4), c = (i - t * (CIN / 4)) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(A + (m0 + t) * CIN + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) X[t * LX + c + e] = v[e];
    }
    __syncthreads();
    if (wave >= NT) return;
    const int rt = wave / NCT, ct = wave % NCT;
    const f32x16 a = mm_lg<CIN>(X + rt * 32 * LX, LX, W + ct * 32, COUT, zero16(), lane);
    const float bs = bias[ct * 32 + lr];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long o = (m0 + rt * 32 + acc_row(r, lane)) * COUT + ct * 32 + lr;
        const float v = a[r] + bs;
        out[o] = skip ? skip[o] + v : v;
    }
}

// the 1x1 conv 64 -> 3 of ToImageBilinaer on the map: [M][64] -> [M][3]; w [3][64]
__global__ __launch_bounds__(256) void op_proj3(const float *A, const float *w, const float *bias, float *out, long long M) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * 3) return;
    const long long m = idx / 3;
    const int o = (int)(idx - m * 3);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(A + m * 64 + c), wt = *reinterpret_cast<const f32x4 *>(w + o * 64 + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(v[e], wt[e], acc);
    }
    out[idx] = acc + bias[o];
}

// z of the net at (y, x) of its (Hp, Wp) output: the x8 bilinear upsample of the map p [hm][wm][3]
__device__ __forceinline__ float up8(const float *p, int hm, int wm, int y, int x, int c) {
    const Lerp ly = lerp_index(y, 0.125f, hm), lx = lerp_index(x, 0.125f, wm);
    const float *r0 = p + (long long)ly.i0 * wm * 3 + c, *r1 = p + (long long)ly.i1 * wm * 3 + c;
    return lerp2(ly, lx, r0[lx.i0 * 3], r0[lx.i1 * 3], r1[lx.i0 * 3], r1[lx.i1 * 3]);
}

__global__ __launch_bounds__(256) void op_exit(const float *x, const unsigned char *mask, const float *proj, float *out, const Geo g,
                                               int mode) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, plane = (long long)g.H * g.W;
    if (idx >= g.B * plane) return;
    const int b = (int)(idx / plane), p = (int)(idx - b * plane), y = p / g.W, xx = p - y * g.W;
    const int hm = g.Hp / kWin, wm = g.Wp / kWin;
    const float *pb = proj + (long long)b * hm * wm * 3;
    const bool m = mask[idx] != 0;
    float z[3];
    if (g.resized) {
        const Lerp ly = lerp_index(y, g.ry, g.nh), lx = lerp_index(xx, g.rx, g.nw);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            z[c] = lerp2(ly, lx, up8(pb, hm, wm, ly.i0, lx.i0, c), up8(pb, hm, wm, ly.i0, lx.i1, c), up8(pb, hm, wm, ly.i1, lx.i0, c),
                         up8(pb, hm, wm, ly.i1, lx.i1, c));
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) z[c] = up8(pb, hm, wm, y, xx, c);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long o = (3 * b + c) * plane + p;
        float v;
        if (mode == MODE_RAW) {
            v = z[c];
        } else if (mode == MODE_COMPOSITE) {
            v = m ? fminf(fmaxf(z[c], 0.f), 1.f) : x[o];
        } else {
            const float mf = m ? 1.f : 0.f;
            v = fminf(fmaxf(x[o] * (1.f - mf) + z[c] * mf, 0.f), 1.f);
        }
        out[o] = v;
    }
}

// pass 4's EMA buffer (multipass_pipeline.py:452-471): one thread owns an element of the [3][H][W] buffer across the batch.
// coarse == NULL is the step before the net: out = the frames with NaN zeroed, mask0 = isnan of channel 0.
__global__ __launch_bounds__(256) void op_buffer(const float *frames, const float *coarse, float *buffer, const unsigned char *reset,
                                                 float d, float a, int B, long long hw, float *out, unsigned char *mask0) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, n = 3 * hw;
    if (i >= n) return;
    if (!coarse) {
        for (int j = 0; j < B; ++j) {
            const float f = frames[j * n + i];
            const bool nan = f != f;
            out[j * n + i] = nan ? 0.f : f;
            if (i < hw) mask0[j * hw + i] = nan;
        }
        return;
    }
    float buf = buffer[i];
    for (int j = 0; j < B; ++j) {
        const float cv = coarse[j * n + i], f = frames[j * n + i];
        if (reset[j]) buf = cv;
        buf = buf * d + cv * a;
        out[j * n + i] = fminf(fmaxf(f != f ? buf : f, 0.f), 1.f);
    }
    buffer[i] = buf;
}

struct Plan {
    Geo g;
    int hm, wm;
    long long off[10], total;       // in4, d1, d2, dct, enc, tmp, mid, dec, m32a, m32b (floats), then proj behind them
    long long proj;
};

int make_plan(int B, int H, int W, int max_size, Plan *p) {
    NUNIF_REQUIRE(B >= 1 && H >= 2 && W >= 2 && max_size >= 2 && (long long)B * H * W < (1LL << 28),
                  "outpaint: B = %d, H = %d, W = %d, max_size = %d", B, H, W, max_size);
    Geo &g = p->g;
    g.B = B; g.H = H; g.W = W; g.nh = H; g.nw = W; g.resized = 0;
    if ((H > W ? H : W) > max_size) {                 // :180-186, Python's round() is round-half-even on a double
        if (H > W) { g.nh = max_size; g.nw = (int)std::nearbyint(W * ((double)g.nh / H)); }
        else { g.nw = max_size; g.nh = (int)std::nearbyint(H * ((double)g.nw / W)); }
        g.resized = 1;
        NUNIF_REQUIRE(g.nh >= 1 && g.nw >= 1, "outpaint: the resized frame is empty");
    }
    g.Hp = (g.nh + kUnit - 1) / kUnit * kUnit; g.Wp = (g.nw + kUnit - 1) / kUnit * kUnit;
    g.padded = g.Hp != g.nh || g.Wp != g.nw;
    g.sy = (float)H / (float)g.nh; g.sx = (float)W / (float)g.nw;
    g.ry = (float)g.nh / (float)H; g.rx = (float)g.nw / (float)W;
    p->hm = g.Hp / kWin; p->wm = g.Wp / kWin;
    const long long full = (long long)B * g.Hp * g.Wp, map = (long long)B * p->hm * p->wm;
    NUNIF_REQUIRE(full < (1LL << 28), "outpaint: the padded batch is too large");
    const long long n[10] = {full * 4, full / 4 * 8, full / 16 * 16, map * 64, map * 64, map * 64, map * 64, map * 64, map * 32, map * 32};
    long long at = 0;
    for (int i = 0; i < 10; ++i) { p->off[i] = at; at += n[i]; }
    p->proj = at;
    p->total = at + ((map * 3 + 3) & ~3LL);
    return NUNIF_HIP_OK;
}

}  // namespace
}  // namespace nunif

using namespace nunif;

struct nunif_outpaint : DeviceOwner {
    struct { float *w, *b; } dct[3], proj_mid, proj_out, to_image;
    MhaW mha[4];                   // enc, mid 0, mid 1, dec
    PoolW pool[4];
};

namespace {

int fetch(nunif_outpaint *h, const TensorMap &m, const std::string &key, size_t n, const float **dst) {
    const HostTensor *t = nullptr;
    int rc = find(m, key, &t);
    if (rc) return rc;
    NUNIF_REQUIRE((size_t)t->numel == n, "outpaint_create: '%s' has %lld elements, expected %zu", key.c_str(), (long long)t->numel, n);
    float *p = nullptr;
    if ((rc = h->upload_f32(t, &p))) return rc;
    *dst = p;
    return NUNIF_HIP_OK;
}

const char *const kBlocks[4] = {"enc", "mid0", "mid1", "dec"};
const int kBlockC[4] = {64, 32, 32, 64};

int load(nunif_outpaint *h, const TensorMap &m) {
    int rc;
    const int dc[4] = {4, 8, 16, 64};
    for (int i = 0; i < 3; ++i) {
        const std::string p = "dct." + std::to_string(i);
        if ((rc = fetch(h, m, p + ".w", (size_t)9 * dc[i] * dc[i + 1], (const float **)&h->dct[i].w))) return rc;
        if ((rc = fetch(h, m, p + ".b", dc[i + 1], (const float **)&h->dct[i].b))) return rc;
    }
    for (int i = 0; i < 4; ++i) {
        const size_t C = kBlockC[i];
        const std::string a = std::string(kBlocks[i]) + ".mha.", q = std::string(kBlocks[i]) + ".pool.";
        MhaW &w = h->mha[i];
        PoolW &pw = h->pool[i];
        struct { const std::string key; size_t n; const float **dst; } parts[] = {
            {a + "qkv.w", C * 3 * C, &w.qkv}, {a + "qkv.b", 3 * C, &w.qkv_b}, {a + "table", (size_t)kTok * kTok, &w.table},
            {a + "proj.w", C * C, &w.proj}, {a + "proj.b", C, &w.proj_b}, {a + "mlp1.w", C * 2 * C, &w.mlp1},
            {a + "mlp1.b", 2 * C, &w.mlp1_b}, {a + "mlp2.w", C * C, &w.mlp2}, {a + "mlp2.b", C, &w.mlp2_b},
            {q + "pw1.w", C * 2 * C, &pw.pw1}, {q + "pw1.b", 2 * C, &pw.pw1_b}, {q + "dw.w", 9 * 2 * C, &pw.dw},
            {q + "dw.b", 2 * C, &pw.dw_b}, {q + "pw2.w", C * C, &pw.pw2}, {q + "pw2.b", C, &pw.pw2_b}};
        for (auto &part : parts)
            if ((rc = fetch(h, m, part.key, part.n, part.dst))) return rc;
    }
    if ((rc = fetch(h, m, "proj_mid.w", 64 * 32, (const float **)&h->proj_mid.w))) return rc;
    if ((rc = fetch(h, m, "proj_mid.b", 32, (const float **)&h->proj_mid.b))) return rc;
    if ((rc = fetch(h, m, "proj_out.w", 32 * 64, (const float **)&h->proj_out.w))) return rc;
    if ((rc = fetch(h, m, "proj_out.b", 64, (const float **)&h->proj_out.b))) return rc;
    if ((rc = fetch(h, m, "to_image.w", 3 * 64, (const float **)&h->to_image.w))) return rc;
    return fetch(h, m, "to_image.b", 3, (const float **)&h->to_image.b);
}

template <int C>
int run_block(const nunif_outpaint *h, int i, const float *in, float *tmp, float *out, const Plan &p, hipStream_t s) {
    const unsigned wins = (unsigned)(p.g.B * (p.hm / kWin) * (p.wm / kWin));
    const double tok = (double)wins * kTok;
    {
        ProfScope prof("outpaint_mha", s, 2.0 * tok * (6.0 * C * C + 2.0 * kTok * C), 0.0);
        hipLaunchKernelGGL(op_mha<C>, dim3(wins), dim3(256), 0, s, in, tmp, h->mha[i], p.hm, p.wm);
        NUNIF_LAUNCH_CHECK();
    }
    ProfScope prof("outpaint_pool", s, 2.0 * tok * 3.0 * C * C, 0.0);
    hipLaunchKernelGGL(op_pool<C>, dim3(wins), dim3(256), 0, s, (const float *)tmp, out, h->pool[i], p.hm, p.wm);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

}  // namespace

extern "C" void nunif_hip_outpaint_destroy(nunif_outpaint *h) {
    if (!h) return;
    h->free_all();
    delete h;
}

extern "C" int nunif_hip_outpaint_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_outpaint **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "outpaint_create: NULL argument");
    nunif_outpaint *h = new nunif_outpaint();
    const int rc = load(h, tensor_map(tensors, n_tensors));
    if (rc != NUNIF_HIP_OK) { nunif_hip_outpaint_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" int64_t nunif_hip_outpaint_work_bytes(int32_t B, int32_t H, int32_t W, int32_t max_size) {
    Plan p;
    if (make_plan(B, H, W, max_size, &p)) return -1;
    return p.total * (int64_t)sizeof(float);
}

extern "C" int nunif_hip_outpaint_infer(nunif_outpaint *h, const float *x, const uint8_t *mask, int32_t B, int32_t H, int32_t W,
                                        int32_t max_size, int32_t mode, float *out, void *work, void *stream) {
    NUNIF_REQUIRE(h && x && mask && out && work && x != out, "outpaint_infer: NULL argument (or out aliases x)");
    NUNIF_REQUIRE(mode == MODE_COMPOSITE || mode == MODE_RAW || mode == MODE_FORWARD, "outpaint_infer: mode %d", mode);
    NUNIF_REQUIRE(((uintptr_t)work & 15) == 0, "outpaint_infer: work must be 16-byte aligned");
    Plan p;
    int rc = make_plan(B, H, W, max_size, &p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *base = (float *)work;
    float *in4 = base + p.off[0], *d1 = base + p.off[1], *d2 = base + p.off[2], *dct = base + p.off[3], *enc = base + p.off[4],
          *tmp = base + p.off[5], *mid = base + p.off[6], *dec = base + p.off[7], *ma = base + p.off[8], *mb = base + p.off[9],
          *proj = base + p.proj;
    const Geo &g = p.g;
    const long long full = (long long)B * g.Hp * g.Wp, map = (long long)B * p.hm * p.wm;
    {
        ProfScope prof("outpaint_entry", s, 0.0, 16.0 * full);
        hipLaunchKernelGGL(op_entry, dim3((unsigned)((full + 255) / 256)), dim3(256), 0, s, x, mask, in4, g);
        NUNIF_LAUNCH_CHECK();
    }
    {
        ProfScope prof("outpaint_down", s, 2.0 * 9 * (full / 4 * 32.0 + full / 16 * 128.0 + full / 64 * 1024.0), 0.0);
        hipLaunchKernelGGL((op_down<4, 8>), dim3((unsigned)((full / 4 * 2 + 255) / 256)), dim3(256), 0, s, (const float *)in4,
                           (const float *)h->dct[0].w, (const float *)h->dct[0].b, d1, full / 4, g.Hp, g.Wp);
        NUNIF_LAUNCH_CHECK();
        hipLaunchKernelGGL((op_down<8, 16>), dim3((unsigned)((full / 16 * 4 + 255) / 256)), dim3(256), 0, s, (const float *)d1,
                           (const float *)h->dct[1].w, (const float *)h->dct[1].b, d2, full / 16, g.Hp / 2, g.Wp / 2);
        NUNIF_LAUNCH_CHECK();
        hipLaunchKernelGGL((op_down<16, 64>), dim3((unsigned)((full / 64 * 16 + 255) / 256)), dim3(256), 0, s, (const float *)d2,
                           (const float *)h->dct[2].w, (const float *)h->dct[2].b, dct, full / 64, g.Hp / 4, g.Wp / 4);
        NUNIF_LAUNCH_CHECK();
    }
    if ((rc = run_block<64>(h, 0, dct, tmp, enc, p, s))) return rc;
    const unsigned rows = (unsigned)(map / kTok);
    {
        ProfScope prof("outpaint_pw", s, 2.0 * map * 64 * 32, 0.0);
        hipLaunchKernelGGL((op_pw<64, 32>), dim3(rows), dim3(256), 0, s, (const float *)enc, (const float *)h->proj_mid.w,
                           (const float *)h->proj_mid.b, (const float *)nullptr, ma);
        NUNIF_LAUNCH_CHECK();
    }
    if ((rc = run_block<32>(h, 1, ma, mb, ma, p, s))) return rc;
    if ((rc = run_block<32>(h, 2, ma, mb, ma, p, s))) return rc;
    {
        ProfScope prof("outpaint_pw", s, 2.0 * map * 64 * 32, 0.0);
        hipLaunchKernelGGL((op_pw<32, 64>), dim3(rows), dim3(256), 0, s, (const float *)ma, (const float *)h->proj_out.w,
                           (const float *)h->proj_out.b, (const float *)enc, mid);
        NUNIF_LAUNCH_CHECK();
    }
    if ((rc = run_block<64>(h, 3, mid, tmp, dec, p, s))) return rc;
    ProfScope prof("outpaint_exit", s, 0.0, 28.0 * B * H * W);
    hipLaunchKernelGGL(op_proj3, dim3((unsigned)((map * 3 + 255) / 256)), dim3(256), 0, s, (const float *)dec,
                       (const float *)h->to_image.w, (const float *)h->to_image.b, proj, map);
    NUNIF_LAUNCH_CHECK();
    hipLaunchKernelGGL(op_exit, dim3((unsigned)(((long long)B * H * W + 255) / 256)), dim3(256), 0, s, x, mask, (const float *)proj,
                       out, g, mode);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_outpaint_debug_taps(nunif_outpaint *h, const void *work, int32_t B, int32_t H, int32_t W, int32_t max_size,
                                             const char *name, float *out, int64_t capacity, int64_t *shape4, void *stream) {
    NUNIF_REQUIRE(h && work && name && out && shape4, "outpaint_debug_taps: NULL argument");
    Plan p;
    int rc = make_plan(B, H, W, max_size, &p);
    if (rc) return rc;
    const struct { const char *name; long long off; int c; } taps[] = {
        {"dct", p.off[3], 64}, {"enc", p.off[4], 64}, {"mid", p.off[6], 64}, {"dec", p.off[7], 64}, {"proj", p.proj, 3}};
    for (const auto &t : taps) {
        if (std::string(name) != t.name) continue;
        const int64_t n = (int64_t)B * p.hm * p.wm * t.c;
        NUNIF_REQUIRE(capacity >= n, "outpaint_debug_taps: %s needs %lld floats", name, (long long)n);
        shape4[0] = B; shape4[1] = p.hm; shape4[2] = p.wm; shape4[3] = t.c;
        NUNIF_HIP_CHECK(hipMemcpyAsync(out, (const float *)work + t.off, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice,
                                       (hipStream_t)stream));
        return NUNIF_HIP_OK;
    }
    set_error("outpaint_debug_taps: no tap named %s", name);
    return NUNIF_HIP_EINVAL;
}

extern "C" int nunif_hip_outpaint_buffer_step(const float *frames, const float *coarse, float *buffer, const uint8_t *reset,
                                              double buffer_decay, int32_t B, int32_t H, int32_t W, float *out, uint8_t *mask0,
                                              void *stream) {
    NUNIF_REQUIRE(frames && out && B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1LL << 28),
                  "outpaint_buffer_step: bad argument (B = %d, H = %d, W = %d)", B, H, W);
    NUNIF_REQUIRE(coarse ? (buffer && reset) : (mask0 != nullptr),
                  "outpaint_buffer_step: the step before the net needs mask0, the step after it buffer and reset");
    const long long hw = (long long)H * W;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("outpaint_buffer", s, 0.0, 12.0 * B * 3 * hw);
    hipLaunchKernelGGL(op_buffer, dim3((unsigned)((3 * hw + 255) / 256)), dim3(256), 0, s, frames, coarse, buffer, reset,
                       (float)buffer_decay, (float)(1.0 - buffer_decay), B, hw, out, mask0);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}
