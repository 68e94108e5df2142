// TransNetV2 shot-boundary network (nunif/utils/transnetv2.py, reference) for gfx950, eval mode, fp32 throughout.
//
// The reference runs this net without autocast and thresholds its output, so operands and accumulation stay fp32: every
// matrix product goes through v_mfma_f32_32x32x2_f32 (exact fp32 inputs, a k-ordered fmaf chain per output element).
//
// Activations are channels-last [frame][h][w][c].  One window is
//   per DDCNN layer:  spatial GEMM   S[pixel][8F']   = im2col(x)[pixel][9*Cin] * Ws         (the four branches' (1,3,3) convs)
//                     temporal GEMM  y[pixel][dF'+f] = gather_t(S)[pixel][3*2F'] * Wt[d]    (branch d, dilation 2^d, BN folded)
//   the second layer of a block orders its rows (frame, pooled pixel, 2x2 corner): one lane's accumulator registers 4g..4g+3 are
//   the four corners of one pooling window, so relu + shortcut + AvgPool3d((1,2,2)) is the epilogue and the rows that the floor
//   of the pooling drops are never computed;
//   tail: spatial means, projection + L2 norm, 512-bin histograms, two 101-wide similarity bands with their Linear, fc1 (GEMM),
//   the two heads.
#include <map>
#include <string>
#include <vector>

#include "gemm_f32.h"
#include "host_weights.h"

namespace nunif {
namespace {

constexpr int kH0 = 27, kW0 = 48, kLookup = 101, kHeadIn = 4864, kD = 1024, kFeat = 448;

enum { A_PLAIN = 0, A_SPATIAL = 1, A_SPATIAL3 = 2, A_TEMPORAL = 3, A_TEMPORAL_POOL = 4 };
enum { E_STORE = 0, E_BIAS = 1, E_POOL = 2 };

struct GemmArgs {
    const float *A, *Bm, *bias, *shortcut;
    float *out;
    int M, N, K;                 // valid rows / output columns / k (B is zero padded to a multiple of kBK rows and of BN columns)
    int lda, ldb, ldo;           // row strides of A (plain: per row; spatial / temporal: channels per pixel), B, out
    int H, W, C;                 // spatial: image and input channels; temporal: C = 2F' (channels of one branch in S)
    int T, Hp, Wp;               // temporal: frames per window; pooled geometry
    long long out_bt_stride;     // E_POOL: floats per frame in the output
    int relu;
    int a_z, o_z;                // per-branch (blockIdx.z) column offsets into A / out and bias
    long long b_z;
};

// The temporal rows gather frames of one window: h = t, w = pixel inside the frame, base = first frame of the window.
template <int AMODE>
__device__ __forceinline__ RowInfo row_info(const GemmArgs &g, int m) {
    if (AMODE == A_PLAIN) return row_plain(m, g.M, g.lda);
    if (AMODE == A_SPATIAL || AMODE == A_SPATIAL3) return row_conv(m, g.M, g.H, g.W);
    RowInfo r;
    r.ok = m < g.M;
    if (!r.ok) m = 0;
    if (AMODE == A_TEMPORAL) {
        const int hw = g.H * g.W, bt = m / hw, p = m - bt * hw;
        r.h = bt % g.T;                                   // t
        r.w = p;                                          // pixel
        r.base = bt - r.h;                                // first frame of this window
    } else {
        // rows ordered (frame, pooled pixel, 2x2 corner)
        const int q = m & 3, mp = m >> 2, pp = g.Hp * g.Wp, bt = mp / pp, p = mp - bt * pp, ph = p / g.Wp, pw = p - ph * g.Wp;
        r.h = bt % g.T;
        r.w = (2 * ph + (q >> 1)) * g.W + 2 * pw + (q & 1);
        r.base = bt - r.h;
    }
    return r;
}

// Four consecutive k of row r starting at k (k % 4 == 0, inside one tap for the vector modes).
template <int AMODE>
__device__ __forceinline__ f32x4 load_a(const GemmArgs &g, const RowInfo &r, int k, int z) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!r.ok) return v;
    if (AMODE == A_PLAIN) {
        v = *reinterpret_cast<const f32x4 *>(g.A + r.base + k);
    } else if (AMODE == A_SPATIAL) {
        const int tap = k / g.C, c = k - tap * g.C, dh = tap / 3, hh = r.h + dh - 1, ww = r.w + (tap - dh * 3) - 1;
        if (hh >= 0 && hh < g.H && ww >= 0 && ww < g.W)
            v = *reinterpret_cast<const f32x4 *>(g.A + ((r.base * g.H + hh) * g.W + ww) * g.C + c);
    } else if (AMODE == A_SPATIAL3) {
        // the network input as handed in: planar [frame][3][H][W], k = tap * 3 + channel, K = 27
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = k + i, tap = kk / 3, c = kk - tap * 3, dh = tap / 3, hh = r.h + dh - 1, ww = r.w + (tap - dh * 3) - 1;
            if (kk < g.K && hh >= 0 && hh < g.H && ww >= 0 && ww < g.W)
                v[i] = g.A[((r.base * 3 + c) * g.H + hh) * g.W + ww];
        }
    } else {
        const int j = k / g.C, c = k - j * g.C, tt = r.h + ((j - 1) << z);
        if (tt >= 0 && tt < g.T)
            v = *reinterpret_cast<const f32x4 *>(g.A + ((r.base + tt) * (long long)(g.H * g.W) + r.w) * g.lda + z * g.a_z + c);
    }
    return v;
}

// C[M][N] = A[M][K] * B[K][N] on v_mfma_f32_32x32x2_f32.  4 waves as WM x WN, each TM x TN tiles of 32 x 32.
// A comes through load_a (implicit im2col / temporal gather), B is a plain row-major matrix.  LDS holds both tiles k-major
// ([k][row]) so that an MFMA operand is one conflict-free ds_read_b32; two LDS stages and a register stage hide the global loads.
// sp_gemm of superpoint.hip holds the same loop (gemm_f32.h says why it is written twice): change both.
template <int AMODE, int EMODE, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void tn_gemm(const GemmArgs g) {
    typedef GemmTile<WM, WN, TM, TN> Tile;
    constexpr int BM = Tile::BM, BN = Tile::BN, LDA = Tile::LDA, LDB = Tile::LDB;
    constexpr int APASS = Tile::APASS, BVEC = Tile::BVEC, BPASS = Tile::BPASS;
    static_assert(BM % 64 == 0, "tile shape");
    __shared__ float As[2][Tile::A_STAGE];
    __shared__ float Bs[2][Tile::B_STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WN, wn = wave % WN;
    const int z = blockIdx.z;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const float *Bz = g.Bm + z * g.b_z;

    const int kq = (tid & 3) * 4, arow = tid >> 2;
    RowInfo rows[APASS];
#pragma unroll
    for (int p = 0; p < APASS; ++p) rows[p] = row_info<AMODE>(g, m0 + p * 64 + arow);

    // acc is the running chain of at most kFlush k; tot collects the finished chains.  One chain over K = 2304 .. 4864 of
    // post-ReLU (same-sign) operands carries 4 - 8 x the error of a blocked sum, and the result is thresholded.
    f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; tot[i][j][r] = 0.f; }

    f32x4 ra[APASS], rb[BPASS];
    const int nk = (g.K + kBK - 1) / kBK;

    auto gload = [&](int kt) {
#pragma unroll
        for (int p = 0; p < APASS; ++p) ra[p] = load_a<AMODE>(g, rows[p], kt * kBK + kq, z);
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + p * 256;
            if (BVEC % 256 == 0 || idx < BVEC) {
                const int kr = idx / (BN / 4), nc = (idx - kr * (BN / 4)) * 4;
                rb[p] = *reinterpret_cast<const f32x4 *>(Bz + (long long)(kt * kBK + kr) * g.ldb + n0 + nc);
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int p = 0; p < APASS; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) As[buf][(kq + i) * LDA + p * 64 + arow] = ra[p][i];
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int idx = tid + p * 256;
            if (BVEC % 256 == 0 || idx < BVEC) {
                const int kr = idx / (BN / 4), nc = (idx - kr * (BN / 4)) * 4;
                *reinterpret_cast<f32x4 *>(&Bs[buf][kr * LDB + nc]) = rb[p];
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
            for (int i = 0; i < TM; ++i) a[i] = As[cur][(kk + lk) * LDA + (wm * TM + i) * 32 + lr];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[cur][(kk + lk) * LDB + (wn * TN + j) * 32 + lr];
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

    // acc_row() of gemm_f32.h, spelled out (through the function the epilogue compiles to other code): registers 4 q4 .. 4 q4 + 3
    // of a lane are rows 8 q4 + 4 lk .. + 3 of the 32 x 32 tile
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 32 + lr;
            if (n >= g.N) continue;
            const int mb = m0 + (wm * TM + i) * 32 + 4 * lk;
            const float bias = EMODE == E_STORE ? 0.f : g.bias[z * g.o_z + n];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int m = mb + 8 * q4;                     // rows m .. m+3 are registers 4 q4 .. 4 q4 + 3
                if (EMODE == E_POOL) {
                    if (m >= g.M) continue;
                    const int mp = m >> 2, pp = g.Hp * g.Wp, bt = mp / pp, p = mp - bt * pp, ph = p / g.Wp, pw = p - ph * g.Wp;
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int pix = (2 * ph + (q >> 1)) * g.W + 2 * pw + (q & 1);
                        const float sc = g.shortcut[((long long)bt * (g.H * g.W) + pix) * g.ldo + z * g.o_z + n];
                        s += fmaxf(tot[i][j][4 * q4 + q] + bias, 0.f) + sc;
                    }
                    g.out[bt * g.out_bt_stride + (long long)p * g.ldo + z * g.o_z + n] = s * 0.25f;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (m + q >= g.M) continue;
                        float v = tot[i][j][4 * q4 + q] + bias;
                        if (EMODE == E_BIAS && g.relu) v = fmaxf(v, 0.f);
                        g.out[(long long)(m + q) * g.ldo + z * g.o_z + n] = v;
                    }
                }
            }
        }
}

// ---- tail -------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float block_sum(float v, float *red) {        // every thread gets the sum; red: blockDim.x floats
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// feats[frame][off + c] = mean over the P pooled positions of x[frame][p][c]
__global__ void tn_spatial_mean(const float *x, long long bt_stride, int P, int C, float *feats, int off) {
    const int bt = blockIdx.x, c = threadIdx.x;
    if (c >= C) return;
    const float *px = x + bt * bt_stride + c;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += px[(long long)p * C];
    feats[(long long)bt * kFeat + off + c] = s / (float)P;
}

// FrameSimilarity.projection + F.normalize (transnetv2.py:244-245): 128 threads, one output each
__global__ __launch_bounds__(128) void tn_project(const float *feats, const float *wt, const float *b, float *out) {
    __shared__ float f[kFeat];
    __shared__ float red[128];
    const int bt = blockIdx.x, o = threadIdx.x;
    for (int k = o; k < kFeat; k += 128) f[k] = feats[(long long)bt * kFeat + k];
    __syncthreads();
    float a = b[o];
    for (int k = 0; k < kFeat; ++k) a = fmaf(f[k], wt[k * 128 + o], a);
    const float n2 = block_sum(a * a, red);
    out[(long long)bt * 128 + o] = a / fmaxf(sqrtf(n2), 1e-12f);
}

// ColorHistograms.compute_color_histograms (transnetv2.py:274-296): frames.int(), >> 5 per channel, 512 LDS counters per frame.
// A value outside 0..255 has no bin in the reference (its scatter index leaves the frame's 512 slots); it is not counted here.
__global__ __launch_bounds__(256) void tn_histogram(const float *frames, float *hist) {
    __shared__ int cnt[512];
    __shared__ float red[256];
    const int bt = blockIdx.x, tid = threadIdx.x;
    constexpr int HW = kH0 * kW0;
    cnt[tid] = 0; cnt[tid + 256] = 0;
    __syncthreads();
    const float *f = frames + (long long)bt * 3 * HW;
    for (int p = tid; p < HW; p += 256) {
        const float r = f[p], gq = f[HW + p], bq = f[2 * HW + p];
        if (r > -1.f && r < 256.f && gq > -1.f && gq < 256.f && bq > -1.f && bq < 256.f) {     // false for NaN
            const int bin = (((int)r >> 5) << 6) + (((int)gq >> 5) << 3) + ((int)bq >> 5);
            atomicAdd(&cnt[bin], 1);
        }
    }
    __syncthreads();
    const float h0 = (float)cnt[tid], h1 = (float)cnt[tid + 256];
    const float n2 = block_sum(h0 * h0 + h1 * h1, red);
    const float inv = 1.f / fmaxf(sqrtf(n2), 1e-12f);
    hist[(long long)bt * 512 + tid] = h0 * inv;
    hist[(long long)bt * 512 + tid + 256] = h1 * inv;
}

// The band of the T x T Gram matrix that the reference gathers (transnetv2.py:248-258 / :302-312): entry j of frame t is
// <x[t], x[t + j - 50]>, zero outside the window; then Linear(101 -> 128) + ReLU into the head's input row.
template <int D>
__global__ __launch_bounds__(256) void tn_band_fc(const float *x, int T, const float *wt, const float *b, float *head, int off) {
    __shared__ float band[kLookup];
    __shared__ float self[D];
    const int bt = blockIdx.x, t = bt % T, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < D; k += 256) self[k] = x[(long long)bt * D + k];
    __syncthreads();
    for (int j = wave; j < kLookup; j += 4) {
        const int t2 = t + j - (kLookup - 1) / 2;
        float s = 0.f;
        if (t2 >= 0 && t2 < T) {
            const float *y = x + (long long)(bt - t + t2) * D;
            for (int k = lane; k < D; k += 64) s = fmaf(self[k], y[k], s);
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        }
        if (lane == 0) band[j] = s;
    }
    __syncthreads();
    if (tid < 128) {
        float a = b[tid];
        for (int j = 0; j < kLookup; ++j) a = fmaf(band[j], wt[j * 128 + tid], a);
        head[(long long)bt * kHeadIn + off + tid] = fmaxf(a, 0.f);
    }
}

// cls_layer1 / cls_layer2 (transnetv2.py:82-85) and the detector's sigmoid of the first head
__global__ __launch_bounds__(256) void tn_heads(const float *h, const float *w1, const float *b1, const float *w2, const float *b2,
                                                float *one_hot, float *many_hot, float *sig) {
    __shared__ float red[256];
    const int bt = blockIdx.x, tid = threadIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int k = tid; k < kD; k += 256) {
        const float v = h[(long long)bt * kD + k];
        s1 = fmaf(v, w1[k], s1);
        s2 = fmaf(v, w2[k], s2);
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (tid == 0) {
        const float l1 = s1 + b1[0];
        one_hot[bt] = l1;
        if (many_hot) many_hot[bt] = s2 + b2[0];
        if (sig) sig[bt] = 1.f / (1.f + expf(-l1));
    }
}

struct Layer { float *ws = nullptr, *wt = nullptr, *bias = nullptr; int cin = 0, f = 0, kpad = 0, npad = 0; };

template <int AMODE, int EMODE, int WM, int WN, int TM, int TN>
void launch(const GemmArgs &g, int nz, hipStream_t s) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    dim3 grid(cdiv(g.M, BM), cdiv(g.N, BN), nz);
    hipLaunchKernelGGL((tn_gemm<AMODE, EMODE, WM, WN, TM, TN>), grid, dim3(256), 0, s, g);
}

}  // namespace
}  // namespace nunif

using namespace nunif;

struct nunif_transnetv2 : DeviceOwner {
    Layer layer[3][2];
    float *proj_wt = nullptr, *proj_b = nullptr, *sim_wt = nullptr, *sim_b = nullptr, *hist_wt = nullptr, *hist_b = nullptr;
    float *fc1_wt = nullptr, *fc1_b = nullptr, *cls1_w = nullptr, *cls1_b = nullptr, *cls2_w = nullptr, *cls2_b = nullptr;
    float *work = nullptr;
    size_t work_floats = 0;
};

namespace {
// floats of scratch per frame: S (largest spatial output), the first layer's output, pooled 1 / 2, head input, features,
// normalised projections, histograms, fc1 output
constexpr size_t kS = 27 * 48 * 128, kY1 = 27 * 48 * 64, kP1 = 13 * 24 * 64, kP2 = 6 * 12 * 128;
constexpr size_t kPerFrame = kS + kY1 + kP1 + kP2 + kHeadIn + kFeat + 128 + 512 + kD;

int fetch(nunif_transnetv2 *h, const std::map<std::string, const nunif_tensor_desc *> &m, const std::string &name, size_t n,
          float **dev) {
    auto it = m.find(name);
    if (it == m.end()) { set_error("transnetv2_create: packed tensor '%s' is missing", name.c_str()); return NUNIF_HIP_EMISSING; }
    size_t have = 1;
    for (int i = 0; i < it->second->ndim; ++i) have *= (size_t)it->second->shape[i];
    NUNIF_REQUIRE(have == n, "transnetv2_create: '%s' has %zu elements, expected %zu", name.c_str(), have, n);
    return h->upload(std::vector<float>(it->second->data, it->second->data + n), dev);
}
}  // namespace

extern "C" void nunif_hip_transnetv2_destroy(nunif_transnetv2 *h) {
    if (!h) return;
    h->free_all();
    if (h->work) (void)hipFree(h->work);
    delete h;
}

extern "C" int nunif_hip_transnetv2_create(const nunif_tensor_desc *tensors, int32_t n_tensors, int32_t filters,
                                           nunif_transnetv2 **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "transnetv2_create: NULL argument");
    if (filters != 16) { set_error("transnetv2_create: only F = 16 (L = 3, S = 2, D = 1024) is built, got F = %d", filters); return NUNIF_HIP_EUNSUPPORTED; }
    std::map<std::string, const nunif_tensor_desc *> m;
    for (int i = 0; i < n_tensors; ++i) m[tensors[i].name] = &tensors[i];
    nunif_transnetv2 *h = new nunif_transnetv2();
    int rc = NUNIF_HIP_OK;
#define TN_FETCH(name, n, dst) if (rc == NUNIF_HIP_OK) rc = fetch(h, m, name, n, dst)
    for (int b = 0; b < 3; ++b)
        for (int l = 0; l < 2; ++l) {
            Layer &L = h->layer[b][l];
            L.f = filters << b;
            L.cin = l == 1 ? 4 * L.f : (b == 0 ? 3 : 2 * L.f);
            L.kpad = cdiv(9 * L.cin, kBK) * kBK;
            L.npad = L.f < 32 ? 32 : L.f;
            const std::string p = "b" + std::to_string(b) + ".l" + std::to_string(l);
            TN_FETCH(p + ".ws", (size_t)L.kpad * 8 * L.f, &L.ws);
            TN_FETCH(p + ".wt", (size_t)4 * 6 * L.f * L.npad, &L.wt);
            TN_FETCH(p + ".bias", (size_t)4 * L.f, &L.bias);
        }
    TN_FETCH("proj.wt", (size_t)kFeat * 128, &h->proj_wt);
    TN_FETCH("proj.b", 128, &h->proj_b);
    TN_FETCH("sim.wt", (size_t)kLookup * 128, &h->sim_wt);
    TN_FETCH("sim.b", 128, &h->sim_b);
    TN_FETCH("hist.wt", (size_t)kLookup * 128, &h->hist_wt);
    TN_FETCH("hist.b", 128, &h->hist_b);
    TN_FETCH("fc1.wt", (size_t)kHeadIn * kD, &h->fc1_wt);
    TN_FETCH("fc1.b", kD, &h->fc1_b);
    TN_FETCH("cls1.w", kD, &h->cls1_w);
    TN_FETCH("cls1.b", 1, &h->cls1_b);
    TN_FETCH("cls2.w", kD, &h->cls2_w);
    TN_FETCH("cls2.b", 1, &h->cls2_b);
#undef TN_FETCH
    if (rc != NUNIF_HIP_OK) { nunif_hip_transnetv2_destroy(h); return rc; }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_transnetv2_forward(nunif_transnetv2 *h, const float *frames, int32_t B, int32_t T, float *one_hot,
                                            float *many_hot, float *sigmoid_out, void *stream) {
    NUNIF_REQUIRE(h && frames && one_hot, "transnetv2_forward: NULL argument");
    NUNIF_REQUIRE(B >= 1 && T >= 1 && (long long)B * T <= 4096, "transnetv2_forward: B = %d, T = %d (need B, T >= 1, B * T <= 4096)", B, T);
    hipStream_t s = (hipStream_t)stream;
    const int BT = B * T;
    const size_t need = (size_t)BT * kPerFrame;
    if (need > h->work_floats) {
        if (h->work) { NUNIF_HIP_CHECK(hipDeviceSynchronize()); (void)hipFree(h->work); h->work = nullptr; h->work_floats = 0; }
        if (hipMalloc((void **)&h->work, need * sizeof(float)) != hipSuccess) { set_error("hipMalloc(%zu) failed", need * sizeof(float)); return NUNIF_HIP_ENOMEM; }
        h->work_floats = need;
    }
    float *S = h->work, *Y1 = S + BT * kS, *P1 = Y1 + BT * kY1, *P2 = P1 + BT * kP1, *X = P2 + BT * kP2;
    float *feats = X + (size_t)BT * kHeadIn, *simn = feats + (size_t)BT * kFeat, *hist = simn + (size_t)BT * 128;
    float *hid = hist + (size_t)BT * 512;

    const float *in = frames;
    long long in_bt = 0;
    int H = kH0, W = kW0, foff = 0;
    for (int b = 0; b < 3; ++b) {
        const int Hp = H / 2, Wp = W / 2, F = h->layer[b][0].f;
        float *pooled = b == 0 ? P1 : b == 1 ? P2 : X + 256;
        const long long pooled_bt = b == 2 ? kHeadIn : (long long)Hp * Wp * 4 * F;
        for (int l = 0; l < 2; ++l) {
            const Layer &L = h->layer[b][l];
            ProfScope prof(l == 0 ? "transnetv2_ddcnn_a" : "transnetv2_ddcnn_b", s,
                           2.0 * BT * H * W * (9.0 * L.cin * 8 * F + 6.0 * F * 4 * F), 0.0);
            GemmArgs g = {};
            g.A = l == 0 ? in : Y1; g.Bm = L.ws; g.out = S;
            g.M = BT * H * W; g.N = 8 * F; g.K = 9 * L.cin; g.ldb = 8 * F; g.ldo = 8 * F;
            g.H = H; g.W = W; g.C = L.cin; g.T = T;
            if (L.cin == 3) launch<A_SPATIAL3, E_STORE, 2, 2, 2, 2>(g, 1, s);
            else if (b == 2) launch<A_SPATIAL, E_STORE, 2, 2, 1, 2>(g, 1, s);
            else launch<A_SPATIAL, E_STORE, 2, 2, 2, 2>(g, 1, s);
            NUNIF_LAUNCH_CHECK();

            GemmArgs t = {};
            t.A = S; t.Bm = L.wt; t.bias = L.bias;
            t.N = F; t.K = 6 * F; t.lda = 8 * F; t.ldb = L.npad; t.ldo = 4 * F;
            t.H = H; t.W = W; t.C = 2 * F; t.T = T; t.Hp = Hp; t.Wp = Wp;
            t.a_z = 2 * F; t.o_z = F; t.b_z = (long long)6 * F * L.npad;
            if (l == 0) {
                t.out = Y1; t.M = BT * H * W; t.relu = 1;
                if (F >= 64) launch<A_TEMPORAL, E_BIAS, 4, 1, 2, 2>(t, 4, s);
                else launch<A_TEMPORAL, E_BIAS, 4, 1, 2, 1>(t, 4, s);
            } else {
                t.out = pooled; t.shortcut = Y1; t.M = BT * Hp * Wp * 4; t.out_bt_stride = pooled_bt;
                if (F >= 64) launch<A_TEMPORAL_POOL, E_POOL, 4, 1, 2, 2>(t, 4, s);
                else launch<A_TEMPORAL_POOL, E_POOL, 4, 1, 2, 1>(t, 4, s);
            }
            NUNIF_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(tn_spatial_mean, dim3(BT), dim3(256), 0, s, pooled, pooled_bt, Hp * Wp, 4 * F, feats, foff);
        NUNIF_LAUNCH_CHECK();
        foff += 4 * F;
        in = pooled; in_bt = pooled_bt; H = Hp; W = Wp;
    }
    (void)in_bt;
    {
        ProfScope prof("transnetv2_tail", s, 2.0 * BT * ((double)kHeadIn * kD), 0.0);
        hipLaunchKernelGGL(tn_project, dim3(BT), dim3(128), 0, s, feats, h->proj_wt, h->proj_b, simn);
        NUNIF_LAUNCH_CHECK();
        hipLaunchKernelGGL(tn_histogram, dim3(BT), dim3(256), 0, s, frames, hist);
        NUNIF_LAUNCH_CHECK();
        hipLaunchKernelGGL(tn_band_fc<512>, dim3(BT), dim3(256), 0, s, hist, T, h->hist_wt, h->hist_b, X, 0);
        NUNIF_LAUNCH_CHECK();
        hipLaunchKernelGGL(tn_band_fc<128>, dim3(BT), dim3(256), 0, s, simn, T, h->sim_wt, h->sim_b, X, 128);
        NUNIF_LAUNCH_CHECK();
        GemmArgs g = {};
        g.A = X; g.Bm = h->fc1_wt; g.bias = h->fc1_b; g.out = hid;
        g.M = BT; g.N = kD; g.K = kHeadIn; g.lda = kHeadIn; g.ldb = kD; g.ldo = kD; g.relu = 1;
        launch<A_PLAIN, E_BIAS, 4, 1, 1, 1>(g, 1, s);
        NUNIF_LAUNCH_CHECK();
        hipLaunchKernelGGL(tn_heads, dim3(BT), dim3(256), 0, s, hid, h->cls1_w, h->cls1_b, h->cls2_w, h->cls2_b, one_hot, many_hot,
                           sigmoid_out);
        NUNIF_LAUNCH_CHECK();
    }
    return NUNIF_HIP_OK;
}
