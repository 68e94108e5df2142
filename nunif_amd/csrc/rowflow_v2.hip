// iw3 "sbs.row_flow_v2" (--method row_flow_v2, the 2024 default) on gfx950: depth planes -> horizontal flow, ONE launch.
//
// Reference: iw3/models/row_flow_v2.py — RowFlowV2.__init__ :13-36 (feature: replicate pad + 1x3 conv 3->16 + ReLU;
// non_overlap: 1x1 conv 16->1; overlap_residual: three replicate-padded 1x9 convs 16->16->32->32 with ReLU and a
// replicate-padded 3x3 conv 32->1), _forward :44-48 (delta = non_overlap + overlap_residual), _forward_delta_only :80-86
// (replicate pad 28, net, crop 28).
//
// The pad of 28 is wider than the net's receptive radius (14 columns, 1 row), so no pixel inside the crop sees one of the inner
// ReplicationPad2d layers: the function is the UNPADDED stack evaluated on the input with clamped coordinates, every
// activation outside the image being computed from the clamped input (not copied from the edge activation).  A tile that
// clamps only when it loads its input halo and computes every layer over the whole halo is therefore exact.
//
// One workgroup (256 threads) owns R x T = 5 x 62 output pixels at a time (persistent grid) and keeps every activation in LDS
// as fp16, channel-innermost ([row][column][C]):
//   stage 0  x planes, clamped (and mirrored when flip), fp32 [3][7][90]                                    VALU
//   stem     feature  [7][88][16] = ReLU(1x3 conv), non_overlap [5][62] fp32 = 1x1 conv of the fp16 feature    VALU
//   L1       [7][80][16] = ReLU(1x9 conv 16->16)   MFMA 16x16x32 f16, K = 10 taps x 16 (tap 9 has zero weights)
//   L2       [7][80][32] = ReLU(1x9 conv 16->32)   MFMA, K = 160 likewise          (72 columns are meaningful)
//   L3       [7][64][32] = ReLU(1x9 conv 32->32)   MFMA, K = 9 taps x 32
//   head     delta = 3x3 conv 32->1 + non_overlap, fp32                                                          VALU
// Tap t of a 1x9 layer is the same LDS row read t columns further right: the B operand of lane (pixel n, group g) is one
// 16-byte read of 8 channels, no im2col copy.  The 33 weight fragments (33 KiB) live in registers for the whole kernel.
//
// Budget for two workgroups per CU: LDS 78720 B of 81920 (feature + L1 39424, aliased by L3 afterwards; L2 35840, aliased by
// the stage-0 planes before; non_overlap 1240; fp32 stem / head weights and biases 2208), <= 256 VGPRs (arch + acc).
// HBM traffic: (R+2)(T+28)/(RT) x 12 + 4 = 28.4 B per output pixel at most (most of the halo re-reads hit L2).
#include <cstring>
#include <vector>

#include "host_weights.h"

namespace nunif {
namespace rf2 {

constexpr int R = 5, T = 62, RH = R + 2;
constexpr int INW = T + 28;                                  // input columns x0-14 .. x0+T+13
constexpr int FW = 88, L1W = 88, L2W = 80, L3W = 64;         // allocated columns; column 0 is x0-13, x0-9, x0-5, x0-1
constexpr int L1C = 5, L2C = 5, L3C = 4;                     // computed 16-column tiles per row
constexpr int FL_BYTES = RH * (FW + L1W) * 16 * 2;           // feature, then L1
constexpr int L2_BYTES = RH * L2W * 32 * 2;
constexpr int NO_OFF = FL_BYTES + L2_BYTES;
constexpr int W_OFF = (NO_OFF + R * T * 4 + 15) / 16 * 16;
// fp32 weight block (floats): stem [co][ci][t], stem bias, non_overlap w, b, head [dy*3+dx][ci], head bias, L1 / L2 / L3 bias
constexpr int WS = 0, BS = 144, WN = 160, BN = 176, WH = 180, BH = 468, B1 = 472, B2 = 488, B3 = 520, NWF = 552;
constexpr int SMEM = W_OFF + NWF * 4;
constexpr int NFRAG = 5 + 10 + 18;
static_assert(RH * L3W * 32 * 2 <= FL_BYTES, "L3 aliases feature + L1");
static_assert(3 * RH * INW * 4 <= L2_BYTES, "the input planes alias L2");
static_assert(SMEM <= 81920, "two workgroups per CU");
static_assert(L1C * 16 + 8 <= FW && L2C * 16 + 8 <= L1W && L3C * 16 + 8 <= L2W, "tap 8 of the last tile stays inside the row");
static_assert(T + 26 <= FW && T + 18 <= L1C * 16 && T + 10 + 8 <= L1C * 16 && T + 2 <= L3C * 16, "halo widths");

struct Args {
    const float *x;          // [B,3,h,w]
    const f16 *wfrag;        // NFRAG fragments: L1 (5), L2 [nt][ks] (10), L3 [nt][ks] (18)
    const float *wf;         // NWF floats
    float *delta;            // [B,1,h,w]
    float *tap[6];           // debug: feature [B,16,h,w], relu1 [B,16,..], relu2 [B,32,..], relu3 [B,32,..], non_overlap, residual
    int B, h, w, flip, nty, ntx, n_tiles;
};

// One 1x9 layer over RH rows x CT column tiles: out[row][c][co] = ReLU(bias + sum_{t,ci} W[co][ci][t] * src[row][c + t][ci]).
template <int CIN, int NT, int KS>
__device__ __forceinline__ void conv9(const f16 *src, int src_w, f16 *dst, int dst_w, int ctiles, const f16x8 (&wr)[NT * KS],
                                      const float *bias, int wave, int lane) {
    const int n = lane & 15, g = lane >> 4;
    for (int item = wave; item < RH * ctiles; item += 4) {
        const int row = item / ctiles, c0 = (item - row * ctiles) * 16;
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = *reinterpret_cast<const f32x4 *>(bias + nt * 16 + 4 * g);
        const f16 *sp = src + (size_t)(row * src_w + c0 + n) * CIN;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            // k = tap * CIN + ci.  CIN = 16: a k-step is two taps, the tenth has zero weights and re-reads tap 8 (finite data)
            const int tap = CIN == 16 ? min(2 * ks + (g >> 1), 8) : ks;
            const int ci0 = CIN == 16 ? (g & 1) * 8 : g * 8;
            const f16x8 b = *reinterpret_cast<const f16x8 *>(sp + tap * CIN + ci0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = MFMA_16x16x32(wr[nt * KS + ks], b, acc[nt]);
        }
        f16 *dp = dst + (size_t)(row * dst_w + c0 + n) * (NT * 16) + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const f16x4 o = {(f16)fmaxf(acc[nt][0], 0.f), (f16)fmaxf(acc[nt][1], 0.f), (f16)fmaxf(acc[nt][2], 0.f),
                             (f16)fmaxf(acc[nt][3], 0.f)};
            *reinterpret_cast<f16x4 *>(dp + nt * 16) = o;
        }
    }
}

// debug: the R x T centre of an LDS map [RH][map_w][C] (column col0 is x0) -> global [B,C,h,w]
template <int C>
__device__ __forceinline__ void dump_map(const f16 *m, int map_w, int col0, float *out, int b, int y0, int x0, int h, int w, int tid) {
    for (int i = tid; i < C * R * T; i += 256) {
        const int x = i % T, t = i / T, r = t % R, c = t / R;
        if (y0 + r < h && x0 + x < w)
            out[(((size_t)b * C + c) * h + y0 + r) * w + x0 + x] = (float)m[((r + 1) * map_w + col0 + x) * C + c];
    }
}

template <bool DBG>
__global__ void __launch_bounds__(256, 2) rf2_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];       // static: gfx950 takes up to 160 KiB per workgroup
    f16 *sF = reinterpret_cast<f16 *>(smem);
    f16 *sL1 = sF + RH * FW * 16;
    f16 *sL3 = sF;
    f16 *sL2 = reinterpret_cast<f16 *>(smem + FL_BYTES);
    float *sIn = reinterpret_cast<float *>(smem + FL_BYTES);
    float *sNo = reinterpret_cast<float *>(smem + NO_OFF);
    float *sW = reinterpret_cast<float *>(smem + W_OFF);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int i = tid; i < NWF; i += 256) sW[i] = a.wf[i];            // (the first barrier of the tile loop covers it)
    f16x8 w1[5], w2[10], w3[18];
    {
        const f16x8 *wg = reinterpret_cast<const f16x8 *>(a.wfrag) + lane;
#pragma unroll
        for (int i = 0; i < 5; ++i) w1[i] = wg[i * 64];
#pragma unroll
        for (int i = 0; i < 10; ++i) w2[i] = wg[(5 + i) * 64];
#pragma unroll
        for (int i = 0; i < 18; ++i) w3[i] = wg[(15 + i) * 64];
    }

    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int tx = tile % a.ntx, t2 = tile / a.ntx;
        const int ty = t2 % a.nty, b = t2 / a.nty;
        const int y0 = ty * R, x0 = tx * T;
        const size_t plane = (size_t)a.h * a.w;

        // stage 0: the only place coordinates are clamped (and mirrored: the right eye runs on the flipped planes)
        for (int i = tid; i < 3 * RH * INW; i += 256) {
            const int c = i % INW, t = i / INW, r = t % RH, ci = t / RH;
            const int gy = min(max(y0 - 1 + r, 0), a.h - 1);
            int gx = min(max(x0 - 14 + c, 0), a.w - 1);
            if (a.flip) gx = a.w - 1 - gx;
            sIn[i] = a.x[((size_t)b * 3 + ci) * plane + (size_t)gy * a.w + gx];
        }
        __syncthreads();

        // stem: 1x3 conv 3 -> 16 + ReLU over the whole halo; non_overlap on the output pixels
        for (int p = tid; p < RH * FW; p += 256) {
            const int row = p / FW, f = p - row * FW;
            float in[9];
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                for (int t = 0; t < 3; ++t) in[ci * 3 + t] = sIn[(ci * RH + row) * INW + f + t];
            f16x8 o[2];
            float no = sW[BN];
#pragma unroll
            for (int co = 0; co < 16; ++co) {
                float acc = sW[BS + co];
#pragma unroll
                for (int k = 0; k < 9; ++k) acc = fmaf(in[k], sW[WS + co * 9 + k], acc);
                const f16 v = (f16)fmaxf(acc, 0.f);
                o[co >> 3][co & 7] = v;
                no = fmaf((float)v, sW[WN + co], no);
            }
            f16x8 *fp = reinterpret_cast<f16x8 *>(sF + (size_t)p * 16);
            fp[0] = o[0];
            fp[1] = o[1];
            if (row >= 1 && row <= R && f >= 13 && f < 13 + T) sNo[(row - 1) * T + f - 13] = no;
        }
        __syncthreads();
        if (DBG) {
            dump_map<16>(sF, FW, 13, a.tap[0], b, y0, x0, a.h, a.w, tid);
            for (int i = tid; i < R * T; i += 256) {
                const int x = i % T, r = i / T;
                if (y0 + r < a.h && x0 + x < a.w) a.tap[4][(size_t)b * plane + (size_t)(y0 + r) * a.w + x0 + x] = sNo[i];
            }
        }

        conv9<16, 1, 5>(sF, FW, sL1, L1W, L1C, w1, sW + B1, wave, lane);
        __syncthreads();
        if (DBG) dump_map<16>(sL1, L1W, 9, a.tap[1], b, y0, x0, a.h, a.w, tid);

        conv9<16, 2, 5>(sL1, L1W, sL2, L2W, L2C, w2, sW + B2, wave, lane);
        __syncthreads();
        if (DBG) dump_map<32>(sL2, L2W, 5, a.tap[2], b, y0, x0, a.h, a.w, tid);

        conv9<32, 2, 9>(sL2, L2W, sL3, L3W, L3C, w3, sW + B3, wave, lane);      // overwrites feature / L1
        __syncthreads();
        if (DBG) dump_map<32>(sL3, L3W, 1, a.tap[3], b, y0, x0, a.h, a.w, tid);

        // head: 3x3 conv 32 -> 1 (four lanes per pixel, 8 channels each) + non_overlap, all fp32
        for (int i = tid; i < (R * T * 4 + 255) / 256 * 256; i += 256) {
            const int q = i & 3, px = min(i >> 2, R * T - 1);
            const int r = px / T, x = px - r * T;
            float acc = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const f16x8 v = *reinterpret_cast<const f16x8 *>(sL3 + (size_t)((r + dy) * L3W + x + dx) * 32 + q * 8);
                    const float *wh = sW + WH + (dy * 3 + dx) * 32 + q * 8;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc = fmaf((float)v[j], wh[j], acc);
                }
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            if (q == 0 && (i >> 2) < R * T && y0 + r < a.h && x0 + x < a.w) {
                const size_t o = (size_t)b * plane + (size_t)(y0 + r) * a.w + x0 + x;
                const float res = acc + sW[BH];
                a.delta[o] = res + sNo[px];
                if (DBG) a.tap[5][o] = res;
            }
        }
        // (no barrier: the next tile's stage 0 writes the L2 region, which nobody reads after the L3 barrier; its stem writes
        // the feature / non_overlap regions only after the next barrier)
    }
}

}  // namespace rf2
}  // namespace nunif

using namespace nunif;

struct nunif_row_flow_v2 : DeviceOwner {
    f16 *wfrag = nullptr;
    float *wf = nullptr;
};

extern "C" int nunif_hip_row_flow_v2_create(const nunif_tensor_desc *tensors, int32_t n_tensors, nunif_row_flow_v2 **handle) {
    NUNIF_REQUIRE(tensors && handle && n_tensors > 0, "row_flow_v2_create: NULL argument");
    const TensorMap m = tensor_map(tensors, n_tensors);
    const HostTensor *wf, *bf, *wn, *bn, *w1, *b1, *w2, *b2, *w3, *b3, *wh, *bh, *ds;
    int rc;
    if ((rc = find(m, "feature.0.weight", &wf)) || (rc = find(m, "feature.0.bias", &bf)) ||
        (rc = find(m, "non_overlap.weight", &wn)) || (rc = find(m, "non_overlap.bias", &bn)) ||
        (rc = find(m, "overlap_residual.0.weight", &w1)) || (rc = find(m, "overlap_residual.0.bias", &b1)) ||
        (rc = find(m, "overlap_residual.2.weight", &w2)) || (rc = find(m, "overlap_residual.2.bias", &b2)) ||
        (rc = find(m, "overlap_residual.4.weight", &w3)) || (rc = find(m, "overlap_residual.4.bias", &b3)) ||
        (rc = find(m, "overlap_residual.6.weight", &wh)) || (rc = find(m, "overlap_residual.6.bias", &bh)) ||
        (rc = find(m, "delta_scale", &ds)))
        return rc;
    NUNIF_REQUIRE(wf->numel == 16 * 3 * 3 && bf->numel == 16 && wn->numel == 16 && bn->numel == 1 && w1->numel == 16 * 16 * 9 &&
                  b1->numel == 16 && w2->numel == 32 * 16 * 9 && b2->numel == 32 && w3->numel == 32 * 32 * 9 && b3->numel == 32 &&
                  wh->numel == 32 * 9 && bh->numel == 1, "row_flow_v2: unexpected layer shape");
    // 1x9 weights [co][ci][1][9] as MFMA A fragments, k = tap * Cin + ci (Cin = 16: padded to ten taps)
    auto pack9 = [](const HostTensor *t, int cout, int cin, int K) {
        const float *wd = t->data;
        return pack_nt_ks(cout, cout, K, [=](int n, int k) {
            const int tap = k / cin, ci = k % cin;
            return tap < 9 ? wd[((size_t)n * cin + ci) * 9 + tap] : 0.0f; }, false, 0);
    };
    std::vector<f16> frags = pack9(w1, 16, 16, 160);
    const std::vector<f16> f2 = pack9(w2, 32, 16, 160), f3 = pack9(w3, 32, 32, 288);
    frags.insert(frags.end(), f2.begin(), f2.end());
    frags.insert(frags.end(), f3.begin(), f3.end());
    NUNIF_REQUIRE(frags.size() == (size_t)rf2::NFRAG * kFragHalfs, "row_flow_v2: fragment count");
    std::vector<float> wv(rf2::NWF, 0.0f);
    std::copy(wf->data, wf->data + 144, wv.begin() + rf2::WS);
    std::copy(bf->data, bf->data + 16, wv.begin() + rf2::BS);
    std::copy(wn->data, wn->data + 16, wv.begin() + rf2::WN);
    wv[rf2::BN] = bn->data[0];
    for (int ci = 0; ci < 32; ++ci)
        for (int t = 0; t < 9; ++t) wv[rf2::WH + t * 32 + ci] = wh->data[ci * 9 + t];
    wv[rf2::BH] = bh->data[0];
    std::copy(b1->data, b1->data + 16, wv.begin() + rf2::B1);
    std::copy(b2->data, b2->data + 32, wv.begin() + rf2::B2);
    std::copy(b3->data, b3->data + 32, wv.begin() + rf2::B3);
    nunif_row_flow_v2 *h = new nunif_row_flow_v2();
    if ((rc = h->upload(frags, &h->wfrag)) || (rc = h->upload(wv, &h->wf))) {
        nunif_hip_row_flow_v2_destroy(h);
        return rc;
    }
    *handle = h;
    return NUNIF_HIP_OK;
}

extern "C" void nunif_hip_row_flow_v2_destroy(nunif_row_flow_v2 *h) {
    if (!h) return;
    h->free_all();
    delete h;
}

template <bool DBG>
static int launch_rf2(rf2::Args a, hipStream_t s) {
    a.nty = cdiv(a.h, rf2::R);
    a.ntx = cdiv(a.w, rf2::T);
    const long tiles = (long)a.B * a.nty * a.ntx;
    NUNIF_REQUIRE(tiles < (1L << 31), "row_flow_v2: map too large");
    a.n_tiles = (int)tiles;
    const double px = (double)a.B * a.h * a.w;
    ProfScope ps("rf2_kernel", s, 2.0 * 16560 * px, 16.0 * px);
    rf2::rf2_kernel<DBG><<<(unsigned)std::min(tiles, 512L), 256, 0, s>>>(a);     // two workgroups on each of 256 CUs
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_row_flow_v2_delta(nunif_row_flow_v2 *h, const float *x, float *delta, int32_t B, int32_t hh, int32_t ww,
                                           int32_t flip, void *stream) {
    NUNIF_REQUIRE(h && x && delta && B > 0 && hh > 0 && ww > 0, "row_flow_v2_delta: bad argument");
    rf2::Args a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.wfrag = h->wfrag; a.wf = h->wf; a.delta = delta; a.B = B; a.h = hh; a.w = ww; a.flip = flip ? 1 : 0;
    return launch_rf2<false>(a, (hipStream_t)stream);
}

extern "C" int nunif_hip_row_flow_v2_debug_taps(nunif_row_flow_v2 *h, const float *x, float *delta, float *feature, float *relu1,
                                                float *relu2, float *relu3, float *non_overlap, float *residual, int32_t B,
                                                int32_t hh, int32_t ww, int32_t flip, void *stream) {
    NUNIF_REQUIRE(h && x && delta && feature && relu1 && relu2 && relu3 && non_overlap && residual && B > 0 && hh > 0 && ww > 0,
                  "row_flow_v2_debug_taps: bad argument");
    rf2::Args a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.wfrag = h->wfrag; a.wf = h->wf; a.delta = delta; a.B = B; a.h = hh; a.w = ww; a.flip = flip ? 1 : 0;
    a.tap[0] = feature; a.tap[1] = relu1; a.tap[2] = relu2; a.tap[3] = relu3; a.tap[4] = non_overlap; a.tap[5] = residual;
    return launch_rf2<true>(a, (hipStream_t)stream);
}
