// Baseline JPEG frame encoder for gfx950: what iw3.desktop's to_jpeg_data (iw3/desktop/utils.py:99-123, reference) does with
// torchvision's encode_jpeg, as four launches on one stream and no host synchronisation.  DESIGN.md ("JPEG frame encoder")
// states the encoder step by step; tests/jpeg_ref.py restates it in float64.
//
//   jpeg_dct_kernel<SS>     one MCU per 64 (4:2:0) or 32 (4:4:4) lanes: u = rint(clamp(x) * 255), full-range BT.601 YCbCr in fp32,
//                           edge replication, the 2 x 2 chroma mean, level shift, 8 x 8 orthonormal DCT-II (rows, then columns,
//                           through LDS), c / Q rounded half away from zero, clamped, stored in scan order (MCU by MCU, block by
//                           block, zigzag) as i16
//   jpeg_entropy_kernel     one wave per restart interval, 64 blocks at a time (one per lane): bit lengths, a wave scan, the codes
//                           OR-ed into an LDS bit buffer at their offsets, then a second wave scan over the buffer's words for the
//                           0xFF stuffing and the bytes out to the interval's staging slot.  The last bits (< 8) of a batch are
//                           carried into the next; the last byte of the interval is filled with 1-bits; RSTn or EOI follows.
//   jpeg_scan_kernel        one workgroup per frame: exclusive scan of the intervals' byte counts, the header, out_len
//   jpeg_gather_kernel      one wave per interval: the staging slot to its place behind the header
//
// The LDS bit buffer holds the worst case of 64 blocks (kMaxBlockBits each) whatever the interval length: an interval of any
// number of MCUs runs through it batch by batch.  A staging slot holds jpeg::interval_bound() bytes, the proven worst case, and
// every store into it is checked against that size all the same.  No float atomics, no atomics on global memory; the LDS atomics
// OR disjoint bits: the bytes depend on the input alone.
#include "common.h"
#include "jpeg_host.h"

namespace nunif {
namespace {

using namespace jpeg;

constexpr int kBatch = 64;                                       // blocks per pass of the entropy kernel: one per lane
constexpr int kBufWords = (7 + kBatch * kMaxBlockBits + 7 + 31) / 32 + 1;      // carried bits, the blocks, the fill; 13.0 KB
static_assert(kBufWords * 4 + 2 * 256 * 4 + 2 * 16 * 4 <= 16 * 1024, "entropy kernel: 16 KB of LDS, ten workgroups per CU");

__device__ const HuffTable kAcTab[2] = {huff_table(kAcLumaBits, kAcLumaVals), huff_table(kAcChromaBits, kAcChromaVals)};
__device__ const HuffTable kDcTab[2] = {huff_table(kDcLumaBits, kDcVals), huff_table(kDcChromaBits, kDcVals)};

// natural index -> zigzag position
__device__ const uint8_t kNatToZig[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                          41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                          46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// orthonormal DCT-II: kDct[k][n] = s(k) cos((2n + 1) k pi / 16), s(0) = sqrt(1/8), s(k) = 1/2
__device__ const float kDct[8][8] = {
    {0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f, 0.353553391f},
    {0.49039264f, 0.415734806f, 0.277785117f, 0.097545161f, -0.097545161f, -0.277785117f, -0.415734806f, -0.49039264f},
    {0.461939766f, 0.191341716f, -0.191341716f, -0.461939766f, -0.461939766f, -0.191341716f, 0.191341716f, 0.461939766f},
    {0.415734806f, -0.097545161f, -0.49039264f, -0.277785117f, 0.277785117f, 0.49039264f, 0.097545161f, -0.415734806f},
    {0.353553391f, -0.353553391f, -0.353553391f, 0.353553391f, 0.353553391f, -0.353553391f, -0.353553391f, 0.353553391f},
    {0.277785117f, -0.49039264f, 0.097545161f, 0.415734806f, -0.415734806f, -0.097545161f, 0.49039264f, -0.277785117f},
    {0.191341716f, -0.461939766f, 0.461939766f, -0.191341716f, -0.191341716f, 0.461939766f, -0.461939766f, 0.191341716f},
    {0.097545161f, -0.277785117f, 0.415734806f, -0.49039264f, 0.49039264f, -0.415734806f, 0.277785117f, -0.097545161f}};

// ---- colour, DCT, quantisation -------------------------------------------------------------------------------------------------------
struct DctArgs {
    const float *rgb;                // [B][3][H][W]
    int16_t *coef;                   // [B][mcus * bpm][64], zigzag
    int H, W, mcus_x, mcus;
    uint8_t q[2][64];                // luma, chroma; natural order
};

struct Ycc {
    float y, cb, cr;
};
__device__ __forceinline__ Ycc to_ycc(float r, float g, float b) {
    r = rintf(fminf(fmaxf(r, 0.f), 1.f) * 255.f);
    g = rintf(fminf(fmaxf(g, 0.f), 1.f) * 255.f);
    b = rintf(fminf(fmaxf(b, 0.f), 1.f) * 255.f);
    Ycc o;
    o.y = 0.299f * r + 0.587f * g + 0.114f * b;
    o.cb = -0.168735892f * r - 0.331264108f * g + 0.5f * b + 128.f;
    o.cr = 0.5f * r - 0.418687589f * g - 0.081312411f * b + 128.f;
    return o;
}

__device__ __forceinline__ void dct8(const float in[8], float out[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float a = 0.f;
#pragma unroll
        for (int n = 0; n < 8; ++n) a += kDct[k][n] * in[n];
        out[k] = a;
    }
}

template <int SS>
__global__ void __launch_bounds__(256) jpeg_dct_kernel(const DctArgs g) {
    constexpr int MS = SS == 420 ? 16 : 8, BPM = SS == 420 ? 6 : 3, TPM = SS == 420 ? 64 : 32, MPW = 256 / TPM;
    __shared__ float px[MPW][BPM][8][9];             // a row stride of 9 floats: the column pass reads 8 rows of one column
    __shared__ float tr[MPW][BPM][8][9];
    __shared__ __attribute__((aligned(4))) int16_t zz[MPW][BPM * 64];
    __shared__ float qf[2][64];
    const int t = threadIdx.x, ml = t / TPM, tl = t % TPM;
    if (t < 128) qf[t >> 6][t & 63] = (float)g.q[t >> 6][t & 63];
    const int m_raw = blockIdx.x * MPW + ml;
    const bool active = m_raw < g.mcus;
    const int m = active ? m_raw : g.mcus - 1;       // lanes past the last MCU repeat it and store nothing
    const int y0 = (m / g.mcus_x) * MS, x0 = (m % g.mcus_x) * MS;
    const long hw = (long)g.H * g.W;
    const float *r = g.rgb + (long)blockIdx.y * 3 * hw, *gr = r + hw, *bl = gr + hw;
    if (SS == 420) {
        const int qy = tl >> 3, qx = tl & 7;         // one 2 x 2 quad per lane
        float cb[4], cr[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int yy = 2 * qy + (d >> 1), xx = 2 * qx + (d & 1);
            const long o = (long)min(y0 + yy, g.H - 1) * g.W + min(x0 + xx, g.W - 1);
            const Ycc c = to_ycc(r[o], gr[o], bl[o]);
            px[ml][(yy >> 3) * 2 + (xx >> 3)][yy & 7][xx & 7] = c.y;
            cb[d] = c.cb;
            cr[d] = c.cr;
        }
        px[ml][4][qy][qx] = ((cb[0] + cb[1]) + (cb[2] + cb[3])) * 0.25f;
        px[ml][5][qy][qx] = ((cr[0] + cr[1]) + (cr[2] + cr[3])) * 0.25f;
    } else {
        const int yy = tl >> 2;                      // two adjacent pixels per lane
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int xx = (tl & 3) * 2 + d;
            const long o = (long)min(y0 + yy, g.H - 1) * g.W + min(x0 + xx, g.W - 1);
            const Ycc c = to_ycc(r[o], gr[o], bl[o]);
            px[ml][0][yy][xx] = c.y;
            px[ml][1][yy][xx] = c.cb;
            px[ml][2][yy][xx] = c.cr;
        }
    }
    __syncthreads();
    const int blk = tl >> 3, line = tl & 7;
    float in[8], out[8];
    if (blk < BPM) {                                 // rows
#pragma unroll
        for (int n = 0; n < 8; ++n) in[n] = px[ml][blk][line][n] - 128.f;
        dct8(in, out);
#pragma unroll
        for (int k = 0; k < 8; ++k) tr[ml][blk][line][k] = out[k];
    }
    __syncthreads();
    if (blk < BPM) {                                 // columns, quantisation
#pragma unroll
        for (int n = 0; n < 8; ++n) in[n] = tr[ml][blk][n][line];
        dct8(in, out);
        const int tab = (SS == 420 ? blk >= 4 : blk >= 1) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nat = k * 8 + line;
            float v = roundf(out[k] / qf[tab][nat]);             // ties away from zero
            v = nat == 0 ? fminf(fmaxf(v, -1024.f), 1023.f) : fminf(fmaxf(v, -1023.f), 1023.f);
            zz[ml][blk * 64 + kNatToZig[nat]] = (int16_t)(int)v;
        }
    }
    __syncthreads();
    if (active) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(g.coef) + ((long)blockIdx.y * g.mcus + m) * (BPM * 32);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(zz[ml]);
        for (int i = tl; i < BPM * 32; i += TPM) dst[i] = src[i];
    }
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------------
struct EntropyArgs {
    const int16_t *coef;             // [B][mcus * bpm][64]
    uint8_t *stage;                  // [B][intervals][slot]
    int32_t *count;                  // [B][intervals]: bytes of the interval, marker included
    int mcus, bpm, restart, intervals;
    long slot;
};

__device__ __forceinline__ int bit_size(int v) { return 32 - __clz(v < 0 ? -v : v); }            // 0 for 0
// the value bits of v in `size` bits: v itself, or v - 1 (the one's complement of |v|) for a negative v
__device__ __forceinline__ unsigned value_bits(int v, int size) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u); }

struct BitCounter {
    int n;
    __device__ __forceinline__ void put(unsigned, int len) { n += len; }
};

// Bits are gathered in a register and leave as whole words: the OR merges the first and the last word of a block with its
// neighbours', the words between are this lane's alone.
struct BitWriter {
    uint32_t *buf;
    unsigned long long acc;
    int w, n;
    __device__ __forceinline__ void start(uint32_t *b, int pos) { buf = b; w = pos >> 5; n = pos & 31; acc = 0ull; }
    __device__ __forceinline__ void put(unsigned v, int len) {                  // len <= 27, n < 32
        acc |= (unsigned long long)v << (64 - n - len);
        n += len;
        if (n >= 32) {
            atomicOr(&buf[w++], (uint32_t)(acc >> 32));
            acc <<= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(&buf[w], (uint32_t)(acc >> 32));
    }
};

template <class Sink>
__device__ __forceinline__ void code_block(const int16_t *blk, int pred, const uint32_t *dc, const uint32_t *ac, Sink &s) {
    const uint4 *p = reinterpret_cast<const uint4 *>(blk);
    int run = 0;
    for (int v = 0; v < 8; ++v) {
        const uint4 q = p[v];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = (int)(int16_t)(w[e >> 1] >> ((e & 1) * 16));
            if (v == 0 && e == 0) {
                const int diff = c - pred, size = bit_size(diff);
                const uint32_t h = dc[size];
                s.put(((h & 0xffffu) << size) | value_bits(diff, size), (int)(h >> 16) + size);
                continue;
            }
            if (c == 0) {
                ++run;
                continue;
            }
            for (; run >= 16; run -= 16) s.put(ac[0xF0] & 0xffffu, (int)(ac[0xF0] >> 16));         // ZRL
            const int size = bit_size(c);
            const uint32_t h = ac[(run << 4) | size];
            s.put(((h & 0xffffu) << size) | value_bits(c, size), (int)(h >> 16) + size);
            run = 0;
        }
    }
    if (run > 0) s.put(ac[0x00] & 0xffffu, (int)(ac[0x00] >> 16));              // EOB
}

__device__ __forceinline__ int wave_scan_inclusive(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ void stage_byte(uint8_t *st, long pos, long slot, unsigned v) {
    if (pos < slot) st[pos] = (uint8_t)v;
}

__global__ void __launch_bounds__(kBatch) jpeg_entropy_kernel(const EntropyArgs g) {
    __shared__ uint32_t buf[kBufWords];
    __shared__ uint32_t ac[2][256];
    __shared__ uint32_t dc[2][16];
    const int lane = threadIdx.x, it = blockIdx.x;
    for (int i = lane; i < 512; i += kBatch) ac[i >> 8][i & 255] = kAcTab[i >> 8].e[i & 255];
    if (lane < 32) dc[lane >> 4][lane & 15] = kDcTab[lane >> 4].e[lane & 15];
    __syncthreads();
    const int mcu0 = it * g.restart;
    const int nblk = min(g.restart, g.mcus - mcu0) * g.bpm;
    const long blk0 = (long)mcu0 * g.bpm;
    const int16_t *cf = g.coef + ((long)blockIdx.y * g.mcus * g.bpm + blk0) * 64;
    uint8_t *st = g.stage + ((long)blockIdx.y * g.intervals + it) * g.slot;
    int pin = 0;                     // bits carried into this batch (< 8), at the top of word 0
    uint32_t carry = 0;
    long outpos = 0;
    for (int j0 = 0; j0 < nblk; j0 += kBatch) {
        const int j = j0 + lane;
        const bool have = j < nblk;
        const int comp = j % g.bpm;                              // 4:2:0: 0..3 Y, 4 Cb, 5 Cr; 4:4:4: Y, Cb, Cr
        const int tab = (g.bpm == 6 ? comp >= 4 : comp >= 1) ? 1 : 0;
        // the block of the same component before this one; the predictor starts at 0 in every interval
        int prev = -1;
        if (g.bpm == 6 && comp < 4) prev = comp > 0 ? j - 1 : j - 3;
        else prev = j - g.bpm;
        const int pred = (have && prev >= 0) ? (int)cf[(long)prev * 64] : 0;
        BitCounter cnt{0};
        if (have) code_block(cf + (long)j * 64, pred, dc[tab], ac[tab], cnt);
        const int inc = wave_scan_inclusive(cnt.n, lane);
        const int total = __shfl(inc, 63);
        const bool last = j0 + kBatch >= nblk;
        int pend = pin + total;
        const int fill = last ? (8 - (pend & 7)) & 7 : 0;
        const int words = (pend + fill + 31) >> 5;               // <= kBufWords - 1
        __syncthreads();                                          // the previous batch's reads of buf
        for (int i = lane; i <= words; i += kBatch) buf[i] = i == 0 ? carry : 0u;
        __syncthreads();
        if (have) {
            BitWriter bw;
            bw.start(buf, pin + inc - cnt.n);
            code_block(cf + (long)j * 64, pred, dc[tab], ac[tab], bw);
            bw.finish();
        }
        if (lane == 0 && fill) {                                  // the interval's last byte, filled with 1-bits
            BitWriter bw;
            bw.start(buf, pend);
            bw.put((1u << fill) - 1u, fill);
            bw.finish();
        }
        pend += fill;
        __syncthreads();
        const int nbytes = pend >> 3;
        for (int w0 = 0; w0 * 4 < nbytes; w0 += kBatch) {         // stuffing: a byte 0xFF is followed by 0x00
            const int w = w0 + lane;
            const int valid = min(max(nbytes - 4 * w, 0), 4);
            const uint32_t word = valid > 0 ? buf[w] : 0u;
            int n = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < valid) n += ((word >> (24 - 8 * i)) & 255u) == 255u ? 2 : 1;
            const int sinc = wave_scan_inclusive(n, lane);
            long p = outpos + sinc - n;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < valid) {
                    const unsigned byte = (word >> (24 - 8 * i)) & 255u;
                    stage_byte(st, p++, g.slot, byte);
                    if (byte == 255u) stage_byte(st, p++, g.slot, 0u);
                }
            }
            outpos += __shfl(sinc, 63);
        }
        pin = pend & 7;
        carry = pin ? buf[nbytes >> 2] & (0xffu << (24 - 8 * (nbytes & 3))) : 0u;
        carry <<= 8 * (nbytes & 3);
    }
    if (lane == 0) {
        const bool eoi = it == g.intervals - 1;
        stage_byte(st, outpos, g.slot, 0xFFu);
        stage_byte(st, outpos + 1, g.slot, eoi ? 0xD9u : 0xD0u + (unsigned)(it & 7));
        g.count[(long)blockIdx.y * g.intervals + it] = (int32_t)min(outpos + 2, g.slot);
    }
}

// ---- compaction ----------------------------------------------------------------------------------------------------------------------
struct Header {
    uint8_t bytes[kHeaderBytes];
};

__global__ void __launch_bounds__(256) jpeg_scan_kernel(const int32_t *__restrict__ count, uint32_t *__restrict__ offset,
                                                        int intervals, const Header hdr, uint8_t *out, long capacity,
                                                        int32_t *out_len) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    count += (long)b * intervals;
    offset += (long)b * intervals;
    long run = 0;
    for (int i0 = 0; i0 < intervals; i0 += 256) {
        const int i = i0 + tid;
        const int v = i < intervals ? count[i] : 0;
        const int inc = wave_scan_inclusive(v, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        if (i < intervals) offset[i] = (uint32_t)(run + before + inc - v);
        run += all;
        __syncthreads();
    }
    const long total = kHeaderBytes + run;
    const bool fits = total <= capacity;
    if (tid == 0) out_len[b] = fits ? (int32_t)total : -1;
    if (fits)
        for (int i = tid; i < kHeaderBytes; i += 256) out[(long)b * capacity + i] = hdr.bytes[i];
}

__global__ void __launch_bounds__(256) jpeg_gather_kernel(const uint8_t *__restrict__ stage, const int32_t *__restrict__ count,
                                                          const uint32_t *__restrict__ offset, int intervals, long slot,
                                                          uint8_t *__restrict__ out, long capacity,
                                                          const int32_t *__restrict__ out_len) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int it = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= intervals || out_len[b] < 0) return;               // too small a capacity: nothing of the scan is written
    const long k = (long)b * intervals + it;
    const uint8_t *src = stage + k * slot;
    uint8_t *dst = out + (long)b * capacity + kHeaderBytes + offset[k];
    const int n = count[k];
    for (int i = lane; i < n; i += 64) dst[i] = src[i];
}

bool aligned256(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

int launch_dct(const float *rgb, int B, int H, int W, int quality, int ss, int16_t *coef, hipStream_t s) {
    const Geometry geo = geometry(H, W, ss, 1);
    DctArgs a;
    a.rgb = rgb; a.coef = coef; a.H = H; a.W = W; a.mcus_x = geo.mcus_x; a.mcus = (int)geo.mcus;
    quant_tables(quality, a.q[0], a.q[1]);
    if (ss == 420) jpeg_dct_kernel<420><<<dim3(cdiv(a.mcus, 4), B), 256, 0, s>>>(a);
    else jpeg_dct_kernel<444><<<dim3(cdiv(a.mcus, 8), B), 256, 0, s>>>(a);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

int check_frame(const char *who, const void *rgb, int B, int H, int W, int quality, int ss, int restart) {
    NUNIF_REQUIRE(rgb, "%s: NULL frame", who);
    NUNIF_REQUIRE(valid_frame(B, H, W, ss, restart),
                  "%s: B=%d H=%d W=%d subsampling=%d restart_mcus=%d is outside 1 <= B <= %d, 1 <= H, W <= %d, subsampling 420 | 444, "
                  "1 <= restart_mcus <= %d", who, B, H, W, ss, restart, kMaxBatch, kMaxDim, kMaxRestart);
    NUNIF_REQUIRE(quality >= 1 && quality <= 100, "%s: quality %d is outside 1..100", who, quality);
    return NUNIF_HIP_OK;
}

}  // namespace
}  // namespace nunif

using namespace nunif;

extern "C" int nunif_hip_jpeg_quant_tables(int32_t quality, uint8_t *luma, uint8_t *chroma) {
    NUNIF_REQUIRE(luma && chroma, "jpeg_quant_tables: NULL table");
    NUNIF_REQUIRE(jpeg::quant_tables(quality, luma, chroma), "jpeg_quant_tables: quality %d is outside 1..100", quality);
    return NUNIF_HIP_OK;
}

extern "C" int64_t nunif_hip_jpeg_header(int32_t H, int32_t W, int32_t quality, int32_t subsampling, int32_t restart_mcus,
                                         uint8_t *out, int64_t capacity) {
    NUNIF_REQUIRE(out && capacity >= jpeg::kHeaderBytes, "jpeg_header: the header needs %d bytes", jpeg::kHeaderBytes);
    const int n = jpeg::header(H, W, quality, subsampling, restart_mcus, out);
    NUNIF_REQUIRE(n > 0, "jpeg_header: H=%d W=%d quality=%d subsampling=%d restart_mcus=%d is refused", H, W, quality, subsampling,
                  restart_mcus);
    return n;
}

extern "C" int64_t nunif_hip_jpeg_max_bytes(int32_t H, int32_t W, int32_t subsampling, int32_t restart_mcus) {
    return jpeg::max_bytes(H, W, subsampling, restart_mcus);
}

extern "C" int64_t nunif_hip_jpeg_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t subsampling, int32_t restart_mcus) {
    return jpeg::workspace_bytes(B, H, W, subsampling, restart_mcus);
}

extern "C" int nunif_hip_jpeg_encode(const float *rgb, int32_t B, int32_t H, int32_t W, int32_t quality, int32_t subsampling,
                                     int32_t restart_mcus, uint8_t *out, int64_t capacity, int32_t *out_len, void *workspace,
                                     void *stream) {
    if (int e = check_frame("jpeg_encode", rgb, B, H, W, quality, subsampling, restart_mcus)) return e;
    NUNIF_REQUIRE(out && out_len && capacity >= 0, "jpeg_encode: NULL output or negative capacity");
    NUNIF_REQUIRE(workspace && aligned256(workspace), "jpeg_encode: the workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const jpeg::Geometry geo = jpeg::geometry(H, W, subsampling, restart_mcus);
    const jpeg::Workspace ws = jpeg::workspace(B, H, W, subsampling, restart_mcus);
    uint8_t *base = static_cast<uint8_t *>(workspace);
    int16_t *coef = reinterpret_cast<int16_t *>(base + ws.coef);
    int32_t *count = reinterpret_cast<int32_t *>(base + ws.count);
    uint32_t *offset = reinterpret_cast<uint32_t *>(base + ws.offset);
    uint8_t *stage = base + ws.stage;
    {
        ProfScope prof("jpeg_dct", s, 0.0, (double)B * (12.0 * H * W + 128.0 * geo.blocks));
        if (int e = launch_dct(rgb, B, H, W, quality, subsampling, coef, s)) return e;
    }
    EntropyArgs ea;
    ea.coef = coef; ea.stage = stage; ea.count = count; ea.mcus = (int)geo.mcus; ea.bpm = geo.bpm; ea.restart = restart_mcus;
    ea.intervals = (int)geo.intervals; ea.slot = (long)ws.slot;
    {
        ProfScope prof("jpeg_entropy", s, 0.0, 0.0);
        jpeg_entropy_kernel<<<dim3(ea.intervals, B), kBatch, 0, s>>>(ea);
        NUNIF_LAUNCH_CHECK();
    }
    Header hdr;
    jpeg::header(H, W, quality, subsampling, restart_mcus, hdr.bytes);
    {
        ProfScope prof("jpeg_scan", s, 0.0, 0.0);
        jpeg_scan_kernel<<<B, 256, 0, s>>>(count, offset, ea.intervals, hdr, out, (long)capacity, out_len);
        NUNIF_LAUNCH_CHECK();
    }
    ProfScope prof("jpeg_gather", s, 0.0, 0.0);
    jpeg_gather_kernel<<<dim3(cdiv(ea.intervals, 4), B), 256, 0, s>>>(stage, count, offset, ea.intervals, (long)ws.slot, out,
                                                                      (long)capacity, out_len);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

extern "C" int nunif_hip_jpeg_debug_coefficients(const float *rgb, int32_t B, int32_t H, int32_t W, int32_t quality,
                                                 int32_t subsampling, int16_t *coef, void *stream) {
    if (int e = check_frame("jpeg_debug_coefficients", rgb, B, H, W, quality, subsampling, 1)) return e;
    NUNIF_REQUIRE(coef && (reinterpret_cast<uintptr_t>(coef) & 3u) == 0, "jpeg_debug_coefficients: coef must be 4-byte aligned");
    return launch_dct(rgb, B, H, W, quality, subsampling, coef, (hipStream_t)stream);
}
