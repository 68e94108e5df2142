// Lossless PNG frame encoder for gfx950: what iw3 --export does per frame with libpng on a host thread pool (iw3/utils.py:224-244
// save_image, iw3/base_depth_model.py:197-210 save_normalized_depth, reference), as five launches on one stream and no host
// synchronisation.  DESIGN.md ("PNG frame encoder") states the stream; tests/png_ref.py restates it from the specifications.
//
//   png_filter_kernel<FORM>  (png_filter.h; the forms 4..6 are instantiated in png_planes.hip) one wave per row: quantise, try the five filter types, keep the one with the smallest sum of
//                            |byte as signed| (the lowest type on a tie), write the filtered row and its two Adler sums
//   png_hist_kernel          one workgroup per stripe, 4 096 filtered bytes per pass (16 per lane, one 16-byte load): the bytes
//                            that repeat the byte one pixel before them, the run position of every byte by a scan carried from
//                            pass to pass, the greedy tokens from that, their histogram in LDS
//   png_codes_kernel         one wave per stripe: the three length-limited canonical codes, the run-length coded code lengths, the
//                            block header bit-packed, the size of the stripe's deflate data
//   png_scan_kernel          one workgroup per frame: exclusive scan of the chunk sizes, out_len, the Adler-32 from the rows' sums,
//                            IEND
//   png_emit_kernel          one workgroup per stripe: the same token walk, bit lengths, a workgroup scan, the codes OR-ed into an
//                            LDS bit buffer, whole 16-byte groups out to the chunk's place in the body; the CRC-32 of the chunk
//                            from per-lane table CRCs of those groups, combined through multiplication by x^(128 k) mod P
//
// The size of every chunk is known from the histogram and the code lengths before a bit is emitted, so the stripes go straight to
// their place: there is no staging copy.  No float atomics, no atomics on global memory; the LDS atomics add integers and OR
// disjoint bits: the bytes depend on the input alone.  Every store is checked against the size it was promised.
#include "common.h"
#include "png_host.h"
#include "png_filter.h"

namespace nunif {
namespace {

using namespace png;
using namespace png_dev;

constexpr int kPass = kThreads * 16;                             // filtered bytes per pass of a stripe's workgroup
constexpr int kAhead = 17;                                       // 16-byte groups read past a pass: a match of 258 needs 257 + 1
constexpr int kEqWords = kThreads + 32;                          // 16 "repeats" bits per lane, the look-ahead, zero fill
constexpr int kBufWords = 2112;                                  // 16 front + 6 + 563 header + 7 680 (15 bits x 4 096) + 16 trailer
static_assert(16 + 6 + kHeaderWords * 4 + kPass * 15 / 8 + 8 + 16 <= kBufWords * 4, "emit kernel: the bit buffer holds one pass");
static_assert(kBufWords / 4 <= kCrcPieces, "emit kernel: one power of x per 16-byte group of the buffer");
static_assert(kBufWords * 4 + 256 * 4 + kCodeWords * 4 + 256 * 4 + kEqWords * 2 + 256 <= 16 * 1024, "emit kernel: 16 KB of LDS");

__device__ const CrcTable kCrcTab = crc_table();
__device__ const CrcPowers kCrcPow = crc_powers();
__device__ const uint16_t kLenBaseDev[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                             31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t kLenExtraDev[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint8_t kClOrderDev[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- the token walk ------------------------------------------------------------------------------------------------------------------
// A byte "repeats" when it equals the byte one pixel before it in the same stripe.  Let k be the number of repeating bytes that end
// right before a byte and m = k mod 258.  Greedy matching of the longest length at that one distance cuts every run of repeating
// bytes into pieces of 258 from its start on: a repeating byte with m = 0 starts a match of min(258, 1 + the repeating bytes after
// it) when that is at least 3 and is a literal otherwise; one with m = 1 is a literal when the byte after it does not repeat and
// is covered otherwise; one with m >= 2 is covered; a byte that does not repeat is a literal.

struct RunScan {                                                 // a lane's 16 bytes: all of them repeat; the repeating bytes at its end
    int full, v;
};
__device__ __forceinline__ RunScan run_join(RunScan a, RunScan b) {          // a, then b
    RunScan o;
    o.full = b.full ? a.full : 0;
    o.v = b.full ? a.v + b.v : b.v;
    return o;
}

// the repeating bytes from bit p of the look-ahead on, at most cap
__device__ __forceinline__ int ones_from(const uint16_t *eq, int p, int cap) {
    int n = 0;
    while (n < cap) {
        const int o = p & 15, avail = 16 - o;
        const unsigned stop = (~(unsigned)eq[p >> 4] & 0xffffu) >> o;
        const int z = stop ? min(__ffs((int)stop) - 1, avail) : avail;
        n += z;
        p += z;
        if (z < avail) break;
    }
    return min(n, cap);
}

struct StripeWalk {
    const uint8_t *d;                                            // the stripe's filtered bytes, 16-byte aligned
    int n;                                                       // how many (a stripe holds at most 8 192 x 32 769 bytes)
    int bpp;
    int carry;                                                   // repeating bytes that end right before this pass
};

// the 16 "repeats" bits of the bytes [off, off + 16), off a multiple of 16
__device__ __forceinline__ unsigned repeats16(const StripeWalk &w, int off, uint4 *bytes) {
    uint4 q = make_uint4(0, 0, 0, 0);
    unsigned mask = 0;
    if (off < w.n) {
        q = *reinterpret_cast<const uint4 *>(w.d + off);          // the slot is padded to 16 bytes
        const uint32_t before = off > 0 ? *reinterpret_cast<const uint32_t *>(w.d + off - 4) : 0u;
        const uint32_t wd[5] = {before, q.x, q.y, q.z, q.w};      // 20 bytes; the bytes of this lane start at byte 4
        const int valid = min(16, w.n - off);
        const int back = 8 * (4 - w.bpp);                        // bpp 1..4: the 16 bytes one pixel back start at byte 4 - bpp
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pw = (uint32_t)((((unsigned long long)wd[k + 1] << 32) | wd[k]) >> back);
            const uint32_t diff = wd[k + 1] ^ pw;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * k + j;
                if (i < valid && off + i >= w.bpp && ((diff >> (8 * j)) & 255u) == 0u) mask |= 1u << i;
            }
        }
    }
    if (bytes) *bytes = q;
    return mask;
}

// One pass: fills eq[] for the pass and its look-ahead, returns this lane's bytes, its mask and m at its first byte; updates the
// carry.  All 256 threads call it.
__device__ __forceinline__ void walk_prepare(StripeWalk &w, int pass0, uint16_t *eq, RunScan *wave_tot, uint4 *bytes, unsigned *mask,
                                             int *m_first) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int off = pass0 + t * 16;
    *mask = repeats16(w, off, bytes);
    __syncthreads();                                             // the previous pass's reads of eq and wave_tot
    eq[t] = (uint16_t)*mask;
    if (t < 32) eq[kThreads + t] = t < kAhead ? (uint16_t)repeats16(w, pass0 + kPass + t * 16, nullptr) : (uint16_t)0;
    RunScan s;
    s.full = *mask == 0xffffu;
    s.v = s.full ? 16 : __clz(~(*mask << 16));                   // the ones at the top of the 16 bits
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        RunScan p;
        p.full = __shfl_up(s.full, dlt);
        p.v = __shfl_up(s.v, dlt);
        if (lane >= dlt) s = run_join(p, s);
    }
    if (lane == 63) wave_tot[wave] = s;
    RunScan ex;
    ex.full = __shfl_up(s.full, 1);
    ex.v = __shfl_up(s.v, 1);
    if (lane == 0) {
        ex.full = 1;
        ex.v = 0;
    }
    __syncthreads();
    RunScan acc;
    acc.full = 0;
    acc.v = w.carry;
    RunScan mine = acc;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == wave) mine = acc;
        acc = run_join(acc, wave_tot[k]);
    }
    mine = run_join(mine, ex);
    *m_first = mine.v % kMaxMatch;
    w.carry = acc.v;
}

// The tokens that start in this lane's 16 bytes, in order: sink.literal(byte), sink.match(length).
template <class Sink>
__device__ __forceinline__ void walk_tokens(uint4 bytes, unsigned mask, int valid, int m, const uint16_t *eq, Sink &sink) {
    const unsigned long long lo = ((unsigned long long)bytes.y << 32) | bytes.x, hi = ((unsigned long long)bytes.w << 32) | bytes.z;
    const int bit0 = threadIdx.x * 16;
    for (int i = 0; i < valid; ++i) {
        const unsigned byte = (unsigned)((i < 8 ? lo : hi) >> (8 * (i & 7))) & 255u;
        if (!((mask >> i) & 1u)) {
            sink.literal(byte);
            m = 0;
            continue;
        }
        if (m == 0) {
            const int after = ones_from(eq, bit0 + i + 1, kMaxMatch - 1);
            if (after >= kMinMatch - 1) sink.match(1 + after);
            else sink.literal(byte);
        } else if (m == 1) {
            const int p = bit0 + i + 1;
            if (!((eq[p >> 4] >> (p & 15)) & 1u)) sink.literal(byte);
        }
        m = m + 1 == kMaxMatch ? 0 : m + 1;
    }
}

__device__ __forceinline__ int length_symbol_index(int length) {             // 0..28
    int k = 28;
    while (kLenBaseDev[k] > length) --k;
    return k;
}

struct HistSink {
    uint32_t *hist;
    const uint8_t *lsym;
    int dist_slot;
    __device__ __forceinline__ void literal(unsigned b) { atomicAdd(&hist[b], 1u); }
    __device__ __forceinline__ void match(int len) {
        atomicAdd(&hist[257 + lsym[len - kMinMatch]], 1u);
        atomicAdd(&hist[dist_slot], 1u);
    }
};

__device__ __forceinline__ StripeWalk stripe_walk(const Frame &f, const uint8_t *filt, long b, int s) {
    StripeWalk w;
    w.d = filt + (b * f.stripes + s) * f.stripe_stride;
    w.n = min(f.stripe_rows, f.H - s * f.stripe_rows) * (int)f.row;
    w.bpp = f.bpp;
    w.carry = 0;
    return w;
}

__global__ void __launch_bounds__(kThreads) png_hist_kernel(const uint8_t *__restrict__ filt, int32_t *__restrict__ hist_out,
                                                             const Frame f) {
    __shared__ uint32_t hist[kSymbolStride];
    __shared__ uint16_t eq[kEqWords];
    __shared__ uint8_t lsym[256];
    __shared__ RunScan wave_tot[4];
    const int t = threadIdx.x, s = blockIdx.x;
    const long b = blockIdx.y;
    for (int i = t; i < kSymbolStride; i += kThreads) hist[i] = i == 256 ? 1u : 0u;              // the end of block
    lsym[t] = (uint8_t)length_symbol_index(t + kMinMatch);
    StripeWalk w = stripe_walk(f, filt, b, s);
    HistSink sink{hist, lsym, kNumLit + f.bpp - 1};
    for (int pass0 = 0; pass0 < w.n; pass0 += kPass) {
        uint4 bytes;
        unsigned mask;
        int m;
        walk_prepare(w, pass0, eq, wave_tot, &bytes, &mask, &m);
        const int off = pass0 + t * 16;
        const int valid = max(0, min(16, w.n - off));
        walk_tokens(bytes, mask, valid, m, eq, sink);
    }
    __syncthreads();
    int32_t *dst = hist_out + (b * f.stripes + s) * kSymbolStride;
    for (int i = t; i < kNumLit + kNumDist; i += kThreads) dst[i] = (int32_t)hist[i];
}

// ---- the codes -----------------------------------------------------------------------------------------------------------------------
// Code lengths of n symbols limited to `limit` bits, by one wave.  The used symbols are ordered by (count, symbol) ascending.
// Huffman's algorithm runs in place over that order (Moffat and Katajainen): two queues, the leaves in order and the internal
// nodes by creation, the leaf first where a leaf and an internal node weigh the same.  The depths are counted per length, those
// above the limit folded into it; while the Kraft sum is too large one code of the limit is dropped and the deepest shorter
// length that has a code gives one up for two of the next length.  The symbols in order take the lengths from the longest on.
__device__ void build_lengths(const uint32_t *hist, int n, int limit, int32_t *lens, uint16_t *order, uint32_t *a, int *count,
                              int *n_used) {
    const int lane = threadIdx.x;
    if (lane == 0) *n_used = 0;
    for (int s = lane; s < n; s += 64) lens[s] = 0;
    __syncthreads();
    int mine = 0;
    for (int s = lane; s < n; s += 64) {
        const uint32_t c = hist[s];
        if (!c) continue;
        int rank = 0;
        for (int o = 0; o < n; ++o) {
            const uint32_t co = hist[o];
            rank += (co != 0 && (co < c || (co == c && o < s))) ? 1 : 0;
        }
        order[rank] = (uint16_t)s;
        ++mine;
    }
    mine = wave_sum(mine);
    __syncthreads();
    if (lane != 0) return;
    const int nu = mine;
    *n_used = nu;
    if (nu == 0) return;
    if (nu == 1) {
        lens[order[0]] = 1;
        return;
    }
    for (int i = 0; i < nu; ++i) a[i] = hist[order[i]];
    // phase 1: the weights of the internal nodes, then the parent of every internal node
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < nu - 1; ++next) {
        if (leaf >= nu || a[root] < a[leaf]) {
            a[next] = a[root];
            a[root++] = (uint32_t)next;
        } else {
            a[next] = a[leaf++];
        }
        if (leaf >= nu || (root < next && a[root] < a[leaf])) {
            a[next] += a[root];
            a[root++] = (uint32_t)next;
        } else {
            a[next] += a[leaf++];
        }
    }
    // phase 2: the depth of every internal node
    a[nu - 2] = 0;
    for (int next = nu - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
    // phase 3: the number of leaves at every depth, counted per (limited) length
    for (int i = 0; i <= 15; ++i) count[i] = 0;                   // count[] is LDS: it is indexed by a depth
    {
        int avail = 1, used = 0, depth = 0;
        root = nu - 2;
        while (avail > 0) {
            while (root >= 0 && (int)a[root] == depth) {
                ++used;
                --root;
            }
            while (avail > used) {
                count[min(depth, limit)] += 1;
                --avail;
            }
            avail = 2 * used;
            ++depth;
            used = 0;
        }
    }
    unsigned total = 0;
    for (int i = 1; i <= limit; ++i) total += (unsigned)count[i] << (limit - i);
    while (total > (1u << limit)) {
        count[limit] -= 1;
        for (int i = limit - 1; i > 0; --i)
            if (count[i]) {
                count[i] -= 1;
                count[i + 1] += 2;
                break;
            }
        total -= 1;
    }
    int k = 0;
    for (int i = limit; i >= 1; --i)
        for (int j = 0; j < count[i] && k < nu; ++j) lens[order[k++]] = i;
}

// RFC 1951 section 3.2.2; codes[s] = length << 16 | the code with its bits reversed (it is sent from its most significant bit on)
__device__ void canonical_codes(const int32_t *lens, int n, uint32_t *codes, unsigned *count, unsigned *next) {
    for (int i = 0; i < 16; ++i) count[i] = 0;
    for (int s = 0; s < n; ++s) count[lens[s]] += 1;
    count[0] = 0;
    unsigned code = 0;
    next[0] = 0;
    for (int bits = 1; bits < 16; ++bits) {
        code = (code + count[bits - 1]) << 1;
        next[bits] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int len = lens[s];
        codes[s] = len ? ((unsigned)len << 16) | (__brev(next[len]++) >> (32 - len)) : 0u;
    }
}

struct WordSink {                                                // one lane, plain stores into zeroed words
    uint32_t *w;
    int words, n;
    __device__ __forceinline__ void put(unsigned v, int len) {   // len <= 16
        if (len == 0) return;
        const int i = n >> 5, o = n & 31;
        if (i < words) w[i] |= v << o;
        if (o + len > 32 && i + 1 < words) w[i + 1] |= v >> (32 - o);
        n += len;
    }
};

__global__ void __launch_bounds__(64) png_codes_kernel(int32_t *__restrict__ hist_io, int32_t *__restrict__ lens_out,
                                                        uint32_t *__restrict__ codes_out, uint32_t *__restrict__ header_out,
                                                        int32_t *__restrict__ meta, const Frame f) {
    __shared__ uint32_t hist[kSymbolStride];
    __shared__ int32_t lens[kSymbolStride];
    __shared__ uint32_t codes[kSymbolStride];
    __shared__ uint16_t order[kNumLit];
    __shared__ uint32_t work[kNumLit];
    __shared__ uint16_t cl_syms[kNumLit + kNumDist];             // symbol | extra value << 8
    __shared__ uint32_t hdr[kHeaderWords];
    __shared__ int n_used, n_cl_syms, hlit, hdist;
    __shared__ int count[16];
    __shared__ unsigned next_code[16];
    const int lane = threadIdx.x;
    const long k = (long)blockIdx.y * f.stripes + blockIdx.x;
    for (int i = lane; i < kSymbolStride; i += 64) hist[i] = i < kNumLit + kNumDist ? (uint32_t)hist_io[k * kSymbolStride + i] : 0u;
    for (int i = lane; i < kHeaderWords; i += 64) hdr[i] = 0u;
    __syncthreads();
    build_lengths(hist, kNumLit, 15, lens, order, work, count, &n_used);
    __syncthreads();
    build_lengths(hist + kNumLit, kNumDist, 15, lens + kNumLit, order, work, count, &n_used);
    __syncthreads();
    if (lane == 0) {
        int hl = kNumLit, hd = kNumDist;
        while (hl > 257 && lens[hl - 1] == 0) --hl;
        while (hd > 1 && lens[kNumLit + hd - 1] == 0) --hd;
        hlit = hl;
        hdist = hd;
        // the lengths of both codes as one sequence: runs of zeros as 18 (11..138) and 17 (3..10), everything else as it is
        int n = 0, i = 0;
        const int total = hl + hd;
        auto at = [&](int j) { return j < hl ? lens[j] : lens[kNumLit + j - hl]; };
        while (i < total) {
            const int v = at(i);
            if (v != 0) {
                cl_syms[n++] = (uint16_t)v;
                hist[kNumLit + kNumDist + v] += 1;
                ++i;
                continue;
            }
            int z = 1;
            while (i + z < total && z < 138 && at(i + z) == 0) ++z;
            if (z >= 11) {
                cl_syms[n++] = (uint16_t)(18 | ((z - 11) << 8));
                hist[kNumLit + kNumDist + 18] += 1;
            } else if (z >= 3) {
                cl_syms[n++] = (uint16_t)(17 | ((z - 3) << 8));
                hist[kNumLit + kNumDist + 17] += 1;
            } else {
                z = 1;
                cl_syms[n++] = 0;
                hist[kNumLit + kNumDist] += 1;
            }
            i += z;
        }
        n_cl_syms = n;
    }
    __syncthreads();
    build_lengths(hist + kNumLit + kNumDist, kNumCl, 7, lens + kNumLit + kNumDist, order, work, count, &n_used);
    __syncthreads();
    if (lane == 0) {
        canonical_codes(lens, kNumLit, codes, (unsigned *)count, next_code);
        canonical_codes(lens + kNumLit, kNumDist, codes + kNumLit, (unsigned *)count, next_code);
        canonical_codes(lens + kNumLit + kNumDist, kNumCl, codes + kNumLit + kNumDist, (unsigned *)count, next_code);
        const int32_t *cl_len = lens + kNumLit + kNumDist;
        const uint32_t *cl_code = codes + kNumLit + kNumDist;
        int hclen = kNumCl;
        while (hclen > 4 && cl_len[kClOrderDev[hclen - 1]] == 0) --hclen;
        WordSink ws{hdr, kHeaderWords, 0};
        ws.put(0u, 1);                                           // BFINAL: the stored block behind carries it
        ws.put(2u, 2);                                           // BTYPE: dynamic Huffman codes
        ws.put((unsigned)(hlit - 257), 5);
        ws.put((unsigned)(hdist - 1), 5);
        ws.put((unsigned)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) ws.put((unsigned)cl_len[kClOrderDev[i]], 3);
        for (int i = 0; i < n_cl_syms; ++i) {
            const int sym = cl_syms[i] & 255, extra = cl_syms[i] >> 8;
            ws.put(cl_code[sym] & 0xffffu, (int)(cl_code[sym] >> 16));
            if (sym == 17) ws.put((unsigned)extra, 3);
            if (sym == 18) ws.put((unsigned)extra, 7);
        }
        meta[k * 4] = ws.n;
    }
    __syncthreads();
    // the bits of the tokens, the end of block included
    unsigned long long bits = 0;
    for (int s = lane; s < kNumLit; s += 64) {
        const int extra = s >= 257 ? kLenExtraDev[s - 257] : 0;
        bits += (unsigned long long)hist[s] * (unsigned)(lens[s] + extra);
    }
    for (int s = lane; s < kNumDist; s += 64) bits += (unsigned long long)hist[kNumLit + s] * (unsigned)lens[kNumLit + s];
    bits = wave_sum64(bits);
    if (lane == 0) {
        const unsigned long long all = (unsigned long long)meta[k * 4] + bits + 3ull;             // the stored block's header
        meta[k * 4 + 1] = (int32_t)((all + 7ull) / 8ull + 4ull);
    }
    for (int i = lane; i < kSymbolStride; i += 64) {
        lens_out[k * kSymbolStride + i] = i < kSymbols ? lens[i] : 0;
        hist_io[k * kSymbolStride + i] = i < kSymbols ? (int32_t)hist[i] : 0;
    }
    for (int i = lane; i < kCodeWords; i += 64) {
        uint32_t c = i < kNumLit ? codes[i] : 0u;
        if (i == kNumLit) c = codes[kNumLit + f.bpp - 1];                                         // the one distance in use
        codes_out[k * kCodeWords + i] = c;
    }
    for (int i = lane; i < kHeaderWords; i += 64) header_out[k * kHeaderWords + i] = hdr[i];
}

// ---- chunk offsets, Adler-32, IEND -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_scan_inclusive(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ long chunk_data_bytes(const int32_t *meta, int s, int stripes) {
    return (long)meta[s * 4 + 1] + (s == 0 ? 2 : 0) + (s == stripes - 1 ? 4 : 0);     // the zlib header, the Adler-32
}

__global__ void __launch_bounds__(kThreads) png_scan_kernel(int32_t *__restrict__ meta, const uint32_t *__restrict__ rowsum,
                                                             uint32_t *__restrict__ frame, const Frame f, uint8_t *out, long capacity,
                                                             int32_t *out_len) {
    __shared__ int wsum[4];
    __shared__ unsigned long long asum[4], bsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    meta += b * f.stripes * 4;
    long run = 0;
    for (int i0 = 0; i0 < f.stripes; i0 += kThreads) {
        const int i = i0 + tid;
        const int v = i < f.stripes ? (int)(12 + chunk_data_bytes(meta, i, f.stripes)) : 0;
        const int inc = wave_scan_inclusive(v, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        if (i < f.stripes) meta[i * 4 + 2] = (int32_t)(run + before + inc - v);
        run += all;
        __syncthreads();
    }
    // Adler-32 of all filtered bytes (RFC 1950) from the rows' sums: A = 1 + sum a_r, B = N + sum (b_r + a_r x bytes behind row r)
    unsigned long long sa = 0, sb = 0;
    for (int r = tid; r < f.H; r += kThreads) {
        const unsigned long long a = rowsum[(b * f.H + r) * 2], bb = rowsum[(b * f.H + r) * 2 + 1];
        const unsigned long long behind = ((unsigned long long)(f.H - 1 - r) * (unsigned long long)f.row) % 65521ull;
        sa += a;
        sb += (bb + a * behind) % 65521ull;
    }
    sa = wave_sum64(sa);
    sb = wave_sum64(sb);
    if (lane == 0) {
        asum[wave] = sa;
        bsum[wave] = sb;
    }
    __syncthreads();
    const long total = run + 12;
    const bool fits = total <= capacity;
    if (tid == 0) {
        const unsigned long long n = (unsigned long long)f.H * (unsigned long long)f.row;
        const unsigned long long A = (1ull + asum[0] + asum[1] + asum[2] + asum[3]) % 65521ull;
        const unsigned long long Bv = (n % 65521ull + bsum[0] + bsum[1] + bsum[2] + bsum[3]) % 65521ull;
        frame[b * 4] = (uint32_t)((Bv << 16) | A);
        out_len[b] = fits ? (int32_t)total : -1;
        if (fits) {
            uint8_t *p = out + b * capacity + run;
            const uint8_t iend[4] = {'I', 'E', 'N', 'D'};
            uint32_t c = 0xFFFFFFFFu;
            for (int i = 0; i < 4; ++i) {
                p[i] = 0;
                p[4 + i] = iend[i];
                c = kCrcTab.e[(c ^ iend[i]) & 255u] ^ (c >> 8);
            }
            c ^= 0xFFFFFFFFu;
            for (int i = 0; i < 4; ++i) p[8 + i] = (uint8_t)(c >> (24 - 8 * i));
        }
    }
}

// ---- the bits ------------------------------------------------------------------------------------------------------------------------
struct CountSink {
    const uint32_t *lit, *mtab;
    int dist_len, n;
    __device__ __forceinline__ void literal(unsigned b) { n += (int)(lit[b] >> 16); }
    __device__ __forceinline__ void match(int len) { n += (int)(mtab[len - kMinMatch] >> 24) + dist_len; }
};

// Bits leave least significant first (RFC 1951 section 3.1.1).  They are gathered in a register and leave as whole words: the OR
// merges the first and the last word of a lane with its neighbours', the words between are this lane's alone.
struct BitWriter {
    uint32_t *buf;
    unsigned long long acc;
    int w, n;
    __device__ __forceinline__ void start(uint32_t *b, int pos) { buf = b; w = pos >> 5; n = pos & 31; acc = 0ull; }
    __device__ __forceinline__ void put(unsigned v, int len) {                  // len <= 32, n < 32
        acc |= (unsigned long long)v << n;
        n += len;
        if (n >= 32) {
            if (w < kBufWords) atomicOr(&buf[w], (uint32_t)acc);
            ++w;
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0 && w < kBufWords) atomicOr(&buf[w], (uint32_t)acc);
    }
};

struct EmitSink {
    const uint32_t *lit, *mtab;
    uint32_t dist;
    BitWriter bw;
    __device__ __forceinline__ void literal(unsigned b) { bw.put(lit[b] & 0xffffu, (int)(lit[b] >> 16)); }
    __device__ __forceinline__ void match(int len) {
        const uint32_t e = mtab[len - kMinMatch];                 // bits << 24 | the length code and its extra bits
        bw.put(e & 0xffffffu, (int)(e >> 24));
        bw.put(dist & 0xffffu, (int)(dist >> 16));
    }
};

__device__ __forceinline__ uint32_t crc_mul_dev(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

struct Flush {
    uint8_t *chunk;                                              // the chunk's first byte (its length field)
    int chunk_bytes;                                             // 12 + data
    int base;                                                    // byte of the chunk that word 0 of the buffer stands for; a multiple
                                                                 // of 16 in the address, negative in front of the chunk
    uint32_t crc;                                                // raw CRC (start 0) of the bytes behind the length field so far
};

// The raw CRC of `count` bytes of the buffer from byte `lo` on; the first four bytes behind the length field (the chunk type) are
// complemented, which is what the start value 0xFFFFFFFF does to a message.
__device__ __forceinline__ uint32_t crc_piece(const uint32_t *buf, const uint32_t *tab, int lo, int count, int base) {
    uint32_t c = 0;
    for (int i = 0; i < count; ++i) {
        const int idx = lo + i;
        unsigned byte = (buf[idx >> 2] >> (8 * (idx & 3))) & 255u;
        const int pos = base + idx;                              // byte of the chunk
        if (pos >= 4 && pos < 8) byte ^= 255u;
        if (pos < 4) byte = 0;                                   // in front of the type: nothing, and zeros leave a raw CRC of 0 alone
        c = tab[(c ^ byte) & 255u] ^ (c >> 8);
    }
    return c;
}

// Writes the buffer's first `groups` 16-byte groups to the chunk and folds them into the CRC.  All threads call it.
__device__ __forceinline__ void flush_groups(Flush &fl, const uint32_t *buf, const uint32_t *tab, uint32_t *red, int groups) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t part = 0;
    for (int g = t; g < groups; g += kThreads) {
        const int pos = fl.base + g * 16;
        const uint4 q = *reinterpret_cast<const uint4 *>(buf + g * 4);
        if (pos >= 4 && pos + 16 <= fl.chunk_bytes - 4) {
            *reinterpret_cast<uint4 *>(fl.chunk + pos) = q;
        } else {
            const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (pos + i >= 4 && pos + i < fl.chunk_bytes - 4) fl.chunk[pos + i] = (uint8_t)(wd[i >> 2] >> (8 * (i & 3)));
        }
        part ^= crc_mul_dev(crc_piece(buf, tab, g * 16, 16, fl.base), kCrcPow.pow16[groups - 1 - g]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part ^= __shfl_xor(part, d);
    __syncthreads();
    if (lane == 0) red[wave] = part;
    __syncthreads();
    fl.crc = crc_mul_dev(fl.crc, kCrcPow.pow16[groups]) ^ red[0] ^ red[1] ^ red[2] ^ red[3];
    fl.base += groups * 16;
}

__global__ void __launch_bounds__(kThreads) png_emit_kernel(const uint8_t *__restrict__ filt, const uint32_t *__restrict__ codes,
                                                             const uint32_t *__restrict__ header, const int32_t *__restrict__ meta,
                                                             const uint32_t *__restrict__ frame, const Frame f, uint8_t *out,
                                                             long capacity, const int32_t *__restrict__ out_len) {
    __shared__ __attribute__((aligned(16))) uint32_t buf[kBufWords];
    __shared__ uint32_t tab[256];
    __shared__ uint32_t lit[kCodeWords];
    __shared__ uint32_t mtab[256];
    __shared__ uint16_t eq[kEqWords];
    __shared__ RunScan wave_tot[4];
    __shared__ int wsum[4];
    __shared__ uint32_t red[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, s = blockIdx.x;
    const long b = blockIdx.y;
    if (out_len[b] < 0) return;                                  // too small a capacity: nothing of the slot is written
    const long k = b * f.stripes + s;
    meta += b * f.stripes * 4;
    const bool first = s == 0, last = s == f.stripes - 1;
    const int hdr_bits = meta[s * 4];
    Flush fl;
    fl.chunk = out + b * capacity + meta[s * 4 + 2];
    const int data_bytes = (int)chunk_data_bytes(meta, s, f.stripes);
    fl.chunk_bytes = 12 + data_bytes;
    fl.crc = 0;
    // word 0 of the buffer stands for the 16-byte aligned address at or below the chunk type
    const int front = (int)(reinterpret_cast<uintptr_t>(fl.chunk + 4) & 15u);
    fl.base = 4 - front;
    tab[t] = kCrcTab.e[t];
    for (int i = t; i < kCodeWords; i += kThreads) lit[i] = codes[k * kCodeWords + i];
    for (int i = t; i < kBufWords; i += kThreads) buf[i] = 0u;
    __syncthreads();
    {
        const int len = t + kMinMatch, idx = length_symbol_index(len), nb = kLenExtraDev[idx];
        const uint32_t c = lit[257 + idx];
        const int cl = (int)(c >> 16);
        mtab[t] = ((uint32_t)(cl + nb) << 24) | (c & 0xffffu) | ((uint32_t)(len - kLenBaseDev[idx]) << cl);
    }
    int pend = front * 8;                                        // bits in the buffer
    if (t == 0) {
        BitWriter bw;
        bw.start(buf, pend);
        bw.put(0x54414449u, 32);                                 // "IDAT"
        if (first) bw.put(0x0178u, 16);                          // zlib: deflate, 32 KB window, no dictionary, fastest; 0x7801 = 31 x 991
        bw.finish();
    }
    pend += first ? 48 : 32;
    for (int i = t; i < kHeaderWords && i * 32 < hdr_bits; i += kThreads) {
        BitWriter bw;
        bw.start(buf, pend + i * 32);
        bw.put(header[k * kHeaderWords + i], 32);
        bw.finish();
    }
    pend += hdr_bits;
    const uint32_t dist = lit[kNumLit];
    StripeWalk w = stripe_walk(f, filt, b, s);
    for (int pass0 = 0; pass0 < w.n; pass0 += kPass) {
        uint4 bytes;
        unsigned mask;
        int m;
        walk_prepare(w, pass0, eq, wave_tot, &bytes, &mask, &m);
        const int off = pass0 + t * 16;
        const int valid = max(0, min(16, w.n - off));
        CountSink cnt{lit, mtab, (int)(dist >> 16), 0};
        walk_tokens(bytes, mask, valid, m, eq, cnt);
        const int inc = wave_scan_inclusive(cnt.n, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();                                          // also: the header and the carried words are in the buffer
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < wave) before += wsum[q];
            all += wsum[q];
        }
        EmitSink es{lit, mtab, dist, {}};
        es.bw.start(buf, pend + before + inc - cnt.n);
        walk_tokens(bytes, mask, valid, m, eq, es);
        es.bw.finish();
        pend += all;
        const bool final_pass = pass0 + kPass >= w.n;
        if (final_pass) {
            __syncthreads();
            if (t == 0) {                                         // end of block; the empty stored block; the Adler-32
                BitWriter bw;
                bw.start(buf, pend);
                bw.put(lit[256] & 0xffffu, (int)(lit[256] >> 16));
                bw.put(last ? 1u : 0u, 3);
                const int fill = (int)((8 - ((pend + (lit[256] >> 16) + 3) & 7)) & 7);
                bw.put(0u, fill);
                bw.put(0xffff0000u, 32);
                if (last) bw.put(__builtin_bswap32(frame[b * 4]), 32);
                bw.finish();
            }
            pend += (lit[256] >> 16) + 3;
            pend = ((pend + 7) & ~7) + 32 + (last ? 32 : 0);
        }
        __syncthreads();
        const int nbytes = pend >> 3;
        const int groups = min(nbytes >> 4, kBufWords / 4 - 1);    // never more than the buffer holds
        flush_groups(fl, buf, tab, red, groups);
        if (final_pass) {
            const int rest = nbytes & 15;                        // the last piece, shorter than 16 bytes
            if (t == 0) {
                uint32_t crc = fl.crc;
                if (rest) {
                    const int pos = fl.base;
                    for (int i = 0; i < rest; ++i) {
                        const int idx = groups * 16 + i;
                        if (pos + i >= 4 && pos + i < fl.chunk_bytes - 4) fl.chunk[pos + i] = (uint8_t)(buf[idx >> 2] >> (8 * (idx & 3)));
                    }
                    crc = crc_mul_dev(crc, kCrcPow.pow1[rest]) ^ crc_piece(buf, tab, groups * 16, rest, fl.base);
                }
                crc ^= 0xFFFFFFFFu;
                // the stream ended where the sizes said it would; a CRC of zero marks a stream that did not
                if (fl.base + rest != fl.chunk_bytes - 4) crc = 0u;
                for (int i = 0; i < 4; ++i) {
                    fl.chunk[i] = (uint8_t)((unsigned)data_bytes >> (24 - 8 * i));
                    fl.chunk[fl.chunk_bytes - 4 + i] = (uint8_t)(crc >> (24 - 8 * i));
                }
            }
        } else {
            // carry what is left (less than 16 bytes and the bits of a byte) to the front of the buffer
            uint32_t keep = 0;
            if (t < 4) keep = buf[groups * 4 + t];
            __syncthreads();
            const int used_words = min(kBufWords, ((pend + 31) >> 5) + 1);
            for (int i = t; i < used_words; i += kThreads) buf[i] = 0u;
            __syncthreads();
            if (t < 4) buf[t] = keep;
            pend -= groups * 128;
        }
    }
}

bool aligned256(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

Frame make_frame(int B, int H, int W, int form, int stripe_rows, const Workspace &ws) {
    const Geometry g = geometry(H, W, form, stripe_rows);
    Frame f;
    f.B = B; f.H = H; f.W = W; f.form = form; f.bpp = g.bpp; f.stripe_rows = stripe_rows; f.stripes = g.stripes;
    f.row = (long)g.row; f.stripe_stride = (long)ws.stripe_stride;
    return f;
}

int launch_filter(const void *src, const Planes &pl, const Frame &f, uint8_t *filt, uint32_t *rowsum, long frame_stride,
                  hipStream_t s) {
    const dim3 grid(cdiv(f.H, 4), f.B);
    if (f.form == kRgb8F32) png_filter_kernel<kRgb8F32><<<grid, kThreads, 0, s>>>(src, pl, filt, rowsum, f, frame_stride);
    else if (f.form == kRgb8U8) png_filter_kernel<kRgb8U8><<<grid, kThreads, 0, s>>>(src, pl, filt, rowsum, f, frame_stride);
    else if (f.form == kGray16F32) png_filter_kernel<kGray16F32><<<grid, kThreads, 0, s>>>(src, pl, filt, rowsum, f, frame_stride);
    else return launch_filter_planes(src, pl, f, filt, rowsum, frame_stride, s);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

struct Parts {
    uint8_t *filt;
    uint32_t *rowsum, *codes, *header, *frame;
    int32_t *hist, *lens, *meta;
};
Parts parts(void *workspace, const Workspace &ws) {
    uint8_t *base = static_cast<uint8_t *>(workspace);
    Parts p;
    p.filt = base + ws.filtered;
    p.rowsum = reinterpret_cast<uint32_t *>(base + ws.rowsum);
    p.hist = reinterpret_cast<int32_t *>(base + ws.hist);
    p.lens = reinterpret_cast<int32_t *>(base + ws.lens);
    p.codes = reinterpret_cast<uint32_t *>(base + ws.codes);
    p.header = reinterpret_cast<uint32_t *>(base + ws.header);
    p.meta = reinterpret_cast<int32_t *>(base + ws.meta);
    p.frame = reinterpret_cast<uint32_t *>(base + ws.frame);
    return p;
}

// launches 1 to 3: filtered bytes, histograms, codes
int launch_front(const void *src, const Planes &pl, const Frame &f, const Workspace &ws, const Parts &p, hipStream_t s) {
    {
        ProfScope prof("png_filter", s, 0.0, 0.0);
        if (int e = launch_filter(src, pl, f, p.filt, p.rowsum, (long)f.stripes * ws.stripe_stride, s)) return e;
    }
    {
        ProfScope prof("png_hist", s, 0.0, 0.0);
        png_hist_kernel<<<dim3(f.stripes, f.B), kThreads, 0, s>>>(p.filt, p.hist, f);
        NUNIF_LAUNCH_CHECK();
    }
    ProfScope prof("png_codes", s, 0.0, 0.0);
    png_codes_kernel<<<dim3(f.stripes, f.B), 64, 0, s>>>(p.hist, p.lens, p.codes, p.header, p.meta, f);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

int check_frame(const char *who, const void *src, int B, int H, int W, int form, int stripe_rows) {
    NUNIF_REQUIRE(src, "%s: NULL frame", who);
    NUNIF_REQUIRE(valid_frame(B, H, W, form, stripe_rows),
                  "%s: B=%d H=%d W=%d form=%d stripe_rows=%d is outside 1 <= B <= %d, 1 <= H, W <= %d, form 0 | 1 | 2 | 4 | 5 | 6, "
                  "1 <= stripe_rows <= H", who, B, H, W, form, stripe_rows, kMaxBatch, kMaxDim);
    return NUNIF_HIP_OK;
}

// the entries that take one source pointer: forms 0..2
int check_single(const char *who, const void *src, int B, int H, int W, int form, int stripe_rows) {
    if (int e = check_frame(who, src, B, H, W, form, stripe_rows)) return e;
    NUNIF_REQUIRE(!planes_form(form), "%s: form %d takes its colour and alpha planes through %s_planes", who, form, who);
    return NUNIF_HIP_OK;
}

// the entries that take the colour planes and the alpha plane apart: forms 4..6
int check_planes(const char *who, const float *colour, const float *alpha, int channels, int B, int H, int W, int form,
                 int stripe_rows, Planes *pl) {
    if (int e = check_frame(who, colour, B, H, W, form, stripe_rows)) return e;
    NUNIF_REQUIRE(planes_form(form), "%s: form %d is not one of 4 (RGBA 8), 5 (grey 8), 6 (grey + alpha 8)", who, form);
    NUNIF_REQUIRE(form == kRgba8F32 ? channels == 3 : (channels == 1 || channels == 3),
                  "%s: form %d with %d colour planes (RGBA takes 3, the grey forms 1 or 3)", who, form, channels);
    NUNIF_REQUIRE(has_alpha(form) ? alpha != nullptr : alpha == nullptr, "%s: form %d %s", who, form,
                  has_alpha(form) ? "needs an alpha plane" : "has no alpha: pass NULL");
    pl->alpha = alpha;
    pl->channels = channels;
    pl->colour_stride = (long)channels * H * W;
    pl->alpha_stride = (long)H * W;
    return NUNIF_HIP_OK;
}

const Planes kNoPlanes = {nullptr, 0, 0, 0};

// One tensor [B][channels + 1][H][W] that holds the colour planes (3 for RGBA, 1 for the grey forms) and then the alpha plane:
// how debug_codes, which has one source pointer, receives forms 4..6
Planes packed_planes(const void *src, int form, int H, int W) {
    if (!planes_form(form)) return kNoPlanes;
    Planes pl;
    pl.channels = form == kRgba8F32 ? 3 : 1;
    const long planes = pl.channels + (has_alpha(form) ? 1 : 0);
    pl.colour_stride = pl.alpha_stride = planes * H * W;
    pl.alpha = has_alpha(form) ? static_cast<const float *>(src) + (long)pl.channels * H * W : nullptr;
    return pl;
}

int encode_frames(const char *who, const void *src, const Planes &pl, int form, int B, int H, int W, int stripe_rows, uint8_t *out,
                  int64_t capacity, int32_t *out_len, void *workspace, void *stream) {
    NUNIF_REQUIRE(out && out_len && capacity >= 0, "%s: NULL output or negative capacity", who);
    NUNIF_REQUIRE(workspace && aligned256(workspace), "%s: the workspace must be 256-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const png::Workspace ws = png::workspace(B, H, W, form, stripe_rows);
    const Frame f = make_frame(B, H, W, form, stripe_rows, ws);
    const Parts p = parts(workspace, ws);
    if (int e = launch_front(src, pl, f, ws, p, s)) return e;
    {
        ProfScope prof("png_scan", s, 0.0, 0.0);
        png_scan_kernel<<<B, kThreads, 0, s>>>(p.meta, p.rowsum, p.frame, f, out, (long)capacity, out_len);
        NUNIF_LAUNCH_CHECK();
    }
    ProfScope prof("png_emit", s, 0.0, 0.0);
    png_emit_kernel<<<dim3(f.stripes, B), kThreads, 0, s>>>(p.filt, p.codes, p.header, p.meta, p.frame, f, out, (long)capacity,
                                                           out_len);
    NUNIF_LAUNCH_CHECK();
    return NUNIF_HIP_OK;
}

int filtered_frames(const void *src, const Planes &pl, int form, int B, int H, int W, uint8_t *filtered, void *stream) {
    // one stripe of H rows and no padding: the rows of a frame, and the frames, lie one behind the other
    png::Workspace ws = png::workspace(B, H, W, form, H);
    ws.stripe_stride = png::geometry(H, W, form, H).stripe_bytes;
    const Frame f = make_frame(B, H, W, form, H, ws);
    return launch_filter(src, pl, f, filtered, nullptr, (long)ws.stripe_stride, (hipStream_t)stream);
}

}  // namespace
}  // namespace nunif

using namespace nunif;

extern "C" int64_t nunif_hip_png_header(int32_t H, int32_t W, int32_t form, const char *const *text_keys,
                                        const char *const *text_values, int32_t n_text, uint8_t *out, int64_t capacity) {
    const int64_t n = png::header(H, W, form, text_keys, text_values, n_text, out, capacity);
    NUNIF_REQUIRE(n != -1, "png_header: H=%d W=%d form=%d with %d text entries is refused (keywords hold 1..79 bytes)", H, W, form,
                  n_text);
    NUNIF_REQUIRE(n != -2, "png_header: the header does not fit into %lld bytes", (long long)capacity);
    return n;
}

extern "C" int64_t nunif_hip_png_max_bytes(int32_t H, int32_t W, int32_t form, int32_t stripe_rows) {
    return png::max_bytes(H, W, form, stripe_rows);
}

extern "C" int64_t nunif_hip_png_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t form, int32_t stripe_rows) {
    return png::workspace_bytes(B, H, W, form, stripe_rows);
}

extern "C" int nunif_hip_png_encode(const void *src, int32_t form, int32_t B, int32_t H, int32_t W, int32_t stripe_rows, uint8_t *out,
                                    int64_t capacity, int32_t *out_len, void *workspace, void *stream) {
    if (int e = check_single("png_encode", src, B, H, W, form, stripe_rows)) return e;
    return encode_frames("png_encode", src, kNoPlanes, form, B, H, W, stripe_rows, out, capacity, out_len, workspace, stream);
}

extern "C" int nunif_hip_png_encode_planes(const float *colour, const float *alpha, int32_t colour_channels, int32_t form, int32_t B,
                                           int32_t H, int32_t W, int32_t stripe_rows, uint8_t *out, int64_t capacity,
                                           int32_t *out_len, void *workspace, void *stream) {
    Planes pl;
    if (int e = check_planes("png_encode_planes", colour, alpha, colour_channels, B, H, W, form, stripe_rows, &pl)) return e;
    return encode_frames("png_encode_planes", colour, pl, form, B, H, W, stripe_rows, out, capacity, out_len, workspace, stream);
}

extern "C" int nunif_hip_png_debug_filtered(const void *src, int32_t form, int32_t B, int32_t H, int32_t W, uint8_t *filtered,
                                            void *stream) {
    if (int e = check_single("png_debug_filtered", src, B, H, W, form, 1)) return e;
    NUNIF_REQUIRE(filtered, "png_debug_filtered: NULL output");
    return filtered_frames(src, kNoPlanes, form, B, H, W, filtered, stream);
}

extern "C" int nunif_hip_png_debug_filtered_planes(const float *colour, const float *alpha, int32_t colour_channels, int32_t form,
                                                   int32_t B, int32_t H, int32_t W, uint8_t *filtered, void *stream) {
    Planes pl;
    if (int e = check_planes("png_debug_filtered_planes", colour, alpha, colour_channels, B, H, W, form, 1, &pl)) return e;
    NUNIF_REQUIRE(filtered, "png_debug_filtered_planes: NULL output");
    return filtered_frames(colour, pl, form, B, H, W, filtered, stream);
}

extern "C" int nunif_hip_png_debug_codes(const void *src, int32_t form, int32_t B, int32_t H, int32_t W, int32_t stripe_rows,
                                         int32_t *hist, int32_t *lengths, void *workspace, void *stream) {
    if (int e = check_frame("png_debug_codes", src, B, H, W, form, stripe_rows)) return e;
    NUNIF_REQUIRE(hist && lengths, "png_debug_codes: NULL output");
    NUNIF_REQUIRE(workspace && aligned256(workspace), "png_debug_codes: the workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const png::Workspace ws = png::workspace(B, H, W, form, stripe_rows);
    const Frame f = make_frame(B, H, W, form, stripe_rows, ws);
    const Parts p = parts(workspace, ws);
    if (int e = launch_front(src, packed_planes(src, form, H, W), f, ws, p, s)) return e;
    const size_t bytes = (size_t)B * f.stripes * png::kSymbolStride * 4;
    NUNIF_HIP_CHECK(hipMemcpyAsync(hist, p.hist, bytes, hipMemcpyDeviceToDevice, s));
    NUNIF_HIP_CHECK(hipMemcpyAsync(lengths, p.lens, bytes, hipMemcpyDeviceToDevice, s));
    return NUNIF_HIP_OK;
}
