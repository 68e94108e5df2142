// Host side of the cliqa engine (cliqa.hip): which shapes a forward accepts, how a batch is cut into groups, where the maps of a
// group lie in the caller's workspace, and the two index maps by which a conv weight [Cout][Cin][3][3] becomes the MFMA fragment
// stream the kernels read.  Header-only and free of HIP calls, so that tests/cpp/cliqa_host_check.cpp runs every expression of it
// on the CPU under the host sanitizers; cliqa.hip uses nothing else for these.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_weights.h"

namespace nunif {
namespace cliqa_host {

constexpr int kTH = 8, kTW = 16;                 // conv outputs per workgroup (rows, columns)
constexpr long kMaxPixels = 1L << 26;            // H * W of one image
constexpr long kGroupPixels = 1L << 23;          // input pixels of one group (512 patches of 128 x 128): bounds the workspace
constexpr int kMaxGroup = 32768;                 // images per group: blockIdx.y of every launch

inline bool shape_ok(int B, int H, int W) { return B > 0 && H >= 8 && W >= 8 && (long)H * W <= kMaxPixels; }

// Images per pass over the batch.  `group` <= 0: as many as kGroupPixels hold; a request is cut to that too, and to the batch.
// Always in [1, min(B, kMaxGroup)]; one image is a group even where it alone exceeds kGroupPixels.
inline int group_size(int B, int H, int W, int group) {
    long g = std::max<long>(1, kGroupPixels / ((long)H * W));
    if (group > 0) g = std::min<long>(g, group);
    return (int)std::min<long>(std::min<long>(g, B), kMaxGroup);
}

struct Geometry {
    int H, W, H1, W1, H2, W2, H3, W3, tiles3;
    // byte offsets into the workspace of one group of G images: conv 1's map [G][H][W][64] fp16, the maps behind the three pools
    // a1 / a2 / a3 [G][Hi][Wi][128] fp16, the ResBlocks' inner maps t1 / t2 of the size of a1 / a2, the heads' partials
    // [G][heads][tiles3][256] fp32; `size[i]` bytes at `offset(i)`, everything 256-byte aligned
    long a0, a1, t1, a2, t2, a3, part, total;
    long size[7];
    long offset(int i) const { const long o[7] = {a0, a1, t1, a2, t2, a3, part}; return o[i]; }
};

inline long align256(long v) { return (v + 255) / 256 * 256; }

inline Geometry geometry(int heads, int G, int H, int W) {
    Geometry q;
    q.H = H; q.W = W; q.H1 = H / 2; q.W1 = W / 2; q.H2 = q.H1 / 2; q.W2 = q.W1 / 2; q.H3 = q.H2 / 2; q.W3 = q.W2 / 2;
    q.tiles3 = ((q.H3 + kTH - 1) / kTH) * ((q.W3 + kTW - 1) / kTW);
    q.size[0] = (long)G * H * W * 64 * 2;
    q.size[1] = q.size[2] = (long)G * q.H1 * q.W1 * 128 * 2;
    q.size[3] = q.size[4] = (long)G * q.H2 * q.W2 * 128 * 2;
    q.size[5] = (long)G * q.H3 * q.W3 * 128 * 2;
    q.size[6] = (long)G * heads * q.tiles3 * 256 * 4;
    long at = 0;
    long *dst[7] = {&q.a0, &q.a1, &q.t1, &q.a2, &q.t2, &q.a3, &q.part};
    for (int i = 0; i < 7; ++i) { *dst[i] = at; at += align256(q.size[i]); }
    q.total = at;
    return q;
}

// what nunif_hip_cliqa_workspace_bytes answers and forward requires: 0 for a shape forward refuses
inline int64_t workspace_bytes(int heads, int B, int H, int W, int group) {
    if (heads < 1 || heads > 2 || !shape_ok(B, H, W)) return 0;
    return geometry(heads, group_size(B, H, W, group), H, W).total;
}

// ---- weights ---------------------------------------------------------------------------------------------------------------------------
// 3 x 3 conv, k = tap * cin + ci (tap = kh * 3 + kw): element of w [Cout][cin][3][3] that row n, column k of the GEMM reads
inline long conv_weight_index(int n, int k, int cin) { return ((long)n * cin + k % cin) * 9 + k / cin; }

// the [k-step][n-tile] stream of the 128 output channels [n0, n0 + 128) of w [Cout][cin][3][3], cin a multiple of 32, followed by
// kRingPadHalfs zero halfs: tile_conv requests the chunk behind the last k-step
inline std::vector<f16> conv_stream(const float *w, int cin, int n0) {
    return pack_ks_nt(128, 128, 9 * cin, [&](int n, int k) { return w[conv_weight_index(n0 + n, k, cin)]; });
}

// the first conv: K = 96 = 12 tap slots x 8 channel slots, k = tap * 8 + c; taps 9 .. 11 and channels cin .. 7 are zero.
// -1: no element (the weight is zero)
constexpr int kEntryK = 96;
inline long entry_weight_index(int n, int k, int cin) {
    const int tap = k / 8, c = k % 8;
    return (tap < 9 && c < cin) ? ((long)n * cin + c) * 9 + tap : -1;
}

// w [64][cin][3][3], cin <= 8 -> 3 k-steps x 4 n-tiles of fragments (+ the ring padding, unused by the entry kernel)
inline std::vector<f16> entry_stream(const float *w, int cin) {
    return pack_ks_nt(64, 64, kEntryK, [&](int n, int k) {
        const long i = entry_weight_index(n, k, cin);
        return i >= 0 ? w[i] : 0.0f;
    });
}

}  // namespace cliqa_host
}  // namespace nunif
