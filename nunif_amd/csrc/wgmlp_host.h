// Host half of the fused window-gMLP kernel and of the waifu2x.wgmlp_4x engine (wgmlp.hip): accepted shapes, window counts, the launch
// size, the LDS map, the workspace layout of a forward and the index of a weight inside a packed fragment array.  Integer arithmetic
// only and no HIP: tests/cpp/wgmlp_host_check.cpp builds it with the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace nunif {

constexpr int kWgWindow = 8;                       // WindowGMLP2d window (wgmlp.py:316-326)
constexpr int kWgTokens = kWgWindow * kWgWindow;   // seq_len of GMLP.proj_spatial
constexpr int kWgLdsPad = 8;                       // halfs behind every LDS row: 16 B, so that the rows of a fragment read spread over the banks

inline bool wgmlp_channels_supported(int C) { return C == 128 || C == 256; }
// a shifted block works on the map zero-padded by half a window (attention.py:679-691)
inline int wgmlp_pad(int shift) { return shift ? kWgWindow / 2 : 0; }
inline bool wgmlp_map_supported(int H, int W) { return H > 0 && W > 0 && H % kWgWindow == 0 && W % kWgWindow == 0; }
inline int wgmlp_windows_along(int n, int shift) { return (n + 2 * wgmlp_pad(shift)) / kWgWindow; }
inline long wgmlp_window_count(int B, int H, int W, int shift) {
    return (long)B * wgmlp_windows_along(H, shift) * wgmlp_windows_along(W, shift);
}
// map coordinate of token t (0 .. 7) of window w along one axis; outside [0, n) it is a padded token
inline int wgmlp_token_coord(int w, int t, int shift) { return w * kWgWindow + t - wgmlp_pad(shift); }

// ---- LDS map of wgmlp_block_kernel<C>: region A, then region H ---------------------------------------------------------------------
// A: first the LayerNorm-1 tile [64 tokens][C + 8] (B operand of proj_in), later the LayerNorm-2 tile TRANSPOSED, [C channels][64 + 8]
//    (B operand of the token mixing: its contraction runs over the tokens);  H: [64 tokens][2 C + 8], gelu(proj_in) = u | v, u
//    overwritten by the gate u * v' (B operand of proj_out)
constexpr int wgmlp_lds_a_halfs(int C) {
    return kWgTokens * (C + kWgLdsPad) > C * (kWgTokens + kWgLdsPad) ? kWgTokens * (C + kWgLdsPad) : C * (kWgTokens + kWgLdsPad);
}
constexpr int wgmlp_lds_h_stride(int C) { return 2 * C + kWgLdsPad; }
constexpr int wgmlp_lds_h_halfs(int C) { return kWgTokens * wgmlp_lds_h_stride(C); }
constexpr size_t wgmlp_lds_bytes(int C) { return (size_t)(wgmlp_lds_a_halfs(C) + wgmlp_lds_h_halfs(C)) * 2; }   // 52224 (C = 128), 103424 (C = 256)

// workgroups of a launch: a workgroup walks windows blockIdx.x, blockIdx.x + grid, ...; 256 CUs, and by LDS two workgroups of the
// C = 128 kernel or one of the C = 256 kernel are resident on a CU
inline int wgmlp_max_groups(int C) { return C == 128 ? 512 : 256; }
inline unsigned wgmlp_grid(long windows, int C) {
    const long cap = wgmlp_max_groups(C);
    return (unsigned)(windows < cap ? windows : cap);
}

// position (in halfs) of W[n][k] inside an [n-tile][k-step] fragment array of a Linear with K input columns (host_weights.h put_frag,
// plain k order): fragment (n / 16) * (K / 32) + k / 32, lane ((k % 32) / 8) * 16 + n % 16, slot k % 8
inline size_t wgmlp_packed_index(int n, int k, int K) {
    const size_t frag = (size_t)(n / 16) * (K / 32) + k / 32;
    const int lane = ((k % 32) / 8) * 16 + n % 16;
    return (frag * 64 + lane) * 8 + k % 8;
}

// ---- workspace of one forward at batch B, tile T: byte offsets of its regions, each aligned to 256 -------------------------------
// stem (fp32 NHWC, wgmlp.py:126-173): cat [T,T,32] = stem conv | overscan, x1 [T+12,T+12,16], x2 [T+8,T+8,8], x3 [T+2,T+2,8], fu [T,T,16];
// ir [T,T,32] fp16 (16 channels + zeros: conv_kernel's Cin granule); level-1 maps l1[3] [S,S,C], level-2 maps l2[2] [S/2,S/2,2C],
// tmp_a [S,S,C], tmp_b [S,S,2C] (fp16), rimg [3,4S,4S] fp32.  S = T - 16.
enum WgRegion { WG_CAT = 0, WG_X1, WG_X2, WG_X3, WG_FU, WG_IR, WG_L1A, WG_L1B, WG_L1C, WG_L2A, WG_L2B, WG_TMPA, WG_TMPB, WG_RIMG, WG_REGIONS };
struct WgWorkspace { size_t off[WG_REGIONS], bytes[WG_REGIONS], total; };

inline bool wgmlp_tile_supported(int T) { return T > 16 && (T - 16) % 16 == 0 && (T - 16) % 12 == 0; }   // tile_size_validator :406-409

inline WgWorkspace wgmlp_workspace(int B, int T, int C) {
    WgWorkspace w{};
    const size_t b = (size_t)B, t = (size_t)T, s = (size_t)(T - 16), c = (size_t)C;
    const size_t m1 = b * s * s, m2 = m1 / 4;
    const size_t bytes[WG_REGIONS] = {
        b * t * t * 32 * 4, b * (t + 12) * (t + 12) * 16 * 4, b * (t + 8) * (t + 8) * 8 * 4, b * (t + 2) * (t + 2) * 8 * 4, b * t * t * 16 * 4,
        b * t * t * 32 * 2, m1 * c * 2, m1 * c * 2, m1 * c * 2, m2 * 2 * c * 2, m2 * 2 * c * 2, m1 * c * 2, m1 * 2 * c * 2,
        b * 3 * (4 * s) * (4 * s) * 4};
    size_t at = 0;
    for (int i = 0; i < WG_REGIONS; ++i) {
        w.off[i] = at;
        w.bytes[i] = bytes[i];
        at += (bytes[i] + 255) / 256 * 256;
    }
    w.total = at;
    return w;
}

}  // namespace nunif
