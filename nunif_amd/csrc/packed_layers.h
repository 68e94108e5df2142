// A state_dict Linear or convolution on its way to the fp16 MFMA kernels, shared by the fp16 engines: the packed weight + bias on the
// device (PackedLinear for gemm_kernel and its relatives, PackedConv for conv_kernel), the host packers that make them from a
// functor, the forms that read `key.weight` / `key.bias` from a state_dict, and the builders that fill GemmArgs / GemmOsArgs /
// ConvArgs from a packed layer and a call's geometry.
//
// Header-only, and without arithmetic, for the reason host_weights.h gives: scale folds, LayerNorm folds and the q pre-scale stay
// in the functors the engines pass in.  The fragment layout itself is host_weights.h's (put_frag).
#pragma once
#include "host_weights.h"
#include "swin_kernels.h"

namespace nunif {

// gemm_kernel's operand: fragments in [n-tile][k-step] order, bias padded to N.  n_real: the valid output columns.
struct PackedLinear { f16 *w = nullptr; float *bias = nullptr; int N = 0, n_real = 0, K = 0; };
// conv_kernel's operand: fragments in [k-step][n-tile] order, k = tap * Cin + ci (cmaj = 0) or chunk-major (ConvArgs::cmaj)
struct PackedConv { f16 *stream = nullptr; float *bias = nullptr; int N = 0, n_real = 0, Cin = 0, k = 3, cmaj = 0; };

// the same on the host, before the upload (an engine that re-orders the fragments for a kernel of its own keeps these)
struct LinearHost { std::vector<f16> w; std::vector<float> bias; int N = 0, n_real = 0, K = 0; };
struct ConvHost { std::vector<f16> stream; std::vector<float> bias; int N = 0, n_real = 0, Cin = 0, k = 3, cmaj = 0; };

inline int pad_to(int n, int granule) { return (n + granule - 1) / granule * granule; }

// a bias accessor over an array that may be absent
inline auto bias_at(const float *b) { return [=](int n) { return b ? b[n] : 0.f; }; }

// W[n][k] = wt(n, k) for n < n_real, k < K_real and zero up to N = n_real padded to `granule` (a multiple of 16; an N that is
// already padded stays) and up to K (a multiple of 32); bias(n) for n < n_real, zero beyond.  Neither functor is asked outside
// the real range.
template <typename F, typename G>
LinearHost pack_linear(int n_real, int granule, int K_real, int K, bool chained, F wt, G bias) {
    LinearHost L;
    L.N = pad_to(n_real, granule); L.n_real = n_real; L.K = K;
    L.w = pack_nt_ks(n_real, L.N, K, [&](int n, int k) { return k < K_real ? wt(n, k) : 0.f; }, chained);
    L.bias.assign(L.N, 0.f);
    for (int n = 0; n < n_real; ++n) L.bias[n] = bias(n);
    return L;
}

// k x k conv, W[n][tap][ci] = wt(n, tap, ci) for n < cout, ci < cin_real, zero up to N (as pack_linear's) and up to cin (a
// multiple of 32).  cmaj = 64 / 32: the chunk-major order of conv3_lds_cm_kernel, [chunk of cmaj channels][tap][32-channel part]
// [n-tile], instead of [k-step][n-tile] with k = tap * cin + ci.
template <typename F, typename G>
ConvHost pack_conv(int cout, int granule, int cin_real, int cin, int k, int cmaj, F wt, G bias) {
    ConvHost C;
    C.N = pad_to(cout, granule); C.n_real = cout; C.Cin = cin; C.k = k; C.cmaj = cmaj;
    const int NT = C.N / 16, KS = k * k * cin / 32;
    auto at = [&](int n, int tap, int ci) { return n < cout && ci < cin_real ? wt(n, tap, ci) : 0.f; };
    if (cmaj) {
        C.stream.assign((size_t)KS * NT * kFragHalfs + kRingPadHalfs, (f16)0.f);
        size_t frag = 0;
        for (int q = 0; q < cin / cmaj; ++q)
            for (int tap = 0; tap < k * k; ++tap)
                for (int c = 0; c < cmaj / 32; ++c)
                    for (int nt = 0; nt < NT; ++nt, ++frag)
                        put_frag(C.stream, frag, nt, c, false, [&](int n, int kk) { return at(n, tap, q * cmaj + kk); });
    } else {
        C.stream = pack_ks_nt(cout, C.N, k * k * cin, [&](int n, int kk) { return at(n, kk / cin, kk % cin); });
    }
    C.bias.assign(C.N, 0.f);
    for (int n = 0; n < cout; ++n) C.bias[n] = bias(n);
    return C;
}

inline int upload(DeviceOwner *h, const LinearHost &src, PackedLinear *L) {
    L->N = src.N; L->n_real = src.n_real; L->K = src.K;
    int rc = h->upload(src.w, &L->w);
    return rc ? rc : h->upload(src.bias, &L->bias);
}
inline int upload(DeviceOwner *h, const ConvHost &src, PackedConv *C) {
    C->N = src.N; C->n_real = src.n_real; C->Cin = src.Cin; C->k = src.k; C->cmaj = src.cmaj;
    int rc = h->upload(src.stream, &C->stream);
    return rc ? rc : h->upload(src.bias, &C->bias);
}
template <typename F, typename G>
int make_linear(DeviceOwner *h, int n_real, int granule, int K_real, F wt, G bias, PackedLinear *L, bool chained = false,
                LinearHost *keep = nullptr) {
    LinearHost host = pack_linear(n_real, granule, K_real, pad_to(K_real, 32), chained, wt, bias);
    if (keep) *keep = host;
    return upload(h, host, L);
}

// `key.weight` [rows][Kt] (a Linear, or a 1x1 conv) and, with has_bias, `key.bias` [rows]: columns k0 .. k0 + K (Kt = 0: the
// whole matrix, Kt = K), N padded to `granule`, K to a multiple of 32
inline int linear_from(DeviceOwner *h, const TensorMap &m, const std::string &key, int rows, int K, int granule, PackedLinear *L,
                       bool chained = false, LinearHost *keep = nullptr, int k0 = 0, int Kt = 0, bool has_bias = true) {
    const HostTensor *w, *b = nullptr;
    int rc;
    if (Kt <= 0) Kt = K;
    if ((rc = find(m, key + ".weight", &w)) || (has_bias && (rc = find(m, key + ".bias", &b)))) return rc;
    NUNIF_REQUIRE(w->numel == (int64_t)rows * Kt && (!b || b->numel == rows), "%s: unexpected shape", key.c_str());
    const float *wd = w->data;
    return make_linear(h, rows, granule, K, [=](int n, int k) { return wd[(size_t)n * Kt + k0 + k]; }, bias_at(b ? b->data : nullptr),
                       L, chained, keep);
}

// `key.weight` [cout][cin_real][k][k] and, with has_bias, `key.bias` [cout]; the producer of the input stores its cin_real
// channels padded with zeros to cin
inline int conv_from(DeviceOwner *h, const TensorMap &m, const std::string &key, int cout, int granule, int cin_real, int cin, int k,
                     PackedConv *C, bool has_bias = true, int cmaj = 0, ConvHost *keep = nullptr) {
    const HostTensor *w, *b = nullptr;
    int rc;
    if ((rc = find(m, key + ".weight", &w)) || (has_bias && (rc = find(m, key + ".bias", &b)))) return rc;
    NUNIF_REQUIRE(w->numel == (int64_t)cout * cin_real * k * k && (!b || b->numel == cout), "%s: unexpected shape", key.c_str());
    NUNIF_REQUIRE(cin % 32 == 0, "%s: Cin=%d must be a multiple of 32", key.c_str(), cin);
    const float *wd = w->data;
    ConvHost host = pack_conv(cout, granule, cin_real, cin, k, cmaj,
                              [=](int n, int tap, int ci) { return wd[((size_t)n * cin_real + ci) * k * k + tap]; },
                              bias_at(b ? b->data : nullptr));
    if (keep) *keep = host;
    return upload(h, host, C);
}

// ---- argument builders: a value-initialised struct with the fields named here set; the caller sets the rest (act, slope, res, mode,
// ps, rev, in_scale, ...) --------------------------------------------------------------------------------------------------------
// NHWC map [B,Hi,Wi,Cin] -> [B,Ho,Wo,n_real]: a 1x1 (K = Cin), or the gather of kw-wide taps at `stride` from (oy, ox) (K = taps Cin).
// Sets a, B, Hi, Wi, Cin, Ho, Wo, stride, oy, ox, kw, K, w, bias, N, n_real, out, ldo = n_real, ps = 1.
inline GemmArgs gemm_map_args(const PackedLinear &L, const f16 *a, int B, int Hi, int Wi, int Cin, int Ho, int Wo, void *out,
                              int stride = 1, int kw = 1, int oy = 0, int ox = 0) {
    GemmArgs g{};
    g.a = a; g.B = B; g.Hi = Hi; g.Wi = Wi; g.Cin = Cin; g.Ho = Ho; g.Wo = Wo; g.stride = stride; g.oy = oy; g.ox = ox; g.kw = kw;
    g.K = L.K; g.w = L.w; g.bias = L.bias; g.N = L.N; g.n_real = L.n_real; g.out = out; g.ldo = L.n_real; g.ps = 1;
    return g;
}
// token matrix [rows][K] -> [rows][n_real]: the map form with B = Hi = Ho = 1, Wi = Wo = rows
inline GemmArgs gemm_token_args(const PackedLinear &L, const f16 *a, long rows, void *out) {
    return gemm_map_args(L, a, 1, 1, (int)rows, L.K, 1, (int)rows, out);
}
// the same for the output-stationary Linear: sets a, M, lda = K, K, w, bias, N, out, ldo = N
inline GemmOsArgs gemm_os_args(const PackedLinear &L, const f16 *a, long rows, f16 *out) {
    GemmOsArgs g{};
    g.a = a; g.M = rows; g.lda = L.K; g.K = L.K; g.w = L.w; g.bias = L.bias; g.N = L.N; g.out = out; g.ldo = L.N;
    return g;
}
// k x k conv on [B,Hi,Wi,Cin] at `stride`: valid (zpad = rpad = 0), zero padding zpad or replication padding rpad;
// Ho = (Hi + 2 pad - k) / stride + 1, Wo alike.  Sets a, B, Hi, Wi, Cin, Ho, Wo, stride, kh, kw, wstream, bias, N, n_real, out,
// zpad, rpad, cmaj.
inline ConvArgs conv_args(const PackedConv &C, const f16 *a, int B, int Hi, int Wi, f16 *out, int stride = 1, int zpad = 0, int rpad = 0) {
    ConvArgs c{};
    c.a = a; c.B = B; c.Hi = Hi; c.Wi = Wi; c.Cin = C.Cin; c.stride = stride; c.kh = C.k; c.kw = C.k;
    c.Ho = (Hi + 2 * (zpad + rpad) - C.k) / stride + 1; c.Wo = (Wi + 2 * (zpad + rpad) - C.k) / stride + 1;
    c.wstream = C.stream; c.bias = C.bias; c.N = C.N; c.n_real = C.n_real; c.out = out; c.zpad = zpad; c.rpad = rpad; c.cmaj = C.cmaj;
    return c;
}

// ---- a conv as launches over output-channel slices: each slice is a stream of its own (stream_slice) of `nt` output tiles and
// writes its channels of the NHWC map through ConvArgs::ldo.  WHETHER to slice is the engine's decision. ---------------------------
struct ConvSlice { const f16 *stream = nullptr; int nt = 0; };
// the launch of a slice that starts at output channel n0 of the whole conv `cv`
inline ConvArgs conv_slice_args(const ConvArgs &cv, const ConvSlice &sl, int n0) {
    ConvArgs t = cv;
    t.wstream = sl.stream; t.N = sl.nt * 16; t.n_real = t.N; t.bias = cv.bias + n0;
    t.ldo = cv.ldo > 0 ? cv.ldo : cv.n_real;
    t.out = cv.out + n0;
    if (cv.res) t.res = cv.res + n0;
    if (cv.res2) t.res2 = cv.res2 + n0;
    return t;
}
inline int launch_conv_sliced(const ConvArgs &cv, const std::vector<ConvSlice> &slices, hipStream_t s) {
    int n0 = 0;
    for (const ConvSlice &sl : slices) {
        int rc = launch_conv(conv_slice_args(cv, sl, n0), s);
        if (rc) return rc;
        n0 += sl.nt * 16;
    }
    return NUNIF_HIP_OK;
}
// uploads tiles [nt0, nt0 + nt) of a host conv's stream for each count of `nts`, in order
inline int upload_slices(DeviceOwner *h, const ConvHost &src, const std::vector<int> &nts, std::vector<ConvSlice> *slices) {
    int nt0 = 0;
    for (int nt : nts) {
        f16 *dev = nullptr;
        int rc = h->upload(stream_slice(src.stream, src.k * src.k * src.Cin / 32, src.N / 16, nt0, nt), &dev);
        if (rc) return rc;
        slices->push_back({dev, nt});
        nt0 += nt;
    }
    return NUNIF_HIP_OK;
}

}  // namespace nunif
