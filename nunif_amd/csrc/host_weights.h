// Host side of weight loading, shared by every engine that takes a state_dict: the name -> tensor map, device allocations
// owned by a handle, and THE definition of the MFMA A-fragment layout the kernels read their weights in.
//
// Header-only on purpose: the engine files are compiled with different floating-point flags.  Nothing here does arithmetic;
// it converts float -> f16, copies and indexes.  An engine's own arithmetic (scale folds, LayerNorm folds, bias tables) lives
// in the functor it passes in, i.e. in its own translation unit.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace nunif {

struct HostTensor { const float *data; std::vector<int64_t> shape; int64_t numel; };
typedef std::map<std::string, HostTensor> TensorMap;

inline TensorMap tensor_map(const nunif_tensor_desc *tensors, int n) {
    TensorMap m;
    for (int i = 0; i < n; ++i) {
        HostTensor t;
        t.data = tensors[i].data;
        t.numel = 1;
        for (int d = 0; d < tensors[i].ndim; ++d) {
            t.shape.push_back(tensors[i].shape[d]);
            t.numel *= tensors[i].shape[d];
        }
        m[tensors[i].name] = t;
    }
    return m;
}

inline int find(const TensorMap &m, const std::string &key, const HostTensor **out) {
    auto it = m.find(key);
    if (it == m.end()) {
        set_error("state_dict is missing '%s'", key.c_str());
        return NUNIF_HIP_EMISSING;
    }
    *out = &it->second;
    return NUNIF_HIP_OK;
}

// a device buffer that only grows (workspaces sized by the largest call seen)
struct DeviceBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return NUNIF_HIP_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            set_error("hipMalloc(%zu) failed", bytes);
            return NUNIF_HIP_ENOMEM;
        }
        cap = bytes;
        return NUNIF_HIP_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// every device allocation a handle makes at create time; free_all() in its destroy
struct DeviceOwner {
    std::vector<void *> owned;
    int alloc(size_t bytes, void **dev) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            set_error("hipMalloc(%zu) failed", bytes);
            return NUNIF_HIP_ENOMEM;
        }
        owned.push_back(p);
        *dev = p;
        return NUNIF_HIP_OK;
    }
    template <typename T>
    int upload(const std::vector<T> &host, T **dev) {
        void *p = nullptr;
        int rc = alloc(host.size() * sizeof(T), &p);
        if (rc) return rc;
        NUNIF_HIP_CHECK(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
        *dev = reinterpret_cast<T *>(p);
        return NUNIF_HIP_OK;
    }
    int upload_f32(const HostTensor *t, float **dev) { return upload(std::vector<float>(t->data, t->data + t->numel), dev); }
    void free_all() { for (void *p : owned) (void)hipFree(p); owned.clear(); }
};

// The LDS-ring kernels prefetch one 8-KiB chunk (16 fragments) ahead of the fragment they consume and do not test for the end
// of the stream: every weight array they may read carries this many zero halfs (16 KiB) behind its last fragment.
constexpr size_t kRingPadHalfs = 8192;
constexpr size_t kFragHalfs = 512;           // one fragment: 64 lanes x 8 halfs = 1 KiB

// The MFMA A operand (v_mfma_f32_16x16x32_f16) of output tile nt and k-step ks is one fragment of 64 lanes x 8 halfs:
//   lane l, slot j holds W[nt*16 + (l & 15)][ks*32 + (l >> 4)*8 + j].
// `chained` is for a GEMM whose B operand is not loaded from memory but taken straight from the fp32 accumulators of the GEMM
// before it: a lane of a 16x16 accumulator tile holds channels 4*(l >> 4) + 0..3, so the 8 k-slots of lane group g = l >> 4 are
// the channels {32ks + 4g + 0..3} (tile 2ks) and {32ks + 16 + 4g + 0..3} (tile 2ks + 1).  The reduction order over k is free, so
// the permutation costs nothing at run time.
// Writes fragment number `frag` of dst; wt(n, k) is consulted for all 16 rows and 32 columns.
template <typename F>
void put_frag(std::vector<f16> &dst, size_t frag, int nt, int ks, bool chained, F wt) {
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
            const int g = l >> 4;
            const int k = ks * 32 + (chained ? (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4)) : g * 8 + j);
            dst[(frag * 64 + l) * 8 + j] = (f16)wt(nt * 16 + (l & 15), k);
        }
}

// W[n][k] (n < n_real, k < K; rows up to the padded N are zero, wt is not asked for them) as fragments in [n-tile][k-step]
// order (gemm_kernel), followed by `pad` zero halfs
template <typename F>
std::vector<f16> pack_nt_ks(int n_real, int N, int K, F wt, bool chained = false, size_t pad = kRingPadHalfs) {
    const int NT = N / 16, KS = K / 32;
    std::vector<f16> packed((size_t)NT * KS * kFragHalfs + pad, (f16)0.0f);
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks)
            put_frag(packed, (size_t)nt * KS + ks, nt, ks, chained, [&](int n, int k) { return n < n_real ? wt(n, k) : 0.0f; });
    return packed;
}

// the same in [k-step][n-tile] order: the stream conv_kernel and the LDS-staged convs walk
template <typename F>
std::vector<f16> pack_ks_nt(int n_real, int N, int K, F wt, bool chained = false, size_t pad = kRingPadHalfs) {
    const int NT = N / 16, KS = K / 32;
    std::vector<f16> packed((size_t)NT * KS * kFragHalfs + pad, (f16)0.0f);
    for (int ks = 0; ks < KS; ++ks)
        for (int nt = 0; nt < NT; ++nt)
            put_frag(packed, (size_t)ks * NT + nt, nt, ks, chained, [&](int n, int k) { return n < n_real ? wt(n, k) : 0.0f; });
    return packed;
}

// appends fragment `frag` of src to dst at fragment position *at, and advances *at (streams in a kernel's consumption order)
inline void copy_frag(const std::vector<f16> &src, size_t frag, std::vector<f16> &dst, size_t *at) {
    std::copy(src.begin() + frag * kFragHalfs, src.begin() + (frag + 1) * kFragHalfs, dst.begin() + *at * kFragHalfs);
    ++*at;
}

// output tiles [nt0, nt0 + nts) of a [k-step][n-tile] stream, as a stream of their own
inline std::vector<f16> stream_slice(const std::vector<f16> &stream, int KS, int NT, int nt0, int nts,
                                     size_t pad = kRingPadHalfs) {
    std::vector<f16> part((size_t)KS * nts * kFragHalfs + pad, (f16)0.0f);
    size_t at = 0;
    for (int ks = 0; ks < KS; ++ks)
        for (int nt = 0; nt < nts; ++nt) copy_frag(stream, (size_t)ks * NT + nt0 + nt, part, &at);
    return part;
}

// a [k-step][n-tile] stream re-ordered to [n-tile][k-step]
inline std::vector<f16> ks_nt_to_nt_ks(const std::vector<f16> &stream, int KS, int NT, size_t pad = kRingPadHalfs) {
    std::vector<f16> packed((size_t)NT * KS * kFragHalfs + pad, (f16)0.0f);
    size_t at = 0;
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks) copy_frag(stream, (size_t)ks * NT + nt, packed, &at);
    return packed;
}

}  // namespace nunif
