// Host half of the reference's WABlock (iw3/models/row_flow_v3.py :14-30, depth_aa.py :11-26: window attention with a learned score
// bias, then conv_mlp = 1x1 + GELU, replicate-pad 3x3, and a residual) and of WindowScoreBias (nunif/modules/attention.py :375-419):
// the score-bias table and the block's packed arrays.  Pure host arithmetic with no HIP call of its own, kept in a header so that a
// stand-alone program can run it under the host sanitizers (tests/cpp/wa_block_host_check.cpp); wa_block.hip has the device half.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_weights.h"

namespace nunif {

inline double gelu_erf_d(double v) { return 0.5 * v * (1.0 + erf(v * 0.70710678118654752440)); }

// WindowScoreBias: the to_bias MLP on the normalised relative offsets of a window x window window, evaluated once in double:
// tab[q * stride + k] = log2(e) * bias[query q][key k].  stride = window * window, or 16 for the kernels that hold a window in one
// MFMA tile: there key columns beyond the window are -1e30 in every row (masked), and the real key columns of the rows beyond it are 0
// (padded queries: any finite row).  `what` names the block in the message.
inline int wa_score_bias_table(const HostTensor *tw0, const HostTensor *tb0, const HostTensor *tw2, const HostTensor *tb2, int window,
                               int stride, const std::string &what, std::vector<float> *tab) {
    const int hidden = (int)tb0->numel, N = window * window;
    NUNIF_REQUIRE(tw0->numel == hidden * 2 && tw2->numel == hidden && tb2->numel == 1, "%s: score-bias MLP shape", what.c_str());
    NUNIF_REQUIRE(window > 1 && stride >= N, "%s: score-bias table of stride %d for a %dx%d window", what.c_str(), stride, window, window);
    const float dmax = (float)(window - 1);
    tab->assign((size_t)stride * stride, -1.0e30f);
    for (int q = 0; q < N; ++q)
        for (int k = 0; k < N; ++k) {
            const float dy = (float)(q / window - k / window) / dmax, dx = (float)(q % window - k % window) / dmax;
            double o = tb2->data[0];
            for (int j = 0; j < hidden; ++j)
                o += (double)tw2->data[j] * gelu_erf_d((double)tw0->data[j * 2] * dy + (double)tw0->data[j * 2 + 1] * dx +
                                                        (double)tb0->data[j]);
            (*tab)[(size_t)q * stride + k] = (float)o * 1.4426950408889634f;
        }
    for (int q = N; q < stride; ++q) for (int k = 0; k < N; ++k) (*tab)[(size_t)q * stride + k] = 0.f;
    return NUNIF_HIP_OK;
}

struct WaBlockHost {
    std::vector<f16> wfrag;              // 3*NT*KS qkv fragments (part, nt, ks) + NT*KS head_proj fragments (nt, ks; chained k order)
    std::vector<float> bqkv, bproj;      // [3C] (q part pre-scaled like its weights), [C]
    std::vector<float> btab;             // wa_score_bias_table
    std::vector<f16> w1, w3;             // conv_mlp[0] 1x1: gemm_kernel packing [nt][ks]; conv_mlp[3] 3x3: conv_kernel stream [ks][nt]
    std::vector<float> b1, b3;
};

// The arrays of the WABlock under prefix `p`: C channels in heads of `hd`, tiled as NT = C/16 output tiles x KS = C/32 k-steps (for
// C = 32 in heads of 16 the qkv fragment (part, nt) is the one of (part, head)).  head_dim^-0.5 * log2(e) is folded into q.
inline int wa_block_pack(const TensorMap &m, const std::string &p, int window, int C, int hd, int btab_stride, WaBlockHost *o) {
    const int NT = C / 16, KS = C / 32;
    const HostTensor *wqkv, *bqkv, *wp, *bp, *w1, *b1, *w3, *b3, *tw0, *tb0, *tw2, *tb2;
    int rc;
    if ((rc = find(m, p + "mha.mha.qkv_proj.weight", &wqkv)) || (rc = find(m, p + "mha.mha.qkv_proj.bias", &bqkv)) ||
        (rc = find(m, p + "mha.mha.head_proj.weight", &wp)) || (rc = find(m, p + "mha.mha.head_proj.bias", &bp)) ||
        (rc = find(m, p + "conv_mlp.0.weight", &w1)) || (rc = find(m, p + "conv_mlp.0.bias", &b1)) ||
        (rc = find(m, p + "conv_mlp.3.weight", &w3)) || (rc = find(m, p + "conv_mlp.3.bias", &b3)) ||
        (rc = find(m, p + "bias.to_bias.0.weight", &tw0)) || (rc = find(m, p + "bias.to_bias.0.bias", &tb0)) ||
        (rc = find(m, p + "bias.to_bias.2.weight", &tw2)) || (rc = find(m, p + "bias.to_bias.2.bias", &tb2)))
        return rc;
    NUNIF_REQUIRE(wqkv->numel == (int64_t)3 * C * C && wp->numel == (int64_t)C * C && w1->numel == (int64_t)C * C &&
                  w3->numel == (int64_t)C * C * 9, "%s: expected %d channels (heads of %d)", p.c_str(), C, hd);
    const float qs = (1.0f / sqrtf((float)hd)) * 1.4426950408889634f;
    o->wfrag.resize((size_t)4 * NT * KS * kFragHalfs);
    const float *wd = wqkv->data, *pd = wp->data;
    for (int part = 0; part < 3; ++part)
        for (int nt = 0; nt < NT; ++nt)
            for (int ks = 0; ks < KS; ++ks)
                put_frag(o->wfrag, (size_t)(part * NT + nt) * KS + ks, nt, ks, false, [=](int n, int k) {
                    return wd[(size_t)(part * C + n) * C + k] * (part == 0 ? qs : 1.0f); });
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks)
            put_frag(o->wfrag, (size_t)3 * NT * KS + nt * KS + ks, nt, ks, true, [=](int n, int k) { return pd[(size_t)n * C + k]; });
    o->bqkv.resize(3 * C);
    for (int n = 0; n < 3 * C; ++n) o->bqkv[n] = bqkv->data[n] * (n < C ? qs : 1.0f);
    o->bproj.assign(bp->data, bp->data + C);
    if ((rc = wa_score_bias_table(tw0, tb0, tw2, tb2, window, btab_stride, p, &o->btab))) return rc;
    const float *d1 = w1->data, *d3 = w3->data;
    o->w1 = pack_nt_ks(C, C, C, [=](int n, int k) { return d1[(size_t)n * C + k]; });
    o->b1.assign(b1->data, b1->data + C);
    o->w3 = pack_ks_nt(C, C, 9 * C, [=](int n, int k) {                  // k = tap*C + ci
        const int tap = k / C, ci = k % C;
        return d3[((size_t)n * C + ci) * 9 + tap]; });
    o->b3.assign(b3->data, b3->data + C);
    return NUNIF_HIP_OK;
}

}  // namespace nunif
