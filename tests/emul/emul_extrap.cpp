// TEST-ONLY host instantiation of the weights of the initial-guess extrapolation (hmcmt_items.h: extrap_weights), driven the way
// kernels_fused.h drives it: k_extrap_prepare's sums over the ring of models -- here one serial fp64 sum per inner product instead of
// 32 blocks of partial sums and a ticket -- then the one thread that takes the decisions, forms the weights and moves the ring heads.
// Like emul_cov.cpp it is NOT part of the product: it holds those decisions and weights against tests/extrap_ref.py without a GPU.
#include <cstdint>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

int emulext_points() { return EXT_NP; }
int emulext_state_len() { return EXT_PART; }
int emulext_nsums() { return EXT_NS; }

// extrap_weights on the caller's sums a[EXT_NS] and state ext[EXT_PART]; returns keep
int emulext_weights(const double* a, double* ext, int32_t maxNp, int32_t coldUnlessSmooth) {
    return extrap_weights(a, ext, maxNp, coldUnlessSmooth) ? 1 : 0;
}

// one call of k_extrap_prepare for a model of n parameters: hist[(EXT_NP + 1)][n] the ring of models, ext[EXT_PART] the state
// {w_0 .., keep, count, field-ring head, model-ring head}; sums (may be NULL) receives a[EXT_NS].  Returns keep
int emulext_call(int64_t n, const double* mNew, double* hist, double* ext, int32_t maxNp, int32_t coldUnlessSmooth, double* sums) {
    const int hm = (int)ext[EXT_MHEAD];
    double* fresh = hist + (int64_t)((hm + EXT_NP) % (EXT_NP + 1)) * n;
    double a[EXT_NS];
    for (int q = 0; q < EXT_NS; ++q) a[q] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double m[EXT_NP], d[EXT_NP];
        for (int j = 0; j < EXT_NP; ++j) m[j] = hist[(int64_t)((hm + j) % (EXT_NP + 1)) * n + i];
        const double mn = mNew[i];
        fresh[i] = mn;
        d[0] = mn - m[0];
        for (int j = 1; j < EXT_NP; ++j) d[j] = m[j - 1] - m[j];
        for (int j = 0; j < EXT_NP; ++j) a[j] += d[j] * d[1];
        a[EXT_NP] += d[0] * d[0];
        for (int j = 2; j < EXT_NP; ++j) a[EXT_NP + j - 1] += d[j] * d[j];
        a[EXT_NS - 1] += m[0] * m[0];
    }
    if (sums) for (int q = 0; q < EXT_NS; ++q) sums[q] = a[q];
    return extrap_weights(a, ext, maxNp, coldUnlessSmooth) ? 1 : 0;
}

}  // extern "C"
