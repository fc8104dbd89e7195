// TEST-ONLY host instantiation of the autocovariance bodies of the HMC chain's commit (hmcmt_items.h: item_chain_acov,
// item_chain_acov_out, item_chain_ess), driven the way kernels_chain.h and host_chain.h drive them: one owner per (target, run of
// lags), every array lag-major, the commit's number from the host's count.  Like emul_hist.cpp it is NOT part of the product: it holds
// the streamed sums, the read-out and the initial-positive-sequence rule against numpy without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

int emulacov_maxlag() { return CHAIN_ACOV_MAXLAG; }
int emulacov_run() { return CHAIN_ACOV_RUN; }

// k_chain_acov over nsamples committed models (rows of a C-ordered [nsamples][n] array) into zeroed state arrays; target == NULL:
// every cell.  The runs of lags of one commit are visited upwards at even commits and downwards at odd ones: their order must not matter
void emulacov_accumulate(int64_t n, int64_t nsamples, const double* samples, int64_t ntarget, const int64_t* target, int32_t K,
                         double* x0, double* tot, double* S, double* H, double* ring) {
    const int nrun = K / CHAIN_ACOV_RUN + 1;
    for (int64_t t = 0; t < nsamples; ++t)
        for (int q = 0; q < nrun; ++q) {
            const int r = (t & 1) ? nrun - 1 - q : q;
            const int k0 = r * CHAIN_ACOV_RUN, k1 = std::min(k0 + CHAIN_ACOV_RUN, K + 1);
            for (int64_t j = 0; j < ntarget; ++j)
                item_chain_acov(samples + t * n, (const long long*)target, x0, tot, S, H, ring, ntarget, K, t, j, k0, k1);
        }
}

// k_chain_acov_out: mean[ntarget], acov[K + 1][ntarget]
void emulacov_out(int64_t ntarget, int32_t K, int64_t N, const double* x0, const double* tot, const double* S, const double* H,
                  const double* ring, double* mean, double* acov) {
    for (int64_t j = 0; j < ntarget; ++j) item_chain_acov_out(x0, tot, S, H, ring, ntarget, K, N, j, mean, acov);
}

// k_chain_ess with the cap formed as hmcmt_chain_ess forms it
void emulacov_ess(int64_t ntarget, int32_t K, int64_t N, const double* acov, double* tau, double* ess, int32_t* window) {
    const double lg = std::max(1.0, std::log10((double)N));
    for (int64_t j = 0; j < ntarget; ++j) item_chain_ess(acov, ntarget, K, N, (double)N * lg, 1.0 / lg, j, tau, ess, (int*)window);
}

}  // extern "C"
