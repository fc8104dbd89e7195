// TEST-ONLY host instantiation of the histogram bodies of the HMC chain's commit (hmcmt_items.h: item_chain_hist_bin,
// item_chain_hist, item_chain_quantile), driven the way kernels_chain.h drives them: one owner per target row, the counters
// bin-major.  Like emul_chain.cpp it is NOT part of the product: it holds the bin rule and the quantile scan against numpy
// without a GPU.
#include <cstdint>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

int emulhist_maxbins() { return CHAIN_HIST_MAXBINS; }

// the bin of every value; scale = (double)nbins / (hi - lo) is formed here as the host code of the library forms it
void emulhist_bins(int64_t n, const double* m, int32_t nbins, double lo, double hi, int32_t* out) {
    const double scale = (double)nbins / (hi - lo);
    for (int64_t i = 0; i < n; ++i) out[i] = item_chain_hist_bin(m[i], lo, scale, nbins);
}

// k_chain_hist over nsamples committed models (rows of a C-ordered [nsamples][n] array), then the counters target-major as
// hmcmt_chain_hist returns them
void emulhist_accumulate(int64_t n, int64_t nsamples, const double* samples, int64_t ntarget, const int64_t* target, int32_t nbins,
                         double lo, double hi, uint32_t* counts) {
    const double scale = (double)nbins / (hi - lo);
    std::vector<unsigned int> dev((size_t)ntarget * nbins, 0u);
    for (int64_t s = 0; s < nsamples; ++s)
        for (int64_t r = 0; r < ntarget; ++r)
            item_chain_hist(samples + s * n, (const long long*)target, dev.data(), ntarget, nbins, lo, scale, r);
    for (int64_t r = 0; r < ntarget; ++r)
        for (int b = 0; b < nbins; ++b) counts[r * nbins + b] = dev[(size_t)b * ntarget + r];
}

// k_chain_quantiles on target-major counters: out[nq][ntarget], bins[nq][ntarget]; x = q * (double)count as hmcmt_chain_hist_quantiles
void emulhist_quantiles(int64_t ntarget, int32_t nbins, const uint32_t* counts, int64_t count, double lo, double hi, int32_t nq,
                        const double* q, double* out, int32_t* bins) {
    const double w = (hi - lo) / (double)nbins;
    std::vector<unsigned int> dev((size_t)ntarget * nbins);
    for (int64_t r = 0; r < ntarget; ++r)
        for (int b = 0; b < nbins; ++b) dev[(size_t)b * ntarget + r] = counts[r * nbins + b];
    for (int i = 0; i < nq; ++i) {
        const double x = q[i] * (double)count;
        for (int64_t r = 0; r < ntarget; ++r) {
            int bin;
            out[i * ntarget + r] = item_chain_quantile(dev.data(), ntarget, nbins, lo, w, x, r, &bin);
            bins[i * ntarget + r] = bin;
        }
    }
}

}  // extern "C"
