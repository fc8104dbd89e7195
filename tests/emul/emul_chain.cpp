// TEST-ONLY host instantiation of the HMC chain's per-parameter bodies (hmcmt_items.h: item_chain_*), driven the way
// kernels_chain.h drives them: parameter a adds to partial sum chain_part_of(a), the partial sums are added in index order.
// Like emul.cpp it is NOT part of the product: it holds the arithmetic of the momentum draw, the two-stage kinetic energy
// and the Welford update against numpy without a GPU.
#include <cstdint>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

int emulchain_layout(int* nb, int* nt) { *nb = CHAIN_NB; *nt = CHAIN_NT; return 0; }

// p = clip(z) / sqrt(invM); returns K = 0.5 p' invM p (k_chain_momentum + the final stage)
double emulchain_momentum(int64_t n, const double* z, const double* invM, double* p) {
    std::vector<double> part(CHAIN_NB, 0.0);
    for (int a = 0; a < (int)n; ++a) part[chain_part_of(a)] += item_chain_momentum(z, invM, p, a);
    return 0.5 * item_chain_total(part.data());
}

void emulchain_clip(int64_t n, const double* z, double* out) {
    for (int a = 0; a < (int)n; ++a) out[a] = item_chain_clip(z, a);
}

// K = 0.5 p' x (x = M^-1 p given) or 0.5 p' invM p (x == NULL): k_chain_kinetic + the final stage
double emulchain_kinetic(int64_t n, const double* p, const double* x, const double* invM) {
    std::vector<double> part(CHAIN_NB, 0.0);
    for (int a = 0; a < (int)n; ++a) part[chain_part_of(a)] += item_chain_kinetic(p, x, invM, a);
    return 0.5 * item_chain_total(part.data());
}

// the commit of hmcmt_chain_step for nsamples samples (columns of a C-ordered [nsamples][n] array): the first `burnin` stay out
int64_t emulchain_welford(int64_t n, int64_t nsamples, int64_t burnin, const double* samples, double* mean, double* m2) {
    int64_t count = 0;
    for (int a = 0; a < (int)n; ++a) mean[a] = m2[a] = 0.0;
    for (int64_t s = 0; s < nsamples; ++s) {
        if (s < burnin) continue;
        ++count;
        for (int a = 0; a < (int)n; ++a) item_chain_welford(samples + s * n, mean, m2, (double)count, a);
    }
    return count;
}

}  // extern "C"
