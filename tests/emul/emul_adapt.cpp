// TEST-ONLY host instantiation of the warm-up adaptation's item functions (hmcmt_items.h: item_adapt_*), driven the way
// host_chain.h's chain_adapt_step drives them.  Like emul_chain.cpp it is NOT part of the product: it holds the dual averaging, the
// window schedule and the mass of a window against tests/adapt_ref.py without a GPU.
#include <cstdint>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

// n updates from a restart at dt0 with the acceptances alpha[n]: x[n], x_bar[n] and the clipped dt[n] behind each
void emuladapt_da(int64_t n, const double* alpha, double dt0, double delta, double gamma, double t0, double kappa, double dt_min,
                  double dt_max, double* x, double* x_bar, double* dt) {
    AdaptDA d;
    item_adapt_restart(d, dt0);
    for (int64_t i = 0; i < n; ++i) {
        x[i] = item_adapt_update(d, alpha[i], delta, gamma, t0, kappa);
        x_bar[i] = d.x_bar;
        dt[i] = item_adapt_dt(x[i], dt_min, dt_max);
    }
}

// the window ends of a warm-up as 0-based steps; returns how many there are (at most cap are written)
int64_t emuladapt_windows(int64_t W, int64_t init, int64_t term, int64_t base, int64_t* ends, int64_t cap) {
    long long size = base, end = init + base - 1;
    int64_t k = 0;
    while (end >= 0) {
        if (k < cap) ends[k] = end;
        ++k;
        end = item_adapt_next_window(end, &size, W, term);
    }
    return k;
}

// the mass of a window of nsamples samples (rows of a C-ordered [nsamples][n] array): item_chain_welford, then item_adapt_mass
void emuladapt_mass(int64_t n, int64_t nsamples, const double* samples, double* invM) {
    std::vector<double> mean(n, 0.0), m2(n, 0.0);
    for (int64_t s = 0; s < nsamples; ++s)
        for (int a = 0; a < (int)n; ++a) item_chain_welford(samples + s * n, mean.data(), m2.data(), (double)(s + 1), a);
    const double dn = (double)nsamples, w = dn / (dn + 5.0), f = 1e-3 * 5.0 / (dn + 5.0);
    for (int a = 0; a < (int)n; ++a) invM[a] = item_adapt_mass(m2.data(), dn - 1.0, w, f, a);
}

}  // extern "C"
