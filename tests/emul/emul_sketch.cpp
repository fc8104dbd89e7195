// TEST-ONLY host instantiation of the row sketch's bodies (hmcmt_items.h: item_chain_sketch_*), driven the way kernels_chain.h and
// host_chain.h drive them: one owner per cell in the commit, the shrink and the lift, one owner per entry of the Gram matrix walking
// the cells upwards, the host's eigenproblems by the library's own functions.  Like emul_cov.cpp it is NOT part of the product: it
// holds the sketch against numpy without a GPU, and the GPU tests compare the kernels with it bit for bit.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

int emulsk_ell_min() { return CHAIN_SKETCH_ELL_MIN; }
int emulsk_ell_max() { return CHAIN_SKETCH_ELL_MAX; }
int emulsk_ell_default() { return CHAIN_SKETCH_ELL_DEFAULT; }
int emulsk_cols() { return CHAIN_SKETCH_COLS; }
int emulsk_sweeps_max() { return ADAPT_LR_SWEEPS_MAX; }

// k_chain_sketch_commit: commit t of the model m[n] into row brow
void emulsk_commit(int64_t n, int64_t t, int32_t pivotGiven, const double* m, double* x0, double* tot, double* q, double* brow) {
    for (int64_t a = 0; a < n; ++a) item_chain_sketch_commit(m, x0, tot, q, brow, t, pivotGiven, a);
}

// k_chain_sketch_gram: K[nw][nw] of the rows 0 .. nrows - 1 of B and, with extra, that row behind them; the upper triangle is
// computed and mirrored as the kernel's tiles do
void emulsk_gram(int64_t n, int32_t nrows, const double* B, const double* extra, double* K) {
    const int nw = nrows + (extra ? 1 : 0);
    for (int i = 0; i < nw; ++i)
        for (int j = i; j < nw; ++j) {
            const int bi = i / ADAPT_LR_TILE, bj = j / ADAPT_LR_TILE;
            const double v = item_chain_sketch_gram(item_chain_sketch_row(B, extra, n, nrows, i), item_chain_sketch_row(B, extra, n, nrows, j), n);
            K[(int64_t)i * nw + j] = v;
            // (inside a diagonal tile the mirror entry has its own thread: the same products in the same order, j and i exchanged)
            K[(int64_t)j * nw + i] = bi != bj ? v : item_chain_sketch_gram(item_chain_sketch_row(B, extra, n, nrows, j), item_chain_sketch_row(B, extra, n, nrows, i), n);
        }
}

// the host's share of a shrink: T[ell][2 ell] and *delta from K[2 ell][2 ell] (kept); 0: the eigensolver gave up
int32_t emulsk_shrink_T(int32_t ell, const double* K, double* T, double* delta) {
    std::vector<double> k(K, K + (size_t)4 * ell * ell), t;
    if (!item_chain_sketch_shrink_T(ell, k.data(), t, delta)) return 0;
    std::memcpy(T, t.data(), sizeof(double) * t.size());
    return 1;
}

// k_chain_sketch_shrink: B[2 ell][n] <- T B in place, column by column through a copy of the column, rows ell .. 2 ell - 1 zeroed
void emulsk_apply(int64_t n, int32_t ell, const double* T, double* B) {
    const int n2 = 2 * ell;
    std::vector<double> col((size_t)n2);
    for (int64_t a = 0; a < n; ++a) {
        for (int j = 0; j < n2; ++j) col[j] = B[(int64_t)j * n + a];
        for (int i = 0; i < ell; ++i) B[(int64_t)i * n + a] = item_chain_sketch_shrink(T + (int64_t)i * n2, col.data(), 1, n2);
        for (int i = ell; i < n2; ++i) B[(int64_t)i * n + a] = 0.0;
    }
}

// k_chain_sketch_mean
void emulsk_mean(int64_t n, int64_t N, const double* tot, double* brow) {
    const double dN = (double)N, sqN = sqrt(dN);
    for (int64_t a = 0; a < n; ++a) brow[a] = item_chain_sketch_mean(tot[a], dN, sqN);
}

// the host's share of hmcmt_chain_pca: theta[r] and coef[nw][r] from G[nw][nw] (kept); returns r, -1: no result
int32_t emulsk_pca(int32_t nw, const double* G, int32_t rank, double* theta, double* coef) {
    std::vector<double> g(G, G + (size_t)nw * nw), th, cf;
    const int r = item_chain_sketch_pca(nw, g.data(), rank, th, cf);
    if (r > 0) {
        std::memcpy(theta, th.data(), sizeof(double) * r);
        std::memcpy(coef, cf.data(), sizeof(double) * (size_t)nw * r);
    }
    return r;
}

// k_chain_sketch_lift and k_adapt_lr_sign: U[r][n]
void emulsk_lift(int64_t n, int32_t nrows, const double* B, const double* extra, const double* coef, int32_t r, double* U) {
    const int nw = nrows + (extra ? 1 : 0);
    for (int k = 0; k < r; ++k) {
        double* u = U + (int64_t)k * n;
        for (int64_t a = 0; a < n; ++a) u[a] = item_chain_sketch_lift(B, extra, coef, n, nrows, nw, r, k, a);
        double best = -1.0;
        long long at = n;
        for (int64_t a = 0; a < n; ++a)
            if (item_adapt_lr_beats(fabs(u[a]), a, best, at)) { best = fabs(u[a]); at = a; }
        if (at < n && u[at] < 0.0)
            for (int64_t a = 0; a < n; ++a) u[a] = -u[a];
    }
}

}  // extern "C"
