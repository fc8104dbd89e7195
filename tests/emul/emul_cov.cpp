// TEST-ONLY host instantiation of the cross-moment bodies of the HMC chain's commit (hmcmt_items.h: item_chain_cov_commit,
// item_chain_cov_flush, item_chain_cov_out, item_chain_corr), driven the way kernels_chain.h and host_chain.h drive them: one owner
// per cell in the commit, one owner per S[r][a] in the flush with the row panel gathered per row tile, the cell index fastest.  Like
// emul_acov.cpp it is NOT part of the product: it holds the streamed sums and the read-outs against numpy without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

namespace {

// k_chain_cov_flush<NB> over the row tiles in the order `order` (a permutation of the tiles) and, inside a tile, the column tiles
// upwards
template <int NB>
void flush_nb(int64_t n, int64_t nrow, const int64_t* row, const double* pend, double* S, const std::vector<int64_t>& order) {
    double panel[CHAIN_COV_TILE_ROWS * NB], ycol[NB];
    for (int64_t tile : order) {
        const int64_t r0 = tile * CHAIN_COV_TILE_ROWS;
        const int nr = (int)std::min<int64_t>(nrow - r0, CHAIN_COV_TILE_ROWS);
        for (int i = 0; i < nr * NB; ++i) {
            const int r = i / NB, b = i - r * NB;
            panel[i] = pend[(int64_t)b * n + (row ? row[r0 + r] : r0 + r)];
        }
        for (int64_t a = 0; a < n; ++a) {
            for (int b = 0; b < NB; ++b) ycol[b] = pend[(int64_t)b * n + a];
            for (int r = 0; r < nr; ++r) S[(r0 + r) * n + a] = item_chain_cov_flush<NB>(panel + r * NB, ycol, S[(r0 + r) * n + a]);
        }
    }
}

void flush(int nb, int64_t n, int64_t nrow, const int64_t* row, const double* pend, double* S, int64_t visit) {
    const int64_t tiles = (nrow + CHAIN_COV_TILE_ROWS - 1) / CHAIN_COV_TILE_ROWS;
    std::vector<int64_t> order((size_t)tiles);
    for (int64_t i = 0; i < tiles; ++i) order[(size_t)i] = (visit & 1) ? tiles - 1 - i : i;      // (downwards at odd flushes of `reverse`)
    switch (nb) {
#define F(NB) case NB: flush_nb<NB>(n, nrow, row, pend, S, order); break;
        F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)
#undef F
    }
}

}  // namespace

extern "C" {

int emulcov_batch_max() { return CHAIN_COV_BATCH_MAX; }
int emulcov_batch_default() { return CHAIN_COV_BATCH_DEFAULT; }
int emulcov_tile_cols() { return CHAIN_COV_TILE_COLS; }
int emulcov_tile_rows() { return CHAIN_COV_TILE_ROWS; }

// the commits t0 .. t1 - 1 (the rows of the C-ordered array samples[t1 - t0][n]) into the state (x0, tot, q, pend[B][n], S[nrow][n]) whose
// count is t0 and which has *npend commits parked, as hmcmt_chain_step drives them: a flush when B are parked.  row == NULL: every
// cell.  reverse != 0: every other flush visits its row tiles downwards (their order must not matter).  final_flush != 0: what a
// read-out does first
void emulcov_accumulate(int64_t n, int64_t t0, int64_t t1, const double* samples, int64_t nrow, const int64_t* row, int32_t B, double* x0,
                        double* tot, double* q, double* pend, double* S, int32_t* npend, int64_t* nflush, int32_t reverse, int32_t final_flush) {
    for (int64_t t = t0; t < t1; ++t) {
        for (int64_t a = 0; a < n; ++a) item_chain_cov_commit(samples + (t - t0) * n, x0, tot, q, pend, n, t, *npend, a);
        if (++*npend == B) { flush(B, n, nrow, row, pend, S, reverse ? (*nflush)++ : 0); *npend = 0; }
    }
    if (final_flush && *npend) { flush(*npend, n, nrow, row, pend, S, reverse ? (*nflush)++ : 0); *npend = 0; }
}

// k_chain_cov_out: mean[n], var[n], cov[nrow][n] (each may be NULL)
void emulcov_out(int64_t n, int64_t nrow, const int64_t* row, int64_t N, const double* x0, const double* tot, const double* q, const double* S,
                 double* mean, double* var, double* cov) {
    const int64_t rows = cov ? nrow : 1;
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t a = 0; a < n; ++a) item_chain_cov_out(x0, tot, q, S, (const long long*)row, n, (double)N, r, a, mean, var, cov);
}

// k_chain_corr
void emulcov_corr(int64_t n, int64_t nrow, const int64_t* row, int64_t N, const double* tot, const double* q, const double* S, double* corr) {
    for (int64_t r = 0; r < nrow; ++r)
        for (int64_t a = 0; a < n; ++a) item_chain_corr(tot, q, S, (const long long*)row, n, (double)N, r, a, corr);
}

}  // extern "C"
