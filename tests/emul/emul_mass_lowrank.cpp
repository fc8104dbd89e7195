// TEST-ONLY host instantiation of the item functions of the low-rank-plus-diagonal mass (hmcmt_items.h: item_mass_lr_*), driven the way
// k_mass_lr_project and k_mass_lr_expand (kernels_mass.h) drive them: CHAIN_NB workgroups of CHAIN_NT threads walk the cells
// grid-stride, MASS_LR_CHUNK directions per pass; the lanes of a wave add up in wave_sum's tree (kernels_cocg.h), written out here for
// the host.  Like emul_cov.cpp it is NOT part of the product: it holds the arithmetic and its order against numpy without a GPU.
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

namespace {

// wave_sum on the host: pairs, quads, the row of 16 by two rotations (lane 0 of a row: (q0 + q3) + (q2 + q1)), then the four rows
double wave_sum_host(const double* v) {
    double row[4];
    for (int r = 0; r < 4; ++r) {
        double q[4];
        for (int i = 0; i < 4; ++i) {
            const double* p = v + 16 * r + 4 * i;
            q[i] = (p[0] + p[1]) + (p[2] + p[3]);
        }
        row[r] = (q[0] + q[3]) + (q[2] + q[1]);
    }
    return (row[0] + row[1]) + (row[2] + row[3]);
}

}  // namespace

extern "C" {

int emulmlr_rank_max() { return MASS_LR_RANK_MAX; }
int emulmlr_chunk() { return MASS_LR_CHUNK; }
int emulmlr_blocks() { return CHAIN_NB; }

// k_mass_lr_project: part[rank][CHAIN_NB]
void emulmlr_project(int64_t n, int32_t rank, int32_t op, const double* s, const double* U, const double* x, double* part) {
    constexpr int WAVES = CHAIN_NT / 64;
    std::vector<double> lanes((size_t)MASS_LR_CHUNK * CHAIN_NT);
    for (int b = 0; b < CHAIN_NB; ++b) {
        double sh[WAVES][MASS_LR_RANK_MAX] = {};
        for (int k0 = 0; k0 < rank; k0 += MASS_LR_CHUNK) {
            const int nk = rank - k0 < MASS_LR_CHUNK ? rank - k0 : MASS_LR_CHUNK;
            for (int t = 0; t < CHAIN_NT; ++t) {
                double acc[MASS_LR_CHUNK] = {};
                for (int64_t a = (int64_t)b * CHAIN_NT + t; a < n; a += (int64_t)CHAIN_NT * CHAIN_NB)
                    item_mass_lr_acc(U, n, k0, nk, item_mass_lr_pre(s, x, op, a), a, acc);
                for (int q = 0; q < MASS_LR_CHUNK; ++q) lanes[(size_t)q * CHAIN_NT + t] = acc[q];
            }
            for (int q = 0; q < MASS_LR_CHUNK; ++q)
                for (int w = 0; w < WAVES; ++w) sh[w][k0 + q] = wave_sum_host(&lanes[(size_t)q * CHAIN_NT + 64 * w]);
        }
        for (int k = 0; k < rank; ++k) part[(int64_t)k * CHAIN_NB + b] = item_mass_lr_block(sh[0][k], sh[1][k], sh[2][k], sh[3][k]);
    }
}

// k_mass_lr_expand: c[rank] = lambda - 1 (op 0) or lambda^-1/2 - 1 (op 1); y may be x
void emulmlr_expand(int64_t n, int32_t rank, int32_t op, const double* s, const double* U, const double* c, const double* part, const double* x,
                    double* y) {
    double w[MASS_LR_RANK_MAX];
    for (int k = 0; k < rank; ++k) w[k] = item_mass_lr_weight(part, c, k);
    for (int64_t a = 0; a < n; ++a) y[a] = item_mass_lr_expand(s, x, U, w, n, rank, op, a);
}

}  // extern "C"
