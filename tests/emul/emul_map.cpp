// TEST-ONLY host instantiation of the MAP optimiser's item functions (hmcmt_items.h: item_map_*) and of its coefficient algebra, driven
// the way the kernels of kernels_map.h drive them: LFNB workgroups of 256 threads, grid-stride, MASS_LR_CHUNK rows per pass, the lanes
// of a wave added up in wave_sum's tree (kernels_cocg.h), the four waves as item_mass_lr_block, the workgroups in index order.  The
// coefficient step is the product's own code: item_map_coef runs here exactly as k_map_coef runs it.  NOT part of the product.
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
double block_sum_host(const double* lanes) {     // 256 threads' values -> the workgroup's partial sum
    return item_mass_lr_block(wave_sum_host(lanes), wave_sum_host(lanes + 64), wave_sum_host(lanes + 128), wave_sum_host(lanes + 192));
}
double total_max(const double* part, int k) {
    double v = 0.0;
    for (int b = 0; b < CHAIN_NB; ++b) v = std::fmax(v, part[(size_t)k * CHAIN_NB + b]);
    return v;
}

// the partial sums of the ring's 2 count rows against x(a), as k_map_project and k_map_pair form them
template <class X>
void project_rows(const MapRing& R, X x, double* part) {
    const int nrows = 2 * R.count;
    for (int b = 0; b < CHAIN_NB; ++b)
        for (int q0 = 0; q0 < nrows; q0 += MASS_LR_CHUNK) {
            const int nq = nrows - q0 < MASS_LR_CHUNK ? nrows - q0 : MASS_LR_CHUNK;
            std::vector<double> lanes((size_t)MASS_LR_CHUNK * CHAIN_NT, 0.0);
            for (int t = 0; t < CHAIN_NT; ++t) {
                double acc[MASS_LR_CHUNK];
                for (int q = 0; q < MASS_LR_CHUNK; ++q) acc[q] = 0.0;
                for (long long a = (long long)b * CHAIN_NT + t; a < R.n; a += (long long)CHAIN_NT * CHAIN_NB) item_map_proj_acc(R, q0, nq, x(a), a, acc);
                for (int q = 0; q < MASS_LR_CHUNK; ++q) lanes[(size_t)q * CHAIN_NT + t] = acc[q];
            }
            for (int q = 0; q < nq; ++q) part[(size_t)(q0 + q) * CHAIN_NB + b] = block_sum_host(&lanes[(size_t)q * CHAIN_NT]);
        }
}

}  // namespace

extern "C" {

int emulmap_history_max() { return MAP_HISTORY_MAX; }
int emulmap_part_rows() { return MAP_PART_ROWS; }
int emulmap_coef_len() { return MAP_COEF; }

// k_map_project: pg [n] and part [MAP_PART_ROWS][CHAIN_NB]
void emulmap_project(int64_t n, int32_t H, int32_t head, int32_t count, const double* rows, const double* m, const double* g, double lo, double hi,
                     double* pg, double* part) {
    const MapRing R{rows, n, H, head, count};
    for (size_t i = 0; i < (size_t)MAP_PART_ROWS * CHAIN_NB; ++i) part[i] = 0.0;
    for (int b = 0; b < CHAIN_NB; ++b) {
        double l2[CHAIN_NT], lnb[CHAIN_NT], mx = 0.0;
        for (int t = 0; t < CHAIN_NT; ++t) {
            double s2 = 0.0, nb = 0.0;
            for (long long a = (long long)b * CHAIN_NT + t; a < n; a += (long long)CHAIN_NT * CHAIN_NB) {
                const bool bd = item_map_bound(m[a], g[a], lo, hi);
                const double v = bd ? 0.0 : g[a];
                pg[a] = v;
                s2 = fma(v, v, s2); mx = std::fmax(mx, std::fabs(v)); nb += bd ? 1.0 : 0.0;
            }
            l2[t] = s2; lnb[t] = nb;
        }
        part[(size_t)MAP_P_X0 * CHAIN_NB + b] = block_sum_host(l2);
        part[(size_t)MAP_P_MAX * CHAIN_NB + b] = mx;
        part[(size_t)MAP_P_NB * CHAIN_NB + b] = block_sum_host(lnb);
    }
    project_rows(R, [&](long long a) { return item_map_pg(m, g, lo, hi, a); }, part);
}

// k_map_coef: coef [MAP_COEF], proj [MAP_ROWS_MAX]
void emulmap_coef(int32_t H, int32_t head, int32_t count, const double* sy, const double* yy, const double* part, double* coef, double* proj) {
    const MapRing R{nullptr, 0, H, head, count};
    double t[MAP_ROWS_MAX];
    for (int q = 0; q < MAP_ROWS_MAX; ++q) { t[q] = q < 2 * count ? item_chain_total(part + (size_t)q * CHAIN_NB) : 0.0; proj[q] = t[q]; }
    item_map_coef(R, sy, yy, t, item_chain_total(part + (size_t)MAP_P_X0 * CHAIN_NB), total_max(part, MAP_P_MAX),
                  item_chain_total(part + (size_t)MAP_P_NB * CHAIN_NB), coef);
}

// k_map_expand
void emulmap_expand(int64_t n, int32_t H, int32_t head, int32_t count, const double* rows, const double* coef, const double* pg, const double* m,
                    const double* g, double lo, double hi, double alpha, double* d, double* mt) {
    const MapRing R{rows, n, H, head, count};
    for (long long a = 0; a < n; ++a) {
        d[a] = item_map_dir(R, coef, pg[a], item_map_bound(m[a], g[a], lo, hi), a);
        mt[a] = item_map_clip(m[a], alpha, d[a], lo, hi);
    }
}
// k_map_clip
void emulmap_clip(int64_t n, const double* m, const double* d, double alpha, double lo, double hi, double* mt) {
    for (long long a = 0; a < n; ++a) mt[a] = item_map_clip(m[a], alpha, d[a], lo, hi);
}

// k_map_trial + k_map_trial_final with the trial's full gradient g1 given: out [7] = g0's, s'y, s's, y'y, |pg1|2^2, |pg1|inf, |B1|
// (m0, g0 NULL: no state yet)
void emulmap_trial(int64_t n, const double* m0, const double* g0, const double* m1, const double* g1, double lo, double hi, double* out) {
    std::vector<double> part((size_t)7 * CHAIN_NB, 0.0);
    for (int b = 0; b < CHAIN_NB; ++b) {
        double lanes[6][CHAIN_NT], mx = 0.0;
        for (int t = 0; t < CHAIN_NT; ++t) {
            double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, nb = 0.0;
            for (long long a = (long long)b * CHAIN_NT + t; a < n; a += (long long)CHAIN_NT * CHAIN_NB) {
                bool bd;
                const double v = item_map_trial(m0, g0, m1, g1[a], lo, hi, a, acc, &bd);
                mx = std::fmax(mx, std::fabs(v)); nb += bd ? 1.0 : 0.0;
            }
            for (int q = 0; q < 5; ++q) lanes[q][t] = acc[q];
            lanes[5][t] = nb;
        }
        for (int q = 0; q < 5; ++q) part[(size_t)q * CHAIN_NB + b] = block_sum_host(lanes[q]);
        part[(size_t)5 * CHAIN_NB + b] = mx;
        part[(size_t)6 * CHAIN_NB + b] = block_sum_host(lanes[5]);
    }
    for (int q = 0; q < 5; ++q) out[q] = item_chain_total(&part[(size_t)q * CHAIN_NB]);
    out[5] = total_max(part.data(), 5);
    out[6] = item_chain_total(&part[(size_t)6 * CHAIN_NB]);
}

// k_map_pair + k_map_pair_final: (head, count) the pairs that STAY, slot the new pair's; rows, sy, yy are updated in place
void emulmap_pair(int64_t n, int32_t H, int32_t head, int32_t count, int32_t slot, double* rows, const double* m0, const double* g0,
                  const double* m1, const double* g1, double sTy, double yTy, double* sy, double* yy) {
    const MapRing R{rows, n, H, head, count};
    for (long long a = 0; a < n; ++a) {
        rows[(size_t)slot * n + a] = m1[a] - m0[a];
        rows[(size_t)(H + slot) * n + a] = g1[a] - g0[a];
    }
    std::vector<double> part((size_t)MAP_PART_ROWS * CHAIN_NB, 0.0);
    project_rows(R, [&](long long a) { return g1[a] - g0[a]; }, part.data());
    for (int i = 0; i < count; ++i) {
        const int si = item_map_slot(R, i);
        sy[si * H + slot] = item_chain_total(&part[(size_t)i * CHAIN_NB]);
        const double v = item_chain_total(&part[(size_t)(count + i) * CHAIN_NB]);
        yy[si * H + slot] = v; yy[slot * H + si] = v;
    }
    sy[slot * H + slot] = sTy;
    yy[slot * H + slot] = yTy;
}

}  // extern "C"
