// TEST-ONLY host instantiation of the No-U-turn sampler's item functions (hmcmt_items.h: item_nuts_*), driven the way host_chain.h and
// kernels_nuts.h drive them: k_nuts_leaf's CHAIN_NB workgroups of CHAIN_NT threads walk the cells grid-stride, NUTS_GROUP due
// checkpoints per pass; the lanes of a wave add up in wave_sum's tree (kernels_cocg.h), written out here for the host as in
// emul_mass_lowrank.cpp; the four waves as item_mass_lr_block; k_nuts_final adds the workgroups in index order.  The scalar state
// machine (item_nuts_leaf, item_nuts_merge) runs on a Gaussian target with a plain C++ leapfrog.  NOT part of the product.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

namespace {

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

template <int NCK, bool FIRST>
void pass(const NutsLeaf& L) {
    constexpr int WAVES = CHAIN_NT / 64, Q0 = FIRST ? 0 : 3, Q1 = 3 + 2 * NCK;
    std::vector<double> lanes((size_t)NUTS_NACC * CHAIN_NT);
    for (int b = 0; b < CHAIN_NB; ++b) {
        for (int t = 0; t < CHAIN_NT; ++t) {
            double acc[NUTS_NACC] = {};
            for (int64_t a = (int64_t)b * CHAIN_NT + t; a < L.n; a += (int64_t)CHAIN_NT * CHAIN_NB) item_nuts_cell<NCK, FIRST>(L, (int)a, acc);
            for (int q = 0; q < NUTS_NACC; ++q) lanes[(size_t)q * CHAIN_NT + t] = acc[q];
        }
        for (int q = Q0; q < Q1; ++q) {
            double sh[WAVES];
            for (int w = 0; w < WAVES; ++w) sh[w] = wave_sum_host(&lanes[(size_t)q * CHAIN_NT + 64 * w]);
            L.part[item_nuts_row(L, q) * CHAIN_NB + b] = item_mass_lr_block(sh[0], sh[1], sh[2], sh[3]);
        }
    }
}

// nuts_leaf_launch of host_chain.h and k_nuts_final: sums[NUTS_NQ], rows that are not due 0
void leaf_sums(NutsLeaf L, int ndue, const double* const (*due)[3], double* sums) {
    std::vector<double> part((size_t)NUTS_NQ * CHAIN_NB, 0.0);
    L.part = part.data();
    for (int c0 = 0; c0 == 0 || c0 < ndue; c0 += NUTS_GROUP) {
        const int nc = ndue - c0 < 0 ? 0 : (ndue - c0 < NUTS_GROUP ? ndue - c0 : NUTS_GROUP);
        L.ndue = nc;
        L.q0 = c0;
        for (int c = 0; c < NUTS_GROUP; ++c) {
            L.dueP[c] = c < nc ? due[c0 + c][0] : nullptr;
            L.dueX[c] = c < nc ? due[c0 + c][1] : nullptr;
            L.dueR[c] = c < nc ? due[c0 + c][2] : nullptr;
        }
        switch (nc + (c0 == 0 ? 0 : 8)) {
            case 0: pass<0, true>(L); break;
            case 1: pass<1, true>(L); break;
            case 2: pass<2, true>(L); break;
            case 3: pass<3, true>(L); break;
            case 4: pass<4, true>(L); break;
            case 9: pass<1, false>(L); break;
            case 10: pass<2, false>(L); break;
            case 11: pass<3, false>(L); break;
            case 12: pass<4, false>(L); break;
        }
    }
    for (int q = 0; q < NUTS_NQ; ++q) sums[q] = q < 3 + 2 * ndue ? item_chain_total(&part[(size_t)q * CHAIN_NB]) : 0.0;
}

}  // namespace

extern "C" {

int emulnuts_nq() { return NUTS_NQ; }
int emulnuts_ck_max() { return NUTS_CK_MAX; }
int emulnuts_group() { return NUTS_GROUP; }
int emulnuts_depth_max() { return NUTS_DEPTH_MAX; }

void emulnuts_rng(uint64_t seed, uint32_t stream, uint64_t t, int32_t kind, uint32_t index, int32_t* forward, double* u) {
    int f = 0;
    item_rng_nuts(seed, stream, t, kind, index, &f, u);
    *forward = f;
}

void emulnuts_checkpoints(int32_t i, int32_t* slot, int32_t* ndue) {
    int s = 0, d = 0;
    item_nuts_checkpoints(i, &s, &d);
    *slot = s; *ndue = d;
}

// One leaf's pass on host vectors, the arguments of hmcmt_debug_nuts_leaf: ck_write[3] (or NULLs), ck_due[ndue][3]
void emulnuts_leaf(int64_t n, int32_t backward, int32_t other_backward, int32_t first, int32_t merged, int32_t ndue, const double* p,
                   const double* x, const double* inv_m, double* rho_s, double* const* ck_write, const double* const* ck_due, const double* rho,
                   double* rho_next, const double* p_other, const double* x_other, double* sums) {
    NutsLeaf L{};
    L.n = (int)n; L.first = first; L.merged = merged;
    L.sign = backward ? -1.0 : 1.0; L.signOther = other_backward ? -1.0 : 1.0;
    L.p = p; L.x = x; L.invM = inv_m; L.rhoS = rho_s;
    if (ck_write && ck_write[0]) { L.ckP = ck_write[0]; L.ckX = ck_write[1]; L.ckR = ck_write[2]; }
    L.rho = rho; L.rhoNext = rho_next; L.pOther = p_other; L.xOther = x_other;
    const double* due[NUTS_CK_MAX][3] = {};
    for (int c = 0; c < ndue; ++c)
        for (int v = 0; v < 3; ++v) due[c][v] = ck_due[3 * c + v];
    leaf_sums(L, ndue, due, sums);
}

// One sample on the Gaussian target H = 0.5 m'Am + 0.5 p'diag(inv_m)p with the plain leapfrog, orchestrated as chain_nuts_sample
// orchestrates the device: the ends' own (m, p) with the backward momentum stored negated, rhoS, the checkpoints, rho and its successor.
// m [n]: the start, replaced by the selected state; p0 [n]: the momentum.  irec = {depth, nleaves, stop, dirs, selected};
// drec = {alpha, H0, H(selected)}; energies [2^max_depth - 1] of the leaves in the order taken.
void emulnuts_sample(int32_t n, const double* A, const double* inv_m, double dt, int32_t max_depth, uint64_t seed, uint32_t stream, uint64_t t,
                     double* m, const double* p0, int64_t* irec, double* drec, double* energies) {
    auto potential = [&](const double* q) {
        double s = 0;
        for (int a = 0; a < n; ++a) {
            double r = 0;
            for (int b = 0; b < n; ++b) r += A[(size_t)a * n + b] * q[b];
            s += q[a] * r;
        }
        return 0.5 * s;
    };
    auto step = [&](double* q, double* p) {
        std::vector<double> g((size_t)n);
        auto grad = [&]() {
            for (int a = 0; a < n; ++a) {
                double r = 0;
                for (int b = 0; b < n; ++b) r += A[(size_t)a * n + b] * q[b];
                g[a] = r;
            }
        };
        grad();
        for (int a = 0; a < n; ++a) p[a] -= 0.5 * dt * g[a];
        for (int a = 0; a < n; ++a) q[a] += dt * (inv_m[a] * p[a]);
        grad();
        for (int a = 0; a < n; ++a) p[a] -= 0.5 * dt * g[a];
    };
    std::vector<double> mE[2], pE[2], rho[2], rhoS((size_t)n), ck[NUTS_CK_MAX][3], selM[2];
    for (int e = 0; e < 2; ++e) {
        mE[e].assign(m, m + n);
        pE[e].assign(p0, p0 + n);
        rho[e].assign(p0, p0 + n);
        selM[e].assign(m, m + n);
    }
    for (int a = 0; a < n; ++a) pE[0][a] = -p0[a];
    for (auto& c : ck)
        for (auto& v : c) v.assign((size_t)n, 0.0);
    double K0 = 0;
    for (int a = 0; a < n; ++a) K0 += p0[a] * (inv_m[a] * p0[a]);
    K0 *= 0.5;
    NutsTree T;
    item_nuts_begin(T, max_depth, potential(m) + K0);
    int r = 0, selTree = 0;
    double Hsel = T.H0, HselS = 0;
    uint32_t leaf = 0;
    double sums[NUTS_NQ];
    while (true) {
        int forward = 0, dummy = 0;
        double uj = 0, ul = 0;
        item_rng_nuts(seed, stream, t, 0, (uint32_t)T.depth, &forward, &uj);
        item_nuts_doubling(T, forward);
        const int d = forward, nl = 1 << T.depth;
        int status = 0;
        for (int i = 0; i < nl; ++i) {
            step(mE[d].data(), pE[d].data());
            int slot = 0, ndue = 0;
            item_nuts_checkpoints(i, &slot, &ndue);
            NutsLeaf L{};
            L.n = n; L.first = i == 0; L.merged = i == nl - 1;
            L.sign = d ? 1.0 : -1.0; L.signOther = d ? -1.0 : 1.0;
            L.p = pE[d].data(); L.invM = inv_m; L.rhoS = rhoS.data();
            const double* due[NUTS_CK_MAX][3] = {};
            if (i & 1) {
                for (int c = 0; c < ndue; ++c)
                    for (int v = 0; v < 3; ++v) due[c][v] = ck[slot - c][v].data();
            } else {
                L.ckP = ck[slot][0].data(); L.ckX = ck[slot][1].data(); L.ckR = ck[slot][2].data();
                ndue = 0;
            }
            L.rho = rho[r].data(); L.rhoNext = rho[r ^ 1].data();
            L.pOther = pE[d ^ 1].data();
            leaf_sums(L, ndue, due, sums);
            const double H = potential(mE[d].data()) + 0.5 * sums[0];
            energies[leaf] = H;
            item_rng_nuts(seed, stream, t, 1, leaf++, &dummy, &ul);
            bool take = false;
            status = item_nuts_leaf(T, H, ul, sums, &take);
            if (status < 0) break;
            if (take) { selM[selTree ^ 1] = mE[d]; HselS = H; }
        }
        if (status < 0) break;
        bool take = false;
        status = item_nuts_merge(T, uj, sums, &take);
        if (take) { selTree ^= 1; Hsel = HselS; }
        r ^= 1;
        if (status < 0) break;
    }
    if (T.selected != 0) std::memcpy(m, selM[selTree].data(), sizeof(double) * n);
    irec[0] = T.depth; irec[1] = T.nleaves; irec[2] = T.stop; irec[3] = T.dirs; irec[4] = T.selected;
    drec[0] = T.alphaSum / (double)T.nleaves; drec[1] = T.H0; drec[2] = Hsel;
}

}  // extern "C"
