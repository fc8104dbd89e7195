// kernels_mass.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// The non-diagonal mass matrix M = Wm of the reference (setMassMatrix(invParam), HMCSampler.jl:478-489): sqrtM = L = chol(Wm).L
// in the natural order of the active cells, invM = Wm^-1.
//
// Wm = (GA)'(GA) (invsetup.smoothnessMatrix) is the 5-point operator of the active cells.  When they fill a box of nzb x nyb
// cells (y fastest) below the air, Wm = I_nzb (x) T_y + T_z (x) I_nyb with
//   T_y = ddx'ddx (Neumann both ends):                 lambda_y,k = 2 - 2 cos(pi k / nyb),            DCT-II vectors
//   T_z = ddx'ddx + e0 e0' (the air above the top row): lambda_z,k = 2 - 2 cos(pi (2k+1) / (2 nzb + 1)), sin(theta_k (i+1))
// and Wm^-1 x is a fast diagonalisation: X = x on the box (nzb x nyb, row-major), Y = Q_z [(Q_z' X Q_y) ./ (lz_i + ly_j)] Q_y'
// -- four small dense fp64 GEMMs (k_mass_gemm).  Otherwise (frozen cells inside the box) Wm^-1 x is fp64 PCG on the CSR with
// that box inverse, zero-extended and restricted, as the preconditioner (host loop in hmcmt_hip.hip).
// Plain fp64 FMA, not v_mfma_f64_16x16x4_f64: at cfg3 (100 x 200 box) the four GEMMs take 10-17 us each (rocprofv3 kernel trace),
// the whole M = Wm addition to a leapfrog step -- Wm^-1 p, its step bound, the separate position and momentum updates -- about
// 70 us of a 1.6 ms step; MFMA could win back part of the 50 us of GEMMs at most.
#pragma once

// ---- fp64 GEMM C[M x N] = A[M x K] * B[K x N], all row-major ---------------------------------------------------------------
// MG_SCATTER_B: B is the box image of the active vector bx (B[k][j] = bx[map[k*N+j]], 0 where map < 0)
// MG_DIVIDE:    C[i][j] = (A B)[i][j] / (lz[i] + ly[j])
// MG_GATHER_C:  the box result is restricted: cy[map[i*N+j]] = (A B)[i][j] where map >= 0 (nothing else is written)
constexpr int MG_SCATTER_B = 1, MG_DIVIDE = 2, MG_GATHER_C = 4;
constexpr int MG_T = 32;       // output tile (MG_T x MG_T) per workgroup of 256 threads, 2 x 2 outputs each
constexpr int MG_KT = 32;      // K slab per LDS stage
struct MassGemm {
    int M, N, K;
    const double* A; const double* B; double* C;
    const int* map; const double* bx; double* cy;
    const double *lz, *ly;
};
template <int MODE>
__global__ __launch_bounds__(256) void k_mass_gemm(MassGemm g) {
    __shared__ double As[MG_KT][MG_T + 1];      // As[k][i] = A[i0 + i][k0 + k]
    __shared__ double Bs[MG_KT][MG_T + 1];      // Bs[k][j] = B[k0 + k][j0 + j]
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * MG_T, j0 = blockIdx.x * MG_T;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    double ra[4], rb[4];
    // each thread stages four elements of either tile: element e = threadIdx.x + 256 q of the MG_T x MG_KT slab
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = threadIdx.x + 256 * q;
            const int ai = e / MG_KT, ak = e % MG_KT;            // A: consecutive threads walk k (row-major A)
            const int gi = i0 + ai, gk = k0 + ak;
            ra[q] = (gi < g.M && gk < g.K) ? g.A[(long)gi * g.K + gk] : 0.0;
            const int bk = e / MG_T, bj = e % MG_T;              // B: consecutive threads walk j
            const int hk = k0 + bk, hj = j0 + bj;
            double b = 0.0;
            if (hk < g.K && hj < g.N) {
                const long o = (long)hk * g.N + hj;
                if (MODE & MG_SCATTER_B) { const int a = g.map[o]; b = a >= 0 ? g.bx[a] : 0.0; }
                else b = g.B[o];
            }
            rb[q] = b;
        }
    };
    load(0);
    for (int k0 = 0; k0 < g.K; k0 += MG_KT) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = threadIdx.x + 256 * q;
            As[e % MG_KT][e / MG_KT] = ra[q];
            Bs[e / MG_T][e % MG_T] = rb[q];
        }
        __syncthreads();
        if (k0 + MG_KT < g.K) load(k0 + MG_KT);                 // (the next slab's loads in flight during this slab's FMAs)
#pragma unroll 8
        for (int k = 0; k < MG_KT; ++k) {
            const double a0 = As[k][ty], a1 = As[k][ty + 16], b0 = Bs[k][tx], b1 = Bs[k][tx + 16];
            acc[0][0] = fma(a0, b0, acc[0][0]); acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]); acc[1][1] = fma(a1, b1, acc[1][1]);
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i >= g.M || j >= g.N) continue;
            double v = acc[r][c];
            if (MODE & MG_DIVIDE) v = v / (g.lz[i] + g.ly[j]);
            const long o = (long)i * g.N + j;
            if (MODE & MG_GATHER_C) { const int a = g.map[o]; if (a >= 0) g.cy[a] = v; }
            else g.C[o] = v;
        }
}

// ---- y = L z, L lower-banded (bandwidth b) stored by rows: L[i][j] = Lb[i*(b+1) + j - i + b], j = i-b .. i -----------------
// one wave per row, lanes over the band (coalesced), deterministic shuffle sum
__global__ __launch_bounds__(256) void k_mass_lmul(int n, int b, const double* __restrict__ Lb, const double* __restrict__ z,
                                                   double* __restrict__ y) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const double* row = Lb + (long)i * (b + 1);
    const int j0 = max(0, i - b);
    double acc = 0.0;
    for (int j = j0 + lane; j <= i; j += 64) acc = fma(row[j - i + b], z[j], acc);
    acc = wave_sum(acc);
    if (lane == 0) y[i] = acc;
}

// ---- PCG pieces (fp64) -------------------------------------------------------------------------------------------------
// q = Wm p (the CSR of hmcmt_set_prior)
__global__ void k_mass_spmv(int n, const long long* __restrict__ row, const long long* __restrict__ col,
                            const double* __restrict__ val, const double* __restrict__ p, double* __restrict__ q) {
    const int a = TID1;
    if (a >= n) return;
    double acc = 0.0;
    for (long long t = row[a]; t < row[a + 1]; ++t) acc += val[t] * p[col[t]];
    q[a] = acc;
}
// out[slot] = sum_a u[a] v[a] (one workgroup: the solves this serves are the ragged, small ones; fixed order)
__global__ __launch_bounds__(1024) void k_mass_dot(int n, const double* __restrict__ u, const double* __restrict__ v,
                                                   double* out, int slot) {
    __shared__ double sh[16];
    double acc = 0.0;
    for (int a = threadIdx.x; a < n; a += 1024) acc += u[a] * v[a];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += sh[w];
        out[slot] = s;
    }
}
// x += alpha p ; r -= alpha q   (alpha = s[0] / s[1])
__global__ void k_mass_xr(int n, const double* s, const double* __restrict__ p, const double* __restrict__ q,
                          double* __restrict__ x, double* __restrict__ r) {
    const int a = TID1;
    if (a >= n) return;
    const double alpha = s[0] / s[1];
    x[a] += alpha * p[a];
    r[a] -= alpha * q[a];
}
// p = z + beta p   (beta = s[2] / s[0], then s[0] <- s[2] by the host's next round)
__global__ void k_mass_p(int n, const double* s, const double* __restrict__ z, double* __restrict__ p) {
    const int a = TID1;
    if (a >= n) return;
    p[a] = z[a] + (s[2] / s[0]) * p[a];
}

// ---- the leapfrog's position update with x = Wm^-1 p (HMCSampler.jl:237-247): dm = dt x, the step clamp and the reflection
// of lf_step_one; the reflection flips p, not x -----------------------------------------------------------------------------
// partial maxima of |dt x| (the step bound that lf_step_bound reads; k_lf_momentum_max's layout: LFNB blocks of 256)
__global__ __launch_bounds__(256) void k_mass_bound(int n, const double* __restrict__ x, double dt, double* part) {
    __shared__ double sh[4];
    double mx = 0.0;
    for (int a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB) mx = fmax(mx, fabs(dt * x[a]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
__global__ void k_mass_step(LfView L, const double* __restrict__ x, double dt, double lo, double hi) {
    const int a = TID1;
    if (a >= L.n) return;
    lf_step_dm(L, a, dt * x[a], lo, hi, lf_step_bound(L));
}
// the diagonal mass through hmcmt_mass_apply: y = invM x (op 0) or y = x / sqrt(invM) (op 1, sqrtM of setMassMatrix(nparam, s))
__global__ void k_mass_diag(int n, const double* __restrict__ invM, const double* x, double* y, int op) {
    const int a = TID1;
    if (a >= n) return;
    y[a] = op == 0 ? invM[a] * x[a] : x[a] / sqrt(invM[a]);
}

// ---- the low-rank-plus-diagonal mass (hmcmt_set_mass_lowrank): M^-1 = S (I + U (Lambda - I) U') S, M = F F' with
// F = S^-1 (I + U (Lambda^-1/2 - I) U'); arithmetic and its order in hmcmt_items.h (item_mass_lr_*).  Two launches per application,
// no atomics: every partial sum and every output has one owner, so the bits repeat.  x and y may be the same vector (thread a reads
// x[a] before it writes y[a], and the projection is complete before the expansion starts) -- hence no __restrict__ on them.
struct MassLr {
    int n, rank, op;               // op: HMCMT_MASS_OP_INV (x' = s x, post = s) or HMCMT_MASS_OP_SQRT (x' = x, post = 1 / s)
    const double* s;               // [n]
    const double* U;               // [rank][n]
    const double* c;               // [rank] lambda - 1 (INV) or lambda^-1/2 - 1 (SQRT)
    double* part;                  // [rank][LFNB] partial sums of U x'
};
static_assert(MASS_LR_RANK_MAX == HMCMT_MASS_RANK_MAX && MASS_LR_RANK_MAX % MASS_LR_CHUNK == 0 && MASS_LR_RANK_MAX <= 256,
              "the projection walks the directions in whole chunks; one thread per direction forms the weights");
// part[k][block] = this workgroup's share of sum_a U[k][a] x'[a]: lanes walk a (U[k][.] is contiguous), MASS_LR_CHUNK directions per
// pass over the cells so that the accumulators stay in registers
__global__ __launch_bounds__(256) void k_mass_lr_project(MassLr m, const double* x) {
    __shared__ double sh[4][MASS_LR_RANK_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k0 = 0; k0 < m.rank; k0 += MASS_LR_CHUNK) {
        const int nk = min(MASS_LR_CHUNK, m.rank - k0);
        double acc[MASS_LR_CHUNK];
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) acc[q] = 0.0;
        for (int a = blockIdx.x * 256 + threadIdx.x; a < m.n; a += 256 * LFNB)
            item_mass_lr_acc(m.U, m.n, k0, nk, item_mass_lr_pre(m.s, x, m.op, a), a, acc);
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) {
            const double t = wave_sum(acc[q]);
            if (lane == 0) sh[wave][k0 + q] = t;
        }
    }
    __syncthreads();
    if (threadIdx.x < m.rank) {
        const int k = threadIdx.x;
        m.part[k * LFNB + blockIdx.x] = item_mass_lr_block(sh[0][k], sh[1][k], sh[2][k], sh[3][k]);
    }
}
// y[a] = post[a] (x'[a] + sum_k U[k][a] w_k), w_k = c_k sum_b part[k][b]: every workgroup forms the rank weights itself (rank * LFNB
// loads, the sums in index order), then walks its cells
__global__ __launch_bounds__(256) void k_mass_lr_expand(MassLr m, const double* x, double* y) {
    __shared__ double w[MASS_LR_RANK_MAX];
    if (threadIdx.x < m.rank) w[threadIdx.x] = item_mass_lr_weight(m.part, m.c, threadIdx.x);
    __syncthreads();
    for (int a = blockIdx.x * 256 + threadIdx.x; a < m.n; a += 256 * LFNB)
        y[a] = item_mass_lr_expand(m.s, x, m.U, w, m.n, m.rank, m.op, a);
}
