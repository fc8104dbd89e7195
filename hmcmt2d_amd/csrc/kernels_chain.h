// kernels_chain.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// The vector kernels of the device-resident HMC chain (hmcmt_chain_*, host_chain.h): momentum draw, kinetic energy, the four
// Hamiltonian scalars of a sample, streaming posterior moments.  Bodies in hmcmt_items.h (item_chain_*).
//
// Plain streaming kernels over nAC doubles in the leapfrog kernels' pattern (kernels_path.h): LFNB workgroups of 256 threads
// leave LFNB partial sums, one thread adds them in index order -- no floating-point atomics, so the bits repeat.
#pragma once

static_assert(CHAIN_NB == LFNB && CHAIN_NT == 256, "the chain's reductions use the leapfrog kernels' launch shape");

// scalars of one sample, device side (Chain::d_scal); the first CHAIN_REC go to the pinned record in one copy
enum { CH_K0 = 0, CH_K1 = 1, CH_D1 = 2, CH_M1 = 3, CH_FLAG = 4, CHAIN_REC = 5, CHAIN_SCAL = 8 };

// p = clip(z, +-2.5) / sqrt(invM) and the partial sums of p' M^-1 p in one pass (diagonal mass)
__global__ __launch_bounds__(256) void k_chain_momentum(int n, const double* __restrict__ z, const double* __restrict__ invM,
                                                        double* __restrict__ p, double* __restrict__ part) {
    __shared__ double sh[32];
    double acc = 0.0, dummy = 0.0;
    for (int a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB) acc += item_chain_momentum(z, invM, p, a);
    block_sum2(acc, dummy, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// M = Wm: the clipped normals, which chol(Wm).L then multiplies (mass_apply_dev)
__global__ void k_chain_clip(int n, const double* __restrict__ z, double* __restrict__ out) {
    const int a = TID1;
    if (a < n) out[a] = item_chain_clip(z, a);
}
// The seeded chain's momentum (hmcmt_chain_sample): k_chain_momentum with the normal of cell a drawn in the thread that owns the cell
// (item_rng_normal: one Philox block, a log, a sqrt and a cos) -- nothing is read from d_z, and the thread-to-cell mapping and with
// it the order of the partial sums are k_chain_momentum's
__global__ __launch_bounds__(256) void k_chain_draw_momentum(int n, unsigned long long seed, unsigned int stream, unsigned long long t,
                                                             const double* __restrict__ invM, double* __restrict__ p,
                                                             double* __restrict__ part) {
    __shared__ double sh[32];
    double acc = 0.0, dummy = 0.0;
    for (int a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB) acc += item_chain_draw_momentum(seed, stream, t, invM, p, a);
    block_sum2(acc, dummy, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// ... and k_chain_clip with the drawn normal: in front of mass_apply_dev for the non-diagonal masses, and hmcmt_chain_normals' read-out
__global__ __launch_bounds__(256) void k_chain_draw_clip(int n, unsigned long long seed, unsigned int stream, unsigned long long t,
                                                         double* __restrict__ out) {
    const int a = TID1;
    if (a < n) out[a] = item_chain_draw_clip(seed, stream, t, a);
}
// partial sums of p' M^-1 p: x = M^-1 p from the mass solve (M = Wm), or x == nullptr and the diagonal invM
__global__ __launch_bounds__(256) void k_chain_kinetic(int n, const double* __restrict__ p, const double* __restrict__ x,
                                                       const double* __restrict__ invM, double* __restrict__ part) {
    __shared__ double sh[32];
    double acc = 0.0, dummy = 0.0;
    for (int a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB) acc += item_chain_kinetic(p, x, invM, a);
    block_sum2(acc, dummy, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// the final stage: [K0, K1, D1, M1, non-finite flag] of the sample.  partK0 / partK1: the partial sums at the start / at the
// proposal; D1 is where the trajectory's last evaluation left it (scal[CH_D1]); mnorm, flag: the leapfrog's own (LfView)
__global__ void k_chain_final(const double* __restrict__ partK0, const double* __restrict__ partK1, const double* __restrict__ mnorm,
                              const int* __restrict__ flag, double* __restrict__ scal) {
    if (TID1 != 0) return;
    scal[CH_K0] = 0.5 * item_chain_total(partK0);
    scal[CH_K1] = 0.5 * item_chain_total(partK1);
    scal[CH_M1] = mnorm[0];
    scal[CH_FLAG] = (double)flag[0];
}
// running mean and sum of squared deviations with the chain's current model; count includes this sample
__global__ void k_chain_welford(int n, const double* __restrict__ m, double* __restrict__ mean, double* __restrict__ m2, double count) {
    const int a = TID1;
    if (a < n) item_chain_welford(m, mean, m2, count, a);
}
// the end of a warm-up window (hmcmt_chain_adapt_*): the diagonal of M^-1 from the window's sums of squared deviations
__global__ void k_chain_adapt_mass(int n, const double* __restrict__ m2, double nm1, double w, double f, double* __restrict__ invM) {
    const int a = TID1;
    if (a < n) invM[a] = item_adapt_mass(m2, nm1, w, f, a);
}
// one count per target row for the chain's current model: thread r owns row r (bin-major counters, hmcmt_items.h), no atomics
__global__ __launch_bounds__(256) void k_chain_hist(long long ntarget, int nbins, double lo, double scale, const double* __restrict__ m,
                                                    const long long* __restrict__ target, unsigned int* __restrict__ counts) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < ntarget) item_chain_hist(m, target, counts, ntarget, nbins, lo, scale, r);
}
// out[iq][r]: one thread per (quantile, target) scans its row; the lanes of a wavefront read neighbouring rows of one bin together
__global__ __launch_bounds__(256) void k_chain_quantiles(long long ntarget, int nbins, int nq, double lo, double w,
                                                         const double* __restrict__ x, const unsigned int* __restrict__ counts,
                                                         double* __restrict__ out) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    const int iq = blockIdx.y;
    if (r >= ntarget || iq >= nq) return;
    int bin;
    out[(long long)iq * ntarget + r] = item_chain_quantile(counts, ntarget, nbins, lo, w, x[iq], r, &bin);
}
// the counters as hmcmt_chain_hist returns them: target-major
__global__ __launch_bounds__(256) void k_chain_hist_out(long long ntarget, int nbins, const unsigned int* __restrict__ counts,
                                                        unsigned int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ntarget * nbins) return;
    const long long r = i / nbins;
    const int b = (int)(i - r * nbins);
    out[i] = counts[(long long)b * ntarget + r];
}
// one counted commit of the autocovariance accumulator: thread (j, run) owns target j's lags [run * CHAIN_ACOV_RUN, ...) -- the lanes of
// a wavefront are neighbouring targets, every array lag-major (hmcmt_items.h); no thread reads what another writes in this launch
__global__ __launch_bounds__(256) void k_chain_acov(long long ntarget, int K, long long t, const double* __restrict__ m,
                                                    const long long* __restrict__ target, double* __restrict__ x0, double* __restrict__ tot,
                                                    double* __restrict__ S, double* __restrict__ H, double* ring) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k0 = (int)blockIdx.y * CHAIN_ACOV_RUN;
    if (j >= ntarget || k0 > K) return;
    const int k1 = k0 + CHAIN_ACOV_RUN < K + 1 ? k0 + CHAIN_ACOV_RUN : K + 1;
    item_chain_acov(m, target, x0, tot, S, H, ring, ntarget, K, t, j, k0, k1);
}
// acov[k][j] and mean[j]: one thread per target walks its lags with a running T_k (O(K) per target); neighbouring targets of one
// lag or ring slot are read and written together
__global__ __launch_bounds__(256) void k_chain_acov_out(long long ntarget, int K, long long N, const double* __restrict__ x0,
                                                        const double* __restrict__ tot, const double* __restrict__ S,
                                                        const double* __restrict__ H, const double* __restrict__ ring,
                                                        double* __restrict__ mean, double* __restrict__ acov) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j < ntarget) item_chain_acov_out(x0, tot, S, H, ring, ntarget, K, N, j, mean, acov);
}
// tau, ess and window: one thread per target walks its lags, neighbouring targets of one lag read together (as k_chain_quantiles)
__global__ __launch_bounds__(256) void k_chain_ess(long long ntarget, int K, long long N, double cap, double capTau,
                                                   const double* __restrict__ acov, double* __restrict__ tau, double* __restrict__ ess,
                                                   int* __restrict__ window) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j < ntarget) item_chain_ess(acov, ntarget, K, N, cap, capTau, j, tau, ess, window);
}
// one counted commit of the cross-moment accumulator: thread a owns cell a's pivot, sums and its double in the slot of this commit
__global__ __launch_bounds__(256) void k_chain_cov_commit(long long n, long long t, int slot, const double* __restrict__ m,
                                                          double* __restrict__ x0, double* __restrict__ tot, double* __restrict__ q,
                                                          double* __restrict__ pend) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a < n) item_chain_cov_commit(m, x0, tot, q, pend, n, t, slot, a);
}
// the rank-NB update of S from the parked commits.  A workgroup owns the tile rows [blockIdx.y * TILE_ROWS, ...) x cells
// [blockIdx.x * TILE_COLS, ...); thread = one cell a, so a wavefront reads and writes 512 contiguous bytes of one row of S.  The
// thread keeps pend[0 .. NB)[a] in registers; the rows' values pend[b][rho] are the same for every lane and come from a panel in
// LDS ([row of the tile][b]: one address per read, a broadcast).  Every S[r][a] has this one owner, which applies its NB fmas in slot
// order: no atomics, and the bits do not depend on how the commits were cut into flushes.  16 bytes of traffic per element against
// 2 NB flops: plain fp64 FMA.
template <int NB>
__global__ __launch_bounds__(CHAIN_COV_TILE_COLS) void k_chain_cov_flush(long long n, long long nrow, const long long* __restrict__ row,
                                                                         const double* __restrict__ pend, double* __restrict__ S) {
    __shared__ double panel[CHAIN_COV_TILE_ROWS * NB];
    const long long a = (long long)blockIdx.x * CHAIN_COV_TILE_COLS + threadIdx.x;
    double ycol[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) ycol[b] = a < n ? pend[(long long)b * n + a] : 0.0;
    // (blockIdx.y strides over the row tiles: the same trips for every thread of the workgroup, so the barriers are met by all)
    for (long long r0 = (long long)blockIdx.y * CHAIN_COV_TILE_ROWS; r0 < nrow; r0 += (long long)gridDim.y * CHAIN_COV_TILE_ROWS) {
        const int nr = (int)(nrow - r0 < CHAIN_COV_TILE_ROWS ? nrow - r0 : CHAIN_COV_TILE_ROWS);
        for (int i = threadIdx.x; i < nr * NB; i += CHAIN_COV_TILE_COLS) {
            const int r = i / NB, b = i - r * NB;
            const long long rho = row ? row[r0 + r] : r0 + r;
            panel[i] = pend[(long long)b * n + rho];
        }
        __syncthreads();
        if (a < n) {
            double* s = S + r0 * n + a;
#pragma unroll 4
            for (int r = 0; r < nr; ++r) s[(long long)r * n] = item_chain_cov_flush<NB>(panel + r * NB, ycol, s[(long long)r * n]);
        }
        __syncthreads();
    }
}
// cov[r][a], and from row 0's owners mean[a] and var[a]: blockIdx.y strides over the rows
__global__ __launch_bounds__(256) void k_chain_cov_out(long long n, long long nrow, double dN, const double* __restrict__ x0,
                                                       const double* __restrict__ tot, const double* __restrict__ q,
                                                       const double* __restrict__ S, const long long* __restrict__ row,
                                                       double* __restrict__ mean, double* __restrict__ var, double* __restrict__ cov) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    for (long long r = blockIdx.y; r < nrow; r += gridDim.y) item_chain_cov_out(x0, tot, q, S, row, n, dN, r, a, mean, var, cov);
}
__global__ __launch_bounds__(256) void k_chain_corr(long long n, long long nrow, double dN, const double* __restrict__ tot,
                                                    const double* __restrict__ q, const double* __restrict__ S,
                                                    const long long* __restrict__ row, double* __restrict__ corr) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    for (long long r = blockIdx.y; r < nrow; r += gridDim.y) item_chain_corr(tot, q, S, row, n, dN, r, a, corr);
}

// ---- low-rank mass in the warm-up (hmcmt_chain_adapt_lowrank; arithmetic and its order in hmcmt_items.h: item_adapt_lr_*) ----------
// Per stored step one launch of nAC threads (k_adapt_lr_store); per window end k_adapt_lr_mean, k_adapt_lr_gram, one download of K,
// then k_adapt_lr_lift and k_adapt_lr_sign.  The Gram matrix is plain fp64 fma, not v_mfma_f64_16x16x4_f64: the matrix instruction
// adds its four products per step in an order of its own, which the host instantiation (and the numpy reference, bit for bit) would
// have to mirror, for a kernel that runs once per window -- the MFMA form was not built, so there is no measurement of it.
struct AdaptLr {
    int nAC, n;                          // cells, stored pairs (W has 2n rows)
    double sq;                           // sqrt(n - 1)
    const double *X, *G;                 // [n][nAC] the stores
    const double *meanX, *meanG, *s;     // [nAC]
};
// row `slot` of both stores from the chain's current model and the data gradient the decision left: one thread per cell writes both
__global__ __launch_bounds__(256) void k_adapt_lr_store(LfView L, const double* __restrict__ gdata, double lambda, double* __restrict__ xrow,
                                                        double* __restrict__ grow) {
    const int a = TID1;
    if (a >= L.n) return;
    xrow[a] = L.m[a];
    grow[a] = item_adapt_lr_grad(gdata, lambda, L.wmRow, L.wmCol, L.wmVal, L.m, L.mref, a);
}
// the stored rows' means and s = sqrt(invM), one thread per cell
__global__ __launch_bounds__(256) void k_adapt_lr_mean(int nAC, int n, const double* __restrict__ X, const double* __restrict__ G,
                                                       const double* __restrict__ invM, double* __restrict__ meanX, double* __restrict__ meanG,
                                                       double* __restrict__ s) {
    const int a = TID1;
    if (a >= nAC) return;
    meanX[a] = item_adapt_lr_mean(X, nAC, n, a);
    meanG[a] = item_adapt_lr_mean(G, nAC, n, a);
    s[a] = sqrt(invM[a]);
}
// K = W W': workgroup b owns the ADAPT_LR_TILE x ADAPT_LR_TILE tile (bi, bj), bi <= bj, of the upper block triangle and writes its mirror;
// thread (ti, tj) owns K[i][j] and walks ALL cells upwards, ADAPT_LR_STRIP at a time: the two row blocks of W are formed on the fly
// (centred, scaled) into LDS, consecutive threads walking the cells of a row
__global__ __launch_bounds__(256) void k_adapt_lr_gram(AdaptLr w, double* __restrict__ K) {
    __shared__ double Ws[2][ADAPT_LR_TILE][ADAPT_LR_STRIP + 1];
    const int N2 = 2 * w.n, T = (N2 + ADAPT_LR_TILE - 1) / ADAPT_LR_TILE;
    int t = blockIdx.x, bi = 0;
    while (t >= T - bi) { t -= T - bi; ++bi; }
    const int bj = bi + t;
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    double acc = 0.0;
    for (int a0 = 0; a0 < w.nAC; a0 += ADAPT_LR_STRIP) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2 * ADAPT_LR_TILE * ADAPT_LR_STRIP / 256; ++q) {
            const int e = threadIdx.x + 256 * q;
            const int blk = e / (ADAPT_LR_TILE * ADAPT_LR_STRIP), row = (e / ADAPT_LR_STRIP) % ADAPT_LR_TILE, col = e % ADAPT_LR_STRIP;
            const int gi = (blk ? bj : bi) * ADAPT_LR_TILE + row, a = a0 + col;
            Ws[blk][row][col] = (gi < N2 && a < w.nAC) ? item_adapt_lr_w(w.X, w.G, w.meanX, w.meanG, w.s, w.nAC, w.n, w.sq, gi, a) : 0.0;
        }
        __syncthreads();
        const int lim = min(ADAPT_LR_STRIP, w.nAC - a0);
        for (int c = 0; c < lim; ++c) acc = item_adapt_lr_dot(Ws[0][ti][c], Ws[1][tj][c], acc);
    }
    const int i = bi * ADAPT_LR_TILE + ti, j = bj * ADAPT_LR_TILE + tj;
    if (i < N2 && j < N2) {
        K[(long long)i * N2 + j] = acc;
        if (bi != bj) K[(long long)j * N2 + i] = acc;       // (the diagonal tile's mirror entry has its own thread: the same products, the same bits)
    }
}
// U[k][a] = sum_i B[i][k] W[i][a]: one thread per cell, MASS_LR_CHUNK directions side by side (W[i][a] is formed once per chunk and row)
__global__ __launch_bounds__(256) void k_adapt_lr_lift(AdaptLr w, const double* __restrict__ B, int r, double* __restrict__ U) {
    const int a = TID1;
    if (a >= w.nAC) return;
    for (int k0 = 0; k0 < r; k0 += MASS_LR_CHUNK) {
        double acc[MASS_LR_CHUNK];
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) acc[q] = 0.0;
        for (int i = 0; i < 2 * w.n; ++i) {
            const double wi = item_adapt_lr_w(w.X, w.G, w.meanX, w.meanG, w.s, w.nAC, w.n, w.sq, i, a);
#pragma unroll
            for (int q = 0; q < MASS_LR_CHUNK; ++q)
                if (k0 + q < r) acc[q] = item_adapt_lr_dot(B[(long long)i * r + k0 + q], wi, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q)
            if (k0 + q < r) U[(long long)(k0 + q) * w.nAC + a] = acc[q];
    }
}
// the sign convention: workgroup k finds direction k's entry of largest magnitude (the lowest index among equals) and flips the
// direction where that entry is negative
__global__ __launch_bounds__(256) void k_adapt_lr_sign(int nAC, double* __restrict__ U) {
    __shared__ double shV[256];
    __shared__ long long shA[256];
    double* u = U + (long long)blockIdx.x * nAC;
    double best = -1.0;
    long long at = nAC;
    for (int a = threadIdx.x; a < nAC; a += 256) {
        const double v = fabs(u[a]);
        if (item_adapt_lr_beats(v, a, best, at)) { best = v; at = a; }
    }
    shV[threadIdx.x] = best; shA[threadIdx.x] = at;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o && item_adapt_lr_beats(shV[threadIdx.x + o], shA[threadIdx.x + o], shV[threadIdx.x], shA[threadIdx.x])) {
            shV[threadIdx.x] = shV[threadIdx.x + o]; shA[threadIdx.x] = shA[threadIdx.x + o];
        }
        __syncthreads();
    }
    const long long top = shA[0];
    if (top >= nAC || !(u[top] < 0.0)) return;
    __syncthreads();                                         // (every thread has read u[top] before its owner flips it)
    for (int a = threadIdx.x; a < nAC; a += 256) u[a] = -u[a];
}

// ---- the row sketch of the committed models (hmcmt_chain_sketch_*, hmcmt_chain_pca; arithmetic and its order in hmcmt_items.h:
// item_chain_sketch_*) ----------------------------------------------------------------------------------------------------------------
// Per counted commit one launch of nAC threads (k_chain_sketch_commit); per ell commits k_chain_sketch_gram, one download of K, one
// upload of T and k_chain_sketch_shrink; per hmcmt_chain_pca k_chain_sketch_mean, k_chain_sketch_gram, one download, one upload,
// k_chain_sketch_lift and k_adapt_lr_sign.  The Gram kernel is k_adapt_lr_gram's tiling over plain rows (a sibling, not a template
// of it: that kernel forms its rows on the fly from four arrays, this one reads them, and a shared body would hide both), in plain
// fp64 fma for the reason recorded above k_adapt_lr_gram: it runs once per ell commits and its host instantiation is bit for bit.
struct SketchRows {
    int nAC, nrows, nw;                  // cells, rows of B taken, rows of the operand (nw = nrows, or nrows + 1 with the extra row)
    const double* B;                     // [.][nAC]
    const double* extra;                 // [nAC] the operand's last row, or nullptr
};
// one counted commit: thread a owns cell a's pivot, sums and its double in the row of this commit
__global__ __launch_bounds__(256) void k_chain_sketch_commit(long long n, long long t, int pivotGiven, const double* __restrict__ m,
                                                             double* __restrict__ x0, double* __restrict__ tot, double* __restrict__ q,
                                                             double* __restrict__ brow) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a < n) item_chain_sketch_commit(m, x0, tot, q, brow, t, pivotGiven, a);
}
// K = W W' [nw][nw]: workgroup b owns the tile (bi, bj), bi <= bj, of the upper block triangle and writes its mirror; thread (ti, tj)
// owns K[i][j] and walks ALL cells upwards, ADAPT_LR_STRIP at a time through LDS, consecutive threads walking the cells of a row
__global__ __launch_bounds__(256) void k_chain_sketch_gram(SketchRows w, double* __restrict__ K) {
    __shared__ double Ws[2][ADAPT_LR_TILE][ADAPT_LR_STRIP + 1];
    const int N = w.nw, T = (N + ADAPT_LR_TILE - 1) / ADAPT_LR_TILE;
    int t = blockIdx.x, bi = 0;
    while (t >= T - bi) { t -= T - bi; ++bi; }
    const int bj = bi + t;
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    double acc = 0.0;
    for (int a0 = 0; a0 < w.nAC; a0 += ADAPT_LR_STRIP) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2 * ADAPT_LR_TILE * ADAPT_LR_STRIP / 256; ++q) {
            const int e = threadIdx.x + 256 * q;
            const int blk = e / (ADAPT_LR_TILE * ADAPT_LR_STRIP), row = (e / ADAPT_LR_STRIP) % ADAPT_LR_TILE, col = e % ADAPT_LR_STRIP;
            const int gi = (blk ? bj : bi) * ADAPT_LR_TILE + row, a = a0 + col;
            Ws[blk][row][col] = (gi < N && a < w.nAC) ? item_chain_sketch_row(w.B, w.extra, w.nAC, w.nrows, gi)[a] : 0.0;
        }
        __syncthreads();
        const int lim = min(ADAPT_LR_STRIP, w.nAC - a0);
        for (int c = 0; c < lim; ++c) acc = item_adapt_lr_dot(Ws[0][ti][c], Ws[1][tj][c], acc);
    }
    const int i = bi * ADAPT_LR_TILE + ti, j = bj * ADAPT_LR_TILE + tj;
    if (i < N && j < N) {
        K[(long long)i * N + j] = acc;
        if (bi != bj) K[(long long)j * N + i] = acc;         // (the diagonal tile's mirror entry has its own thread: the same products, the same bits)
    }
}
// B <- T B in place, rows ell .. 2 ell - 1 zeroed.  Thread = one cell a: it first copies ALL of column a (2 ell doubles, too many for
// registers) into its own column of the workgroup's LDS ([j][thread]: a wavefront's read of one j is 512 contiguous bytes, no bank
// conflict), so every later write of column a finds its inputs already taken -- that is what makes the update safe in place.  No
// thread reads another's column: no barrier.  T[i][j] is the same address for every lane (a scalar load); CHAIN_SKETCH_CHUNK output
// rows share one LDS read of col[j].  LDS: 2 ell * CHAIN_SKETCH_COLS * 8 bytes, dynamic (64 KiB at ell = 64: two workgroups per CU).
__global__ __launch_bounds__(CHAIN_SKETCH_COLS) void k_chain_sketch_shrink(long long nAC, int ell, const double* __restrict__ T, double* B) {
    extern __shared__ double sketchCol[];
    const long long a = (long long)blockIdx.x * CHAIN_SKETCH_COLS + threadIdx.x;
    if (a >= nAC) return;
    const int n2 = 2 * ell;
    double* col = sketchCol + threadIdx.x;
    for (int j = 0; j < n2; ++j) col[j * CHAIN_SKETCH_COLS] = B[(long long)j * nAC + a];
    for (int i0 = 0; i0 < ell; i0 += CHAIN_SKETCH_CHUNK) {
        double acc[CHAIN_SKETCH_CHUNK];
#pragma unroll
        for (int q = 0; q < CHAIN_SKETCH_CHUNK; ++q) acc[q] = 0.0;
        for (int j = 0; j < n2; ++j) {
            const double c = col[j * CHAIN_SKETCH_COLS];
#pragma unroll
            for (int q = 0; q < CHAIN_SKETCH_CHUNK; ++q)
                if (i0 + q < ell) acc[q] = fma(T[(long long)(i0 + q) * n2 + j], c, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < CHAIN_SKETCH_CHUNK; ++q)
            if (i0 + q < ell) B[(long long)(i0 + q) * nAC + a] = acc[q];
    }
    for (int i = ell; i < n2; ++i) B[(long long)i * nAC + a] = 0.0;
}
// the read-out's mean row sqrt(N) ybar into the staging row of B, one thread per cell
__global__ __launch_bounds__(256) void k_chain_sketch_mean(long long n, double dN, double sqN, const double* __restrict__ tot, double* __restrict__ brow) {
    const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
    if (a < n) brow[a] = item_chain_sketch_mean(tot[a], dN, sqN);
}
// U[k][a] = sum_i coef[i][k] W[i][a]: one thread per cell, MASS_LR_CHUNK directions side by side
__global__ __launch_bounds__(256) void k_chain_sketch_lift(SketchRows w, const double* __restrict__ coef, int r, double* __restrict__ U) {
    const int a = TID1;
    if (a >= w.nAC) return;
    for (int k0 = 0; k0 < r; k0 += MASS_LR_CHUNK) {
        double acc[MASS_LR_CHUNK];
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) acc[q] = 0.0;
        for (int i = 0; i < w.nw; ++i) {
            const double wi = item_chain_sketch_row(w.B, w.extra, w.nAC, w.nrows, i)[a];
#pragma unroll
            for (int q = 0; q < MASS_LR_CHUNK; ++q)
                if (k0 + q < r) acc[q] = item_adapt_lr_dot(coef[(long long)i * r + k0 + q], wi, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q)
            if (k0 + q < r) U[(long long)(k0 + q) * w.nAC + a] = acc[q];
    }
}
