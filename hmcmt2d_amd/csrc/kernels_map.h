// kernels_map.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// The MAP optimiser's kernels (hmcmt_map_*, host_map.h; include/hmcmt.h has the algorithm): projected L-BFGS whose direction is formed
// in the compact form -- one pass over the cells for the up to 2 history dot products, one serial launch for the small algebra, one
// pass for the direction and the trial model.  Arithmetic and its order in hmcmt_items.h (item_map_*): fp64 streaming kernels over at
// most 2 x 32 rows of n doubles, no floating-point atomics, every partial sum and every output with one owner, so the bits repeat and
// tests/emul reproduces them on the host.  Shapes: k_map_project is k_mass_lr_project's (LFNB workgroups of 256 threads, grid-stride,
// MASS_LR_CHUNK rows per pass in registers indexed at compile time, wave_sum, LDS, one partial sum per row and workgroup),
// k_map_expand is k_mass_lr_expand's (the coefficients into LDS, then one cell per thread and stride).
#pragma once

static_assert(MAP_HISTORY_MAX == HMCMT_MAP_HISTORY_MAX && MAP_ROWS_MAX % MASS_LR_CHUNK == 0 && MAP_PART_ROWS <= 256,
              "the projection walks the rows in whole chunks; one thread per row writes the workgroup's partial sum");

struct MapDir {
    MapRing R;                     // the ring as the direction reads it
    const double *m, *g;           // [n] the state
    double lo, hi;
    double* pg;                    // [n] projected gradient (written by the projection)
    double* d;                     // [n] direction (written by the expansion)
    double* mt;                    // [n] trial model
    double* part;                  // [MAP_PART_ROWS][LFNB]
    const double *SY, *YY;         // [H][H] by slot
    double* coef;                  // [MAP_COEF]
};

// the four waves' sums of one row -> the workgroup's partial sum; maxima and counts alike
__device__ __forceinline__ void map_block_rows(double (*sh)[MAP_PART_ROWS], int nrows, int extra0, int nextra, double* part) {
    __syncthreads();
    const int k = threadIdx.x;
    if (k < nrows || (k >= extra0 && k < extra0 + nextra)) {
        double v;
        if (k == MAP_P_MAX) v = fmax(fmax(sh[0][k], sh[1][k]), fmax(sh[2][k], sh[3][k]));
        else v = item_mass_lr_block(sh[0][k], sh[1][k], sh[2][k], sh[3][k]);
        part[k * LFNB + blockIdx.x] = v;
    }
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// Projection: pg from m, g and the bounds (written), the partial sums of [S; Y] pg (rows 0 .. 2 count - 1), of |pg|2^2 (MAP_P_X0), the
// partial maxima of |pg| (MAP_P_MAX) and the workgroup's share of |B| (MAP_P_NB, a count held in a double: exact below 2^53)
__global__ __launch_bounds__(256) void k_map_project(MapDir D) {
    __shared__ double sh[4][MAP_PART_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = D.R.n;
    {
        double s2 = 0.0, mx = 0.0, nb = 0.0;
        for (long long a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB) {
            const bool b = item_map_bound(D.m[a], D.g[a], D.lo, D.hi);
            const double pg = b ? 0.0 : D.g[a];
            D.pg[a] = pg;
            s2 = fma(pg, pg, s2); mx = fmax(mx, fabs(pg)); nb += b ? 1.0 : 0.0;
        }
        s2 = wave_sum(s2); nb = wave_sum(nb); mx = wave_max(mx);
        if (lane == 0) {
            sh[wave][MAP_P_X0] = s2; sh[wave][MAP_P_MAX] = mx; sh[wave][MAP_P_NB] = nb;
            sh[wave][MAP_P_X1] = sh[wave][MAP_P_X2] = sh[wave][MAP_P_X3] = sh[wave][MAP_P_X4] = 0.0;      // (a trial's rows: not this pass's)
        }
    }
    const int nrows = 2 * D.R.count;
    for (int q0 = 0; q0 < nrows; q0 += MASS_LR_CHUNK) {
        const int nq = min(MASS_LR_CHUNK, nrows - q0);
        double acc[MASS_LR_CHUNK];
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) acc[q] = 0.0;
        for (long long a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB)
            item_map_proj_acc(D.R, q0, nq, item_map_pg(D.m, D.g, D.lo, D.hi, a), a, acc);
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) {
            const double t = wave_sum(acc[q]);
            if (lane == 0) sh[wave][q0 + q] = t;
        }
    }
    map_block_rows(sh, nrows, MAP_P_X0, MAP_PART_ROWS - MAP_P_X0, D.part);
}

// the workgroups' partial sums of row k in index order
__device__ __forceinline__ double map_total(const double* part, int k) { return item_chain_total(part + (long long)k * LFNB); }
__device__ __forceinline__ double map_total_max(const double* part, int k) {
    double v = 0.0;
    for (int b = 0; b < LFNB; ++b) v = fmax(v, part[(long long)k * LFNB + b]);
    return v;
}

// Coefficients: ONE THREAD.  history <= 32, so the work is two triangular solves of at most 32 unknowns and a 32 x 32 product in fp64 --
// dependency chains a wave could shorten only by cross-lane reductions whose order the host instantiation would have to copy; latency
// is all that matters and one thread's serial order is the simplest one to repeat bit for bit.  totals (may be nullptr): the 2 count sums.
__global__ void k_map_coef(MapDir D, double* totals) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double t[MAP_ROWS_MAX];
    const int nrows = 2 * D.R.count;
    for (int q = 0; q < nrows; ++q) t[q] = map_total(D.part, q);
    if (totals)
        for (int q = 0; q < MAP_ROWS_MAX; ++q) totals[q] = q < nrows ? t[q] : 0.0;
    item_map_coef(D.R, D.SY, D.YY, t, map_total(D.part, MAP_P_X0), map_total_max(D.part, MAP_P_MAX), map_total(D.part, MAP_P_NB), D.coef);
}

// Expansion: d = -(gamma pg + S a + Y w) off B, 0 on B (written); the trial m_t = clip(m + alpha d)
__global__ __launch_bounds__(256) void k_map_expand(MapDir D, double alpha) {
    __shared__ double coef[MAP_COEF];
    if (threadIdx.x < MAP_COEF) coef[threadIdx.x] = D.coef[threadIdx.x];
    __syncthreads();
    for (long long a = blockIdx.x * 256 + threadIdx.x; a < D.R.n; a += 256 * LFNB) {
        const double d = item_map_dir(D.R, coef, D.pg[a], item_map_bound(D.m[a], D.g[a], D.lo, D.hi), a);
        D.d[a] = d;
        D.mt[a] = item_map_clip(D.m[a], alpha, d, D.lo, D.hi);
    }
}
// a backtrack: the clip alone with the new alpha
__global__ void k_map_clip(long long n, const double* __restrict__ m, const double* __restrict__ d, double alpha, double lo, double hi,
                           double* __restrict__ mt) {
    const long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a < n) mt[a] = item_map_clip(m[a], alpha, d[a], lo, hi);
}

// A trial behind its evaluation: the full gradient of the trial model and the sums the host decides with
struct MapTrial {
    long long n;
    const double *m0, *g0;         // the state (nullptr at hmcmt_map_begin: no step yet)
    const double* m1;              // the trial model
    const double* gdata;           // its data gradient
    double* g1;                    // its full gradient (written)
    double lambda;
    const double *mref, *wmVal;
    const long long *wmRow, *wmCol;
    double lo, hi;
    double* part;                  // [MAP_PART_ROWS][LFNB]: rows MAP_P_X0 .. MAP_P_X4 g0's, s'y, s's, y'y, |pg1|2^2; MAP_P_MAX, MAP_P_NB
};
__global__ __launch_bounds__(256) void k_map_trial(MapTrial T) {
    __shared__ double sh[4][MAP_PART_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, mx = 0.0, nb = 0.0;
    for (long long a = blockIdx.x * 256 + threadIdx.x; a < T.n; a += 256 * LFNB) {
        const double g1 = item_adapt_lr_grad(T.gdata, T.lambda, T.wmRow, T.wmCol, T.wmVal, T.m1, T.mref, a);
        T.g1[a] = g1;
        bool b;
        const double pg = item_map_trial(T.m0, T.g0, T.m1, g1, T.lo, T.hi, a, acc, &b);
        mx = fmax(mx, fabs(pg)); nb += b ? 1.0 : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const double t = wave_sum(acc[q]);
        if (lane == 0) sh[wave][MAP_P_X0 + q] = t;
    }
    mx = wave_max(mx); nb = wave_sum(nb);
    if (lane == 0) { sh[wave][MAP_P_MAX] = mx; sh[wave][MAP_P_NB] = nb; }
    map_block_rows(sh, 0, MAP_P_X0, MAP_PART_ROWS - MAP_P_X0, T.part);
}
// ... finished by one thread: scal[MS_GTS ..] from the partial sums in index order; M from k_lf_mnorm_final's scalar (D is already there)
__global__ void k_map_trial_final(const double* part, const double* mnorm, double* scal) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    scal[MS_M] = mnorm[0];
    scal[MS_GTS] = map_total(part, MAP_P_X0); scal[MS_STY] = map_total(part, MAP_P_X1); scal[MS_STS] = map_total(part, MAP_P_X2);
    scal[MS_YTY] = map_total(part, MAP_P_X3); scal[MS_PG2] = map_total(part, MAP_P_X4);
    scal[MS_PGINF] = map_total_max(part, MAP_P_MAX); scal[MS_NB] = map_total(part, MAP_P_NB);
}

// The pair of an accepted trial: s = m1 - m0 and y = g1 - g0 into the slot's rows, and the partial sums of [S; Y] y over the pairs that
// stay (R: the ring WITHOUT the new pair and, where it was full, without its oldest, whose slot the new pair takes -- no row that is
// read is written).  k_map_pair_final puts the new column of S'Y and the new row and column of Y'Y in place.
struct MapPair {
    MapRing R;
    double* rows;                  // the ring, writable
    int slot;
    const double *m0, *g0, *m1, *g1;
    double* part;
    double *SY, *YY;
    const double* scal;            // the accepted trial's (s'y, y'y)
};
__global__ __launch_bounds__(256) void k_map_pair(MapPair P) {
    __shared__ double sh[4][MAP_PART_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = P.R.n;
    double* srow = P.rows + (long long)P.slot * n;
    double* yrow = P.rows + (long long)(P.R.H + P.slot) * n;
    for (long long a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB) {
        srow[a] = P.m1[a] - P.m0[a];
        yrow[a] = P.g1[a] - P.g0[a];
    }
    const int nrows = 2 * P.R.count;
    for (int q0 = 0; q0 < nrows; q0 += MASS_LR_CHUNK) {
        const int nq = min(MASS_LR_CHUNK, nrows - q0);
        double acc[MASS_LR_CHUNK];
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) acc[q] = 0.0;
        for (long long a = blockIdx.x * 256 + threadIdx.x; a < n; a += 256 * LFNB)
            item_map_proj_acc(P.R, q0, nq, P.g1[a] - P.g0[a], a, acc);
#pragma unroll
        for (int q = 0; q < MASS_LR_CHUNK; ++q) {
            const double t = wave_sum(acc[q]);
            if (lane == 0) sh[wave][q0 + q] = t;
        }
    }
    map_block_rows(sh, nrows, 0, 0, P.part);
}
__global__ void k_map_pair_final(MapPair P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int H = P.R.H, c = P.R.count, ns = P.slot;
    for (int i = 0; i < c; ++i) {
        const int si = item_map_slot(P.R, i);
        P.SY[si * H + ns] = map_total(P.part, i);
        const double yy = map_total(P.part, c + i);
        P.YY[si * H + ns] = yy; P.YY[ns * H + si] = yy;
    }
    P.SY[ns * H + ns] = P.scal[MS_STY];
    P.YY[ns * H + ns] = P.scal[MS_YTY];
}
