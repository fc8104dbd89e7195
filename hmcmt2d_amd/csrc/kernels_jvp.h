// kernels_jvp.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// Matrix-free Jacobian products at a linearisation point (hmcmt_linearize, hmcmt_jvp / hmcmt_jtvp / hmcmt_gn_hessvec and their
// _block forms): nvec directions, ONE solve per route for all of them.  ONE family of kernels; nvec = 1 is the single product.
//   J V    the tangent-linear route: dsigma -> tangent of the boundary values -> tangent right-hand sides -> the solve -> the data
//          functionals applied to the tangent fields.  Bodies: hmcmt_items.h (item_dsigma .. item_tangent_data), the transposes of
//          the gradient's / Jacobian's items.
//   J^T U  the gradient's adjoint half with vbar from the caller's U (item_vbar_free): receiver coefficients, adjoint sources, the
//          solve, boundary weights, the dBC contraction, P-terms, final assembly.  The explicit Jacobian's batches (host_jacobian.h)
//          launch k_dir_wb and k_contract<1> of this family with nvec = 1.
// To the solver a block is a problem with nvec * nFreq frequencies whose frequency list repeats nvec times -- the VIRTUAL systems
//     sv(j, s) = j nFreq + s                          s <  nFreq   (TE)
//                nvec nFreq + j nFreq + (s - nFreq)   s >= nFreq   (TM)
// so that `mode = sv >= nvec nFreq` holds as in every solver kernel (nvec = 1: sv = s).  Two kinds of arrays per direction:
//     work arrays   [nvec][...] in one direction's layout, the REAL system index inside a direction (dSig, dbc*, vbar, rxCoef,
//                   qPart, gPartG, srcB, wL/wR, colw, gL/gR, jv, u, scale, sysOn)
//     solver fields [nvec S][vstride] by virtual system (R, the tangent field dF, the adjoint field Lam)
// dir_view moves a View's pointers to direction j: uniform arithmetic (j and the mode come from the block index; the identity at
// nvec = 1), after which an item function sees one direction's View.  The two dense contractions with dBC do not go that way: they
// hold a chunk of KB directions in registers and read every dBC element once per chunk (k_dbc, k_contract; KB = 1 where nvec = 1).
// Small, latency-bound launches around one long one; every output element has one thread (or one wavefront) and a fixed
// summation order.
#pragma once

constexpr int BLK_KB = 8;               // directions per register chunk of the dBC contractions where nvec > 1

// the virtual system of (direction j, real system s)
__host__ __device__ __forceinline__ int blk_sv(int j, int s, int nFreq, int nvec) {
    return s < nFreq ? j * nFreq + s : nvec * nFreq + j * nFreq + (s - nFreq);
}

// the View of direction j for work on systems of `mode` (work that touches no solver field: either mode)
__device__ __forceinline__ View dir_view(View v, int j, int mode, int nvec) {
    const long sa = (long)j * v.S;
    v.tanV += (long)j * v.nAC; v.dSig += (long)j * v.nCell;
    v.dbcL += sa * v.nz; v.dbcR += sa * v.nz; v.dbcB += sa * (v.ny + 1);
    v.vbar += (long)j * v.nData; v.uData += (long)j * v.nData; v.jv += (long)j * v.nData;
    v.rxCoef += sa * v.nRx; v.qPart += sa * v.ny; v.gPartG += (long)j * 2 * GRAD_NG * v.nCell;
    v.srcB += sa * 4; v.wL += sa * v.nz; v.wR += sa * v.nz; v.colw += sa * v.ny; v.gL += sa * v.nz; v.gR += sa * v.nz;
    v.tanScale += 4 * j; v.sysOn += sa;
    const long sh = ((long)j * v.nFreq + (mode ? (long)(nvec - 1) * v.nFreq : 0)) * v.vstride;
    v.R += sh; v.dF += sh; v.Lam += sh;
    return v;
}

// ----------------------------------------------------------------------------------------------
// the steps of a block alone (nvec > 1): the second solver instance's pivots, the flags of the virtual systems, the sources
// ----------------------------------------------------------------------------------------------
// the operator's per-system arrays for the virtual systems: every direction gets the real system's inverse pivots
__global__ __launch_bounds__(256) void k_blk_replicate(const cplx* __restrict__ ip, const float2* __restrict__ ip32, cplx* __restrict__ op,
                                                       float2* __restrict__ op32, int nFreq, int nvec, long vstride) {
    const int s = blockIdx.y, j = blockIdx.z;
    const int svi = blk_sv(j, s, nFreq, nvec);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < vstride; e += (long)gridDim.x * blockDim.x) {
        op[(long)svi * vstride + e] = ip[(long)s * vstride + e];
        op32[(long)svi * vstride + e] = ip32[(long)s * vstride + e];
    }
}

// the systems solved: (direction j not identically zero) and (real system s carries data), by direction for the products' kernels
// (onDir[j S + s]) and by virtual system for the solver (onV[sv]); hostV: the latter again in mapped host memory, for the records
__global__ __launch_bounds__(256) void k_blk_flags(const int* __restrict__ dirOn, const int* __restrict__ realOn, int* __restrict__ onDir,
                                                   int* __restrict__ onV, int* __restrict__ hostV, int nFreq, int nvec) {
    const int i = TID1, S = 2 * nFreq;
    if (i >= nvec * S) return;
    const int j = i / S, s = i % S, q = (dirOn[j] && realOn[s]) ? 1 : 0, sv = blk_sv(j, s, nFreq, nvec);
    onDir[i] = q; onV[sv] = q; hostV[sv] = q;
}

// adjoint sources and receiver-layer Q-terms per direction (k_src's two halves, the item functions): blocks x < nsrc the sources.
// THE ONE PLACE where the pipeline chooses between two kernels: nvec = 1 launches k_src (kernels_path.h), the gradient's own
// hot-path kernel, untouched -- it stages the receiver table in LDS, worth 12 us at 40 receivers, which this one does not do.
__global__ __launch_bounds__(128) void k_blk_src(View v, int nsrc, int nvec) {
    const int s = blockIdx.y;
    const View w = dir_view(v, blockIdx.z, s >= v.nFreq, nvec);
    if ((int)blockIdx.x >= nsrc) {
        const int ky = (blockIdx.x - nsrc) * blockDim.x + threadIdx.x;
        if (ky < w.ny) item_qterm(w, s, ky);
        return;
    }
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < 2 * (w.ny + 1)) item_src(w, s, e / (w.ny + 1), e % (w.ny + 1));
}

// ----------------------------------------------------------------------------------------------
// J V
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dir_dsig(View v, int wrt, int nvec) {
    const int c = TID1;
    if (c < v.nCell) item_dsigma(dir_view(v, blockIdx.y, 0, nvec), c, wrt);
}

// Power-of-two normalisation of a product's input, workgroup j direction j (x + j stride): x <- 2^-e x with
// e = floor(log2 max_i |x_i| / den_i) (den null: 1), scale[4 j + off ..] = {2^-e, 2^e}; dirOn[j] = the direction is not identically
// zero (its systems are solved; null: not written).  The products are linear, and their right-hand sides have no natural scale --
// d sigma = 1 S/m on a cell of 5e-4 S/m is 2000 times the cell, and the TM source carries d sigma / sigma^2 --, while the
// mixed-precision preconditioner works in fp32 / bf16: the solve runs on an input of the size of the model itself
// (max |d sigma| / sigma in [1, 2)) and the result is multiplied back.  Powers of two: exact in binary; the maximum does not depend
// on the order it is taken in.
__global__ __launch_bounds__(1024) void k_dir_norm(double* x, const double* den, long n, long stride, double* scale, int off, int* dirOn) {
    __shared__ double sh[1024];
    const int j = blockIdx.x;
    x += (long)j * stride;
    double mx = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const double a = den ? fabs(x[i]) / den[i] : fabs(x[i]);
        mx = fmax(mx, a);
    }
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    mx = sh[0];
    const int e = (mx > 0.0 && mx < 1.7e308) ? ilogb(mx) : 0;
    const double dn = ldexp(1.0, -e);
    for (long i = threadIdx.x; i < n; i += blockDim.x) x[i] *= dn;
    if (threadIdx.x == 0) {
        scale[4 * j + off] = dn; scale[4 * j + off + 1] = ldexp(1.0, e);
        if (dirOn) dirOn[j] = mx > 0.0 ? 1 : 0;
    }
}

// Tangent of the boundary values, dbc = dBC dSigma, for a chunk of KB directions (a thin GEMM; KB = 1: one direction).  A row of
// dBC is contiguous, so a wavefront takes one boundary node -- lanes across the layers, DPP wave sum (fixed order) -- with one
// accumulator per direction in every lane: a dBC element (side nodes) / a gMn element (bottom nodes) is loaded once and used for
// all directions of the chunk.  Nodes of a system: 2 nz side nodes (left, then right; iz = 1..nz), then ny - 1 bottom nodes.
// Per direction the terms are dbc_side_term's / dbc_bottom_term's, in their order.
constexpr int DBC_WAVES = 4;
template <int KB>
__global__ __launch_bounds__(64 * DBC_WAVES) void k_dbc(View v, int nvec) {
    const int s = blockIdx.y, j0 = blockIdx.z * KB, lane = threadIdx.x & 63, node = blockIdx.x * DBC_WAVES + (threadIdx.x >> 6);
    const int nside = 2 * v.nz, nnode = nside + v.ny - 1;
    if (node >= nnode) return;                               // (uniform over the wavefront)
    const int nj = min(KB, nvec - j0);
    cplx acc[KB];
    bool on[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q) { acc[q] = cplx{0.0, 0.0}; on[q] = q < nj && v.sysOn[(long)(j0 + q) * v.S + s] != 0; }
    if (node < nside) {
        const int prof = node / v.nz, iz = node % v.nz + 1;
        const cplx* D = v.dBC + (((long)s * 2 + prof) * v.nz + (iz - 1)) * v.nz;
        const double* ds = v.dSig + (long)j0 * v.nCell + (prof ? v.ny - 1 : 0);
        for (int c = lane; c < v.nz; c += 64) {
            const cplx d = D[c];
#pragma unroll
            for (int q = 0; q < KB; ++q)
                if (on[q]) acc[q] += ds[(long)q * v.nCell + (long)c * v.ny] * d;
        }
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            const cplx t = cplx{wave_sum(acc[q].re), wave_sum(acc[q].im)};
            if (lane == 0 && q < nj) (prof ? v.dbcR : v.dbcL)[((long)(j0 + q) * v.S + s) * v.nz + iz - 1] = t;
        }
    } else {
        const int iy = node - nside + 1;
        const double ya = v.yLen[iy - 1], yb = v.yLen[iy];
        const double* ds = v.dSig + (long)j0 * v.nCell;
        for (int c = lane; c < v.nz; c += 64) {
            const cplx g = v.gMn[(long)s * v.nz + c];
#pragma unroll
            for (int q = 0; q < KB; ++q)
                if (on[q]) {
                    const double* d = ds + (long)q * v.nCell + (long)c * v.ny;
                    acc[q] += ((ya / (ya + yb)) * d[iy - 1] + (yb / (ya + yb)) * d[iy]) * g;
                }
        }
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            const cplx t = cplx{wave_sum(acc[q].re), wave_sum(acc[q].im)};
            if (lane == 0 && q < nj) v.dbcB[((long)(j0 + q) * v.S + s) * (v.ny + 1) + iy] = t;
        }
    }
}

// Tangent right-hand side of every system into the padded nodal layout the solver reads (every element of the system's slice is
// written: zero on the boundary nodes, the pad columns and the systems without data).  Grid (nodes, S, nvec): the forward fields
// of a system stay in cache across its directions.
__global__ __launch_bounds__(256) void k_dir_rhs(View v, int nvec) {
    const int s = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= v.vstride) return;
    item_tangent_rhs(dir_view(v, blockIdx.z, s >= v.nFreq, nvec), s, (int)(e % v.NYP), (int)(e / v.NYP));
}

// data side: a thread per (system, functional), its data scattered to data order; the directions in a loop -- the functional's
// record (rxD, rxN0, Zrx) stays in cache
__global__ __launch_bounds__(64) void k_dir_data(View v, int nvec) {
    const int r = TID1, s = blockIdx.y;
    if (r >= v.nRx) return;
    for (int j = 0; j < nvec; ++j) item_tangent_data(dir_view(v, j, s >= v.nFreq, nvec), s, r);
}

// u = W^2 (J v), the Gauss-Newton product's intermediate, kept on the device; every direction: dataW read once per datum
__global__ __launch_bounds__(256) void k_dir_w2(View v, cplx* u, int nvec) {
    const int p = TID1;
    if (p >= v.nData) return;
    const double w2 = v.dataW[p] * v.dataW[p];
    for (int j = 0; j < nvec; ++j) u[(long)j * v.nData + p] = w2 * v.jv[(long)j * v.nData + p];
}

// ----------------------------------------------------------------------------------------------
// J^T U
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dir_vbar(View v, int nvec) {
    const int p = TID1;
    if (p >= v.nData) return;
    for (int j = 0; j < nvec; ++j) item_vbar_free(dir_view(v, j, 0, nvec), p);
}

__global__ __launch_bounds__(64) void k_dir_rxcoef(View v, int nvec) {
    const int r = TID1, s = blockIdx.y;
    if (r >= v.nRx) return;
    for (int j = 0; j < nvec; ++j) item_rxcoef(dir_view(v, j, 0, nvec), s, r);
}

// boundary weights -Aio^T s (+ the source's boundary part) and the bottom-row column weights per direction
__global__ __launch_bounds__(128) void k_dir_wb(View v, int nvec) {
    const int s = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
    const View w = dir_view(v, blockIdx.z, s >= v.nFreq, nvec);
    if (!w.sysOn[s]) return;
    if (e < w.nz) item_wside(w, s, e + 1);
    else if (e < w.nz + w.ny) item_colw(w, s, e - w.nz);
}

// dBC^T w per edge profile for a chunk of KB directions: k_bcsens_contract's arithmetic (BCC_L lanes per column, contiguous
// quarters of the rows, the quarters added in lane order) with one accumulator per direction -- a dBC element is loaded once per
// chunk.  Rows go in batches of 8 / KB (the loads of a batch are requested together: eight in flight per lane, as in
// k_bcsens_contract, whatever KB is), and within a batch the accumulators are updated row by row: per direction the terms and
// their order are the same for every KB.  (k_bcsens_contract itself, on the gradient's path, stays its own copy.)
template <int KB>
__global__ __launch_bounds__(128) void k_contract(View v, int nvec) {
    constexpr int RB = 8 / KB;
    const int t = blockIdx.x * blockDim.x + threadIdx.x, c = t / BCC_L, l = t % BCC_L, prof = blockIdx.y & 1, j0 = (blockIdx.y >> 1) * KB, s = blockIdx.z;
    const int nj = min(KB, nvec - j0);
    cplx acc[KB];
    bool on[KB], any = false;
#pragma unroll
    for (int q = 0; q < KB; ++q) {
        acc[q] = cplx{0.0, 0.0};
        on[q] = q < nj && c < v.nz && v.sysOn[(long)(j0 + q) * v.S + s] != 0;
        any = any || on[q];
    }
    if (any) {
        const cplx* D = v.dBC + ((long)s * 2 + prof) * v.nz * v.nz + c;
        const cplx* w = (prof == 0 ? v.wL : v.wR) + ((long)j0 * v.S + s) * v.nz;
        const int per = (v.nz + BCC_L - 1) / BCC_L, r0 = l * per, r1 = min(r0 + per, v.nz);
        for (int rb = r0; rb < r1; rb += RB) {
            cplx d[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) d[i] = D[(long)min(rb + i, r1 - 1) * v.nz];      // (a short last batch: loaded again, not used)
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int q = 0; q < KB; ++q)
                    if (on[q] && rb + i < r1) acc[q] += d[i] * w[(long)q * v.S * v.nz + min(rb + i, r1 - 1)];
        }
    }
    // lanes 4c .. 4c+3 are neighbours in a wave (128 threads per workgroup: a multiple of four)
#pragma unroll
    for (int q = 0; q < KB; ++q) {
        const double r1 = __shfl_down(acc[q].re, 1, BCC_L), r2 = __shfl_down(acc[q].re, 2, BCC_L), r3 = __shfl_down(acc[q].re, 3, BCC_L);
        const double i1 = __shfl_down(acc[q].im, 1, BCC_L), i2 = __shfl_down(acc[q].im, 2, BCC_L), i3 = __shfl_down(acc[q].im, 3, BCC_L);
        if (on[q] && l == 0) {
            const cplx tot = cplx{((acc[q].re + r1) + r2) + r3, ((acc[q].im + i1) + i2) + i3};
            (prof == 0 ? v.gL : v.gR)[((long)(j0 + q) * v.S + s) * v.nz + c] = tot;
        }
    }
}

// P-terms: grid (cells, 2 modes x GRAD_NG groups, nvec)
__global__ __launch_bounds__(128) void k_dir_gradcell(View v, int nvec) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, mode = blockIdx.y / GRAD_NG, grp = blockIdx.y % GRAD_NG;
    if (c < v.nCell) item_gradcell_group(dir_view(v, blockIdx.z, mode, nvec), mode, grp, c);
}

// final assembly: a thread per active cell (partial sums in group order, then the systems in order), the directions in a loop
// (cell geometry and exp(m) read once)
__global__ __launch_bounds__(128) void k_dir_final(View v, int wrt, double* out, int nvec) {
    const int a = TID1;
    if (a >= v.nAC) return;
    for (int j = 0; j < nvec; ++j) {
        const View w = dir_view(v, j, 0, nvec);
        out[(long)j * v.nAC + a] = jtvp_cell(w, a, wrt, w.gPartG, 2 * GRAD_NG, w.tanScale[3]);
    }
}
