// kernels_jvp_block.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// Block Jacobian products (hmcmt_jvp_block / hmcmt_jtvp_block / hmcmt_gn_hessvec_block): nvec directions at one linearisation
// point, ONE solve per route for all of them.  To the solver the block is a problem with nvec * nFreq frequencies whose frequency
// list repeats nvec times -- the VIRTUAL systems
//     sv(j, s) = j nFreq + s                          s <  nFreq   (TE)
//                nvec nFreq + j nFreq + (s - nFreq)   s >= nFreq   (TM)
// so that `mode = sv >= nvec nFreq` holds as in every solver kernel.  The kernels here are the direction-blocked forms of
// kernels_jvp.h and of the gradient's / Jacobian's kernels J^T u runs; the item functions are the shared ones of hmcmt_items.h.
// Two kinds of arrays per direction:
//     work arrays   [nvec][...] in the single product's layout, the REAL system index inside a direction (dSig, dbc*, vbar, rxCoef,
//                   qPart, gPartG, srcB, wL/wR, colw, gL/gR, jv, u, scale, sysOn)
//     solver fields [nvec S][vstride] by virtual system (R, the tangent field dF, the adjoint field Lam)
// dir_view moves a View's pointers to direction j: uniform arithmetic (j and the mode come from the block index), after which an
// item function sees the single product's View.  The two dense contractions with dBC do not go that way: they hold a chunk of
// directions in registers and read every dBC element once per chunk (k_blk_dbc, k_blk_contract).
#pragma once

constexpr int BLK_KB = 8;               // directions per register chunk of the dBC contractions

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

__global__ __launch_bounds__(256) void k_blk_dsig(View v, int wrt, int nvec) {
    const int c = TID1;
    if (c < v.nCell) item_dsigma(dir_view(v, blockIdx.y, 0, nvec), c, wrt);
}

// k_jvp_norm for every direction at once: workgroup j normalises direction j (x + j stride) and leaves its pair of scales in
// scale[4 j + off]; dirOn[j] = the direction is not identically zero (its systems are solved)
__global__ __launch_bounds__(1024) void k_blk_norm(double* x, const double* den, long n, long stride, double* scale, int off, int* dirOn) {
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
    if (threadIdx.x == 0) { scale[4 * j + off] = dn; scale[4 * j + off + 1] = ldexp(1.0, e); dirOn[j] = mx > 0.0 ? 1 : 0; }
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

// dbc = dBC dSigma for a chunk of BLK_KB directions: a thin GEMM.  k_jvp_dbc's shape -- a wavefront per boundary node, lanes across
// the layers, DPP wave sum -- with one accumulator per direction in every lane: a dBC element (side nodes) / a gMn element (bottom
// nodes) is loaded once and used for all directions of the chunk.  Per direction the terms and their order are k_jvp_dbc's.
__global__ __launch_bounds__(64 * DBC_WAVES) void k_blk_dbc(View v, int nvec) {
    const int s = blockIdx.y, j0 = blockIdx.z * BLK_KB, lane = threadIdx.x & 63, node = blockIdx.x * DBC_WAVES + (threadIdx.x >> 6);
    const int nside = 2 * v.nz, nnode = nside + v.ny - 1;
    if (node >= nnode) return;                               // (uniform over the wavefront)
    const int nj = min(BLK_KB, nvec - j0);
    cplx acc[BLK_KB];
    bool on[BLK_KB];
#pragma unroll
    for (int q = 0; q < BLK_KB; ++q) { acc[q] = cplx{0.0, 0.0}; on[q] = q < nj && v.sysOn[(long)(j0 + q) * v.S + s] != 0; }
    if (node < nside) {
        const int prof = node / v.nz, iz = node % v.nz + 1;
        const cplx* D = v.dBC + (((long)s * 2 + prof) * v.nz + (iz - 1)) * v.nz;
        const double* ds = v.dSig + (long)j0 * v.nCell + (prof ? v.ny - 1 : 0);
        for (int c = lane; c < v.nz; c += 64) {
            const cplx d = D[c];
#pragma unroll
            for (int q = 0; q < BLK_KB; ++q)
                if (on[q]) acc[q] += ds[(long)q * v.nCell + (long)c * v.ny] * d;
        }
#pragma unroll
        for (int q = 0; q < BLK_KB; ++q) {
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
            for (int q = 0; q < BLK_KB; ++q)
                if (on[q]) {
                    const double* d = ds + (long)q * v.nCell + (long)c * v.ny;
                    acc[q] += ((ya / (ya + yb)) * d[iy - 1] + (yb / (ya + yb)) * d[iy]) * g;
                }
        }
#pragma unroll
        for (int q = 0; q < BLK_KB; ++q) {
            const cplx t = cplx{wave_sum(acc[q].re), wave_sum(acc[q].im)};
            if (lane == 0 && q < nj) v.dbcB[((long)(j0 + q) * v.S + s) * (v.ny + 1) + iy] = t;
        }
    }
}

// tangent right-hand sides: grid (nodes, S, nvec) -- the forward fields of a system stay in cache across its directions
__global__ __launch_bounds__(256) void k_blk_rhs(View v, int nvec) {
    const int s = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= v.vstride) return;
    item_tangent_rhs(dir_view(v, blockIdx.z, s >= v.nFreq, nvec), s, (int)(e % v.NYP), (int)(e / v.NYP));
}

// data side: a thread per (system, functional), the directions in a loop -- the functional's record (rxD, rxN0, Zrx) stays in cache
__global__ __launch_bounds__(64) void k_blk_data(View v, int nvec) {
    const int r = TID1, s = blockIdx.y;
    if (r >= v.nRx) return;
    for (int j = 0; j < nvec; ++j) item_tangent_data(dir_view(v, j, s >= v.nFreq, nvec), s, r);
}

// u = W^2 (J v), every direction: dataW read once per datum
__global__ __launch_bounds__(256) void k_blk_w2(View v, cplx* u, int nvec) {
    const int p = TID1;
    if (p >= v.nData) return;
    const double w2 = v.dataW[p] * v.dataW[p];
    for (int j = 0; j < nvec; ++j) u[(long)j * v.nData + p] = w2 * v.jv[(long)j * v.nData + p];
}

__global__ __launch_bounds__(256) void k_blk_vbar(View v, int nvec) {
    const int p = TID1;
    if (p >= v.nData) return;
    for (int j = 0; j < nvec; ++j) item_vbar_free(dir_view(v, j, 0, nvec), p);
}

__global__ __launch_bounds__(64) void k_blk_rxcoef(View v, int nvec) {
    const int r = TID1, s = blockIdx.y;
    if (r >= v.nRx) return;
    for (int j = 0; j < nvec; ++j) item_rxcoef(dir_view(v, j, 0, nvec), s, r);
}

// adjoint sources and receiver-layer Q-terms (k_src's two halves, the item functions): blocks x < nsrc the sources
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

// boundary weights and bottom-row column weights (k_jac_wb per direction)
__global__ __launch_bounds__(128) void k_blk_wb(View v, int nvec) {
    const int s = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
    const View w = dir_view(v, blockIdx.z, s >= v.nFreq, nvec);
    if (!w.sysOn[s]) return;
    if (e < w.nz) item_wside(w, s, e + 1);
    else if (e < w.nz + w.ny) item_colw(w, s, e - w.nz);
}

// dBC^T w per edge profile for a chunk of BLK_KB directions: k_jac_contract's arithmetic (BCC_L lanes per column, contiguous
// quarters of the rows, the quarters added in lane order) with one accumulator per direction -- a dBC element is loaded once per chunk
__global__ __launch_bounds__(128) void k_blk_contract(View v, int nvec) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, c = t / BCC_L, l = t % BCC_L, prof = blockIdx.y & 1, j0 = (blockIdx.y >> 1) * BLK_KB, s = blockIdx.z;
    const int nj = min(BLK_KB, nvec - j0);
    cplx acc[BLK_KB];
    bool on[BLK_KB];
#pragma unroll
    for (int q = 0; q < BLK_KB; ++q) { acc[q] = cplx{0.0, 0.0}; on[q] = q < nj && c < v.nz && v.sysOn[(long)(j0 + q) * v.S + s] != 0; }
    if (c < v.nz) {
        const cplx* D = v.dBC + ((long)s * 2 + prof) * v.nz * v.nz + c;
        const cplx* w = (prof == 0 ? v.wL : v.wR) + ((long)j0 * v.S + s) * v.nz;
        const int per = (v.nz + BCC_L - 1) / BCC_L, r0 = l * per, r1 = min(r0 + per, v.nz);
        for (int r = r0; r < r1; ++r) {
            const cplx d = D[(long)r * v.nz];
#pragma unroll
            for (int q = 0; q < BLK_KB; ++q)
                if (on[q]) acc[q] += d * w[(long)q * v.S * v.nz + r];
        }
    }
#pragma unroll
    for (int q = 0; q < BLK_KB; ++q) {
        const double r1 = __shfl_down(acc[q].re, 1, BCC_L), r2 = __shfl_down(acc[q].re, 2, BCC_L), r3 = __shfl_down(acc[q].re, 3, BCC_L);
        const double i1 = __shfl_down(acc[q].im, 1, BCC_L), i2 = __shfl_down(acc[q].im, 2, BCC_L), i3 = __shfl_down(acc[q].im, 3, BCC_L);
        if (on[q] && l == 0) {
            const cplx tot = cplx{((acc[q].re + r1) + r2) + r3, ((acc[q].im + i1) + i2) + i3};
            (prof == 0 ? v.gL : v.gR)[((long)(j0 + q) * v.S + s) * v.nz + c] = tot;
        }
    }
}

// P-terms: grid (cells, 2 modes x GRAD_NG groups, nvec)
__global__ __launch_bounds__(128) void k_blk_gradcell(View v, int nvec) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, mode = blockIdx.y / GRAD_NG, grp = blockIdx.y % GRAD_NG;
    if (c < v.nCell) item_gradcell_group(dir_view(v, blockIdx.z, mode, nvec), mode, grp, c);
}

// final assembly: a thread per active cell, the directions in a loop (cell geometry and exp(m) read once)
__global__ __launch_bounds__(128) void k_blk_final(View v, int wrt, double* out, int nvec) {
    const int a = TID1;
    if (a >= v.nAC) return;
    for (int j = 0; j < nvec; ++j) {
        const View w = dir_view(v, j, 0, nvec);
        out[(long)j * v.nAC + a] = jtvp_cell(w, a, wrt, w.gPartG, 2 * GRAD_NG, w.tanScale[3]);
    }
}
