// kernels_jac.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// The explicit Jacobian (hmcmt_jacobian / hmcmt_sensitivity; compJacMat.jl / compJacTMat.jl by the adjoint route).  One batch =
// one receiver j in every system: the adjoint solve of the gradient with receiver j's functional row as its source (unit
// coefficient), then per datum of that receiver the complex row of J over the active cells.  The View handed to these kernels
// is the context's with the Jacobian's own solution and boundary arrays (Lam, srcB, wL, wR, colw, gL, gR) and the batch's
// system flags (sysOn); the bodies are the gradient's item functions (hmcmt_items.h), kept complex and per system.
#pragma once

struct JacEntry { int p, row, s, kind; };   // datum p (data order) -> output row, its system and data kind (item_resid)

// The right-hand side of the batch: receiver j's functional row L_j^T on the two node rows of the receiver layer (interior
// part -> R, boundary part -> srcB; item_src with coefficient 1 for receiver j, 0 for the others), and the complex Q-term per
// system and receiver-layer cell (item_qterm, same coefficient).  Blocks x < nsrc: the sources; the blocks behind them: qJ.
__global__ __launch_bounds__(128) void k_jac_src(View v, int j, cplx* qJ, int nsrc) {
    const int s = blockIdx.y;
    if (!v.sysOn[s]) return;
    const long k = (long)s * v.nRx + j;
    const int n0 = v.rxN0[k];
    const cplx* D = v.rxD + k * 11;
    if ((int)blockIdx.x >= nsrc) {
        const int ky = (blockIdx.x - nsrc) * blockDim.x + threadIdx.x;
        if (ky < v.ny) {
            const int o = ky - n0;
            qJ[(long)s * v.ny + ky] = (o >= 0 && o < 3) ? D[8 + o] : cplx{0, 0};
        }
        return;
    }
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * (v.ny + 1)) return;
    const int row = e / (v.ny + 1), iy = e % (v.ny + 1), iz = v.zid + row;
    const int o = iy - n0;
    const cplx acc = (o >= 0 && o < 4) ? D[row * 4 + o] : cplx{0, 0};
    const bool interior = iz >= 1 && iz <= v.nz - 1 && iy >= 1 && iy <= v.ny - 1;
    if (interior) v.R[(long)s * v.vstride + nidx(v, iy, iz)] = acc;
    else if (iy == 0) v.srcB[(long)s * 4 + row * 2 + 0] = acc;
    else if (iy == v.ny) v.srcB[(long)s * 4 + row * 2 + 1] = acc;
}

// (behind the batch's solve: the boundary weights and the dBC contraction are the products' kernels at one direction, k_dir_wb and
// k_contract<1> of kernels_jvp.h)

// The rows of one batch are grouped by system (JacGroup: a run of the batch's list with one system): dZ of the system is formed
// once per cell (jac_cell), and every datum of the group -- for Rho_Pha the apparent resistivity and the phase of one receiver and
// system -- is derived from it (jac_datum; d/d(ln sigma) = sigma d/dsigma when wrt != 0).
struct JacGroup { int first, count; };   // entries [first, first + count) of the list

__device__ __forceinline__ cplx jac_scale(cplx val, const View& v, int a, int wrt) {
    if (!wrt) return val;
    const double sg = exp(v.m[a]);
    return cplx{val.re * sg, val.im * sg};
}

// rows of the batch: blockIdx.y = group, threads over the active cells -- a row is contiguous in a, the writes coalesce.
// cplxOut: interleaved complex rows of 2*nAC doubles (Impedance), else real rows of nAC doubles
__global__ __launch_bounds__(128) void k_jac_rows(View v, const JacEntry* __restrict__ list, const JacGroup* __restrict__ groups, int j,
                                                  const cplx* __restrict__ qJ, int wrt, int cplxOut, double* __restrict__ out) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= v.nAC) return;
    const JacGroup g = groups[blockIdx.y];
    const int s = list[g.first].s;
    const int cell = v.act[a];
    const cplx dz = jac_cell(v, s, cell % v.ny, cell / v.ny, qJ);
    const cplx z = v.Zrx[(long)s * v.nRx + j];
    for (int q = g.first; q < g.first + g.count; ++q) {
        const JacEntry e = list[q];
        const cplx val = jac_scale(jac_datum(e.kind, z, v.omega[s], dz), v, a, wrt);
        if (cplxOut) {
            double* o = out + ((long)e.row * v.nAC + a) * 2;
            o[0] = val.re; o[1] = val.im;
        } else out[(long)e.row * v.nAC + a] = val.re;
    }
}

// cumulative weighted sensitivity: sens2[a] += |dataW_p J_pa|^2 over the batch's data (groups in order, entries in order within a
// group); one thread per cell, so the sum order is fixed (bitwise repeatable).  k_jac_sens_final takes the square root.
__global__ __launch_bounds__(128) void k_jac_sens(View v, const JacEntry* __restrict__ list, const JacGroup* __restrict__ groups, int ng, int j,
                                                  const cplx* __restrict__ qJ, int wrt, double* __restrict__ sens2) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= v.nAC) return;
    const int cell = v.act[a];
    const int ky = cell % v.ny, kz = cell / v.ny;
    double acc = sens2[a];
    for (int gi = 0; gi < ng; ++gi) {
        const JacGroup g = groups[gi];
        const int s = list[g.first].s;
        const cplx dz = jac_cell(v, s, ky, kz, qJ);
        const cplx z = v.Zrx[(long)s * v.nRx + j];
        for (int q = g.first; q < g.first + g.count; ++q) {
            const JacEntry e = list[q];
            const cplx val = jac_scale(jac_datum(e.kind, z, v.omega[s], dz), v, a, wrt);
            const double w = v.dataW[e.p];
            acc += cabs2(cplx{w * val.re, w * val.im});
        }
    }
    sens2[a] = acc;
}
__global__ void k_jac_sens_final(double* sens, int n) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < n) sens[a] = sqrt(sens[a]);
}
