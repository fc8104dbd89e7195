// kernels_jvp.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// Matrix-free Jacobian products at a linearisation point (hmcmt_linearize / hmcmt_jvp / hmcmt_jtvp / hmcmt_gn_hessvec).
//   J v    the tangent-linear route: dsigma -> tangent of the boundary values -> tangent right-hand side -> ONE solve of all live
//          systems -> the data functionals applied to the tangent field.  Bodies: hmcmt_items.h (item_dsigma .. item_tangent_data),
//          the transposes of the gradient's / Jacobian's items.
//   J^T u  the gradient's adjoint half with vbar from the caller's u (item_vbar_free), then the gradient's own kernels (k_rxcoef,
//          k_src, k_jac_wb, k_jac_contract, k_gradcell) on the product's arrays and k_jtvp_final.
// The View handed to these kernels is the context's with the product's own solution, boundary and work arrays.  Small,
// latency-bound launches around one long one; every output element has one thread (or one wavefront) and a fixed summation order.
#pragma once

__global__ __launch_bounds__(256) void k_jvp_dsig(View v, int wrt) {
    const int c = TID1;
    if (c < v.nCell) item_dsigma(v, c, wrt);
}

// Power-of-two normalisation of a product's input (one workgroup): x <- 2^-e x with e = floor(log2 max_i |x_i| / den_i) (den null:
// 1), scale = {2^-e, 2^e}.  The products are linear, and their right-hand sides have no natural scale -- d sigma = 1 S/m on a cell
// of 5e-4 S/m is 2000 times the cell, and the TM source carries d sigma / sigma^2 --, while the mixed-precision preconditioner
// works in fp32 / bf16: the solve runs on an input of the size of the model itself (max |d sigma| / sigma in [1, 2)) and the result
// is multiplied back.  Powers of two: exact in binary; the maximum does not depend on the order it is taken in.
__global__ __launch_bounds__(1024) void k_jvp_norm(double* x, const double* den, long n, double* scale) {
    __shared__ double sh[1024];
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
    if (threadIdx.x == 0) { scale[0] = dn; scale[1] = ldexp(1.0, e); }
}

// Tangent of the boundary values: a row of dBC is contiguous, so a wavefront takes one boundary node -- lanes across the layers,
// DPP wave sum (fixed order).  Nodes of a system: 2 nz side nodes (left, then right; iz = 1..nz), then ny - 1 bottom nodes.
constexpr int DBC_WAVES = 4;
__global__ __launch_bounds__(64 * DBC_WAVES) void k_jvp_dbc(View v) {
    const int s = blockIdx.y, lane = threadIdx.x & 63, node = blockIdx.x * DBC_WAVES + (threadIdx.x >> 6);
    const int nside = 2 * v.nz, nnode = nside + v.ny - 1;
    if (node >= nnode) return;                               // (uniform over the wavefront)
    const bool on = v.sysOn[s] != 0;
    cplx acc = cplx{0.0, 0.0};
    if (node < nside) {
        const int prof = node / v.nz, iz = node % v.nz + 1;
        if (on) for (int c = lane; c < v.nz; c += 64) acc += dbc_side_term(v, s, prof, iz, c);
        acc = cplx{wave_sum(acc.re), wave_sum(acc.im)};
        if (lane == 0) (prof ? v.dbcR : v.dbcL)[(long)s * v.nz + iz - 1] = acc;
    } else {
        const int iy = node - nside + 1;
        if (on) for (int c = lane; c < v.nz; c += 64) acc += dbc_bottom_term(v, s, iy, c);
        acc = cplx{wave_sum(acc.re), wave_sum(acc.im)};
        if (lane == 0) v.dbcB[(long)s * (v.ny + 1) + iy] = acc;
    }
}

// Tangent right-hand side of every system into the padded nodal layout the solver reads (every element of the system's slice is
// written: zero on the boundary nodes, the pad columns and the systems without data).
__global__ __launch_bounds__(256) void k_jvp_rhs(View v) {
    const int s = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= v.vstride) return;
    item_tangent_rhs(v, s, (int)(e % v.NYP), (int)(e / v.NYP));
}

// data side: one thread per (system, functional), its data scattered to data order
__global__ __launch_bounds__(64) void k_jvp_data(View v) {
    const int e = TID1;
    if (e < v.S * v.nRx) item_tangent_data(v, e / v.nRx, e % v.nRx);
}

// u = W^2 (J v): the Gauss-Newton product's intermediate, kept on the device
__global__ __launch_bounds__(256) void k_jvp_w2(View v, cplx* u) {
    const int p = TID1;
    if (p >= v.nData) return;
    const double w2 = v.dataW[p] * v.dataW[p];
    u[p] = w2 * v.jv[p];
}

__global__ __launch_bounds__(256) void k_jtvp_vbar(View v) {
    const int p = TID1;
    if (p < v.nData) item_vbar_free(v, p);
}

// final assembly: one thread per active cell (partial sums in group order, then the systems in order)
__global__ __launch_bounds__(128) void k_jtvp_final(View v, int wrt, const double* scale, double* out) {
    const int a = TID1;
    if (a < v.nAC) out[a] = jtvp_cell(v, a, wrt, v.gPartG, 2 * GRAD_NG, scale[1]);
}
