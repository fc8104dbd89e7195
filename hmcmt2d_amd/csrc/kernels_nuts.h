// kernels_nuts.h -- part of libhmcmt_hip.so; included by hmcmt_hip.hip INSIDE its anonymous namespace (one translation unit).
// The vector kernels of the device chain's No-U-turn sampler (hmcmt_chain_nuts_*, host_chain.h): beyond the leapfrog step and the mass
// application a leaf costs one pass over the cells (k_nuts_leaf) and one workgroup that finishes its sums (k_nuts_final).  Bodies in
// hmcmt_items.h (item_nuts_*).
//
// Launch shape and reduction are k_mass_lr_project's: LFNB workgroups of 256 threads walk the cells grid-stride, a thread's sums stay in
// registers indexed at compile time, the 64 lanes add up in wave_sum's tree, the four waves through LDS, the LFNB workgroups in index
// order in k_nuts_final -- no floating-point atomics, so the bits repeat.
#pragma once

static_assert(NUTS_DEPTH_MAX == HMCMT_NUTS_DEPTH_MAX, "the checkpoint slots are sized for the header's depth");
static_assert((long long)HMCMT_NUTS_HOOK_NMAX + 256LL * LFNB <= 0x7fffffffLL, "k_nuts_leaf's grid-stride index is an int: one stride past n must fit");

// the sample's buffers at the tree's start: both ends are the start state, the backward end with its momentum negated; rho = p0
__global__ void k_nuts_begin(int n, const double* __restrict__ m0, const double* __restrict__ p0, const double* __restrict__ x0,
                             double* __restrict__ mB, double* __restrict__ mF, double* __restrict__ pB, double* __restrict__ pF,
                             double* __restrict__ xB, double* __restrict__ xF, double* __restrict__ rho) {
    const int a = TID1;
    if (a >= n) return;
    const double m = m0[a], p = p0[a];
    mB[a] = m; mF[a] = m;
    pB[a] = -p; pF[a] = p;
    rho[a] = p;
    if (x0) { const double x = x0[a]; xB[a] = -x; xF[a] = x; }
}

// One pass of a leaf over the cells with NCK due checkpoints (NutsLeaf).  FIRST: rhoS, the checkpoint of an even leaf, p.x, and on a
// subtree's last leaf rhoNext and the merged tree's pair; a leaf with more than NUTS_GROUP due checkpoints takes the rest in further
// passes that only read.
template <int NCK, bool FIRST>
__global__ __launch_bounds__(256) void k_nuts_leaf(NutsLeaf L) {
    __shared__ double sh[4][NUTS_NACC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[NUTS_NACC];
#pragma unroll
    for (int q = 0; q < NUTS_NACC; ++q) acc[q] = 0.0;
    for (int a = blockIdx.x * 256 + threadIdx.x; a < L.n; a += 256 * LFNB) item_nuts_cell<NCK, FIRST>(L, a, acc);
    constexpr int Q0 = FIRST ? 0 : 3, Q1 = 3 + 2 * NCK;
#pragma unroll
    for (int q = Q0; q < Q1; ++q) {
        const double t = wave_sum(acc[q]);
        if (lane == 0) sh[wave][q] = t;
    }
    __syncthreads();
    if (threadIdx.x >= Q0 && threadIdx.x < Q1) {
        const int q = threadIdx.x;
        L.part[item_nuts_row(L, q) * LFNB + blockIdx.x] = item_mass_lr_block(sh[0][q], sh[1][q], sh[2][q], sh[3][q]);
    }
}

// One workgroup behind a leaf's passes: thread q adds row q of part in index order; thread 0 puts D1, M1 and the flag that the
// evaluation left in front of them, and the sample's K0 from the momentum's partial sums.  The leaf's one scalar copy follows.
__global__ __launch_bounds__(64) void k_nuts_final(int nq, const double* __restrict__ part, const double* __restrict__ partK0,
                                                   const double* __restrict__ misfit, const double* __restrict__ mnorm,
                                                   const int* __restrict__ flag, double* __restrict__ scal) {
    const int q = threadIdx.x;
    if (q < nq) scal[NS_SUM + q] = item_chain_total(part + q * LFNB);
    if (q == 0) {
        scal[NS_D1] = misfit[0];
        scal[NS_M1] = mnorm[0];
        scal[NS_FLAG] = (double)flag[0];
        scal[NS_K0] = 0.5 * item_chain_total(partK0);
    }
}
