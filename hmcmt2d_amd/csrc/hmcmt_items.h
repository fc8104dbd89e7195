// Per-item bodies of the "one thread = one item" kernels of the hot path, written against a
// plain-pointer view of the context's HBM arrays (struct View).  hmcmt_kernels.hip wraps each in
// a __global__ launcher; tests/emul/ instantiates the same bodies on the host for CPU unit tests.
//
// Data layout.  S = 2*nFreq systems, s < nFreq: TE at frequency s, else TM at
// frequency s-nFreq.  Every field-like vector lives on the PADDED NODAL GRID
//     v[s][iz][iy],  iz = 0..nz (NZP = nz+1 rows),  iy = 0..NYP-1,  NYP = roundup(ny+1, 16)
// with iy fastest; columns iy > ny are always zero, boundary nodes (iy=0, iy=ny, iz=0, iz=nz)
// hold Dirichlet values for a forward field and zero for residuals / search directions / adjoint
// fields.  This is the reference's nodal ordering `(iz-1)(ny+1)+iy` (MT2DFwdSolver.jl:232) with a
// padded row stride, so the interior/boundary split of getBoundaryIndex (:227-248) is implicit.
#pragma once
#include "hmcmt_math.h"
#include <stdint.h>
#if !defined(__HIPCC__)
#include <algorithm>
#endif
#include <cmath>
#include <vector>

namespace hmcmt {

struct View {
    // sizes
    int ny, nz, NYP, NZP, nFreq, S, nRx, nData, nAC, nCell;
    int twist;                     // 1: twisted (two-sided) factorisation of the FDM tridiagonals, see item_pivot
    int zid;                       // node row of the receivers (mt2DTE.jl:66-67), 0-based
    long long* ticks;              // HMCMT_TICKS (measurement only): [2][32] earliest start / latest end of the kernels around the solves
    int dbg;                       // test hooks (hmcmt_debug_flags): bit 1 = leave the boundary-derivative terms B^T v out of the gradient
    const int* gate;               // non-null: the kernel was queued BEHIND a persistent solve before the host knew its outcome and runs only if
    int gateGen;                   //   the solve left *gate == gateGen (every system converged); else it returns at once and the host queues it again
    long vstride;                  // NZP*NYP elements per system
    // mesh (constant)
    const double* yLen;            // [ny]
    const double* zLen;            // [nz]
    const double* omega;           // [S]
    const double* lam;             // [NYP] generalised eigenvalues of the y-operator (0 in the pad)
    const int* sysOn;              // [S] 0 for the systems of a polarisation without data (never solved)
    // model-dependent
    const double* m;               // [nAC] ln(sigma) on active cells
    double* sigma;                 // [nCell]
    const int* cell2act;           // [nCell] active index or -1
    const double* bg;              // [nCell]
    const int* act;                // [nAC] cell id of each active cell
    double* sigMeanA;              // [nz] arithmetic lateral mean (MT1DSensitivity.jl:313)
    double* sigMeanG;              // [nz] geometric lateral mean (the FDM background of both modes)
    // stencil coefficients on the padded nodal grid, per mode: [2][NZP*NYP]
    double* cY;                    // coupling node (iy,iz) <-> (iy+1,iz)
    double* cZ;                    // coupling node (iy,iz) <-> (iy,iz+1)
    double* dK;                    // diagonal of K
    double* dM;                    // node mass D (A = K + i*omega*D)
    // FDM background tridiagonals per mode: [2][NZP]
    double* mzq;                   // multiplies lambda_j
    double* dgz;                   // z-stiffness diagonal
    double* ofz;                   // z-stiffness coupling iz <-> iz+1
    double* mzs;                   // multiplies i*omega
    cplx* invp;                    // [S][NZP][NYP] inverse pivots of the per-(s,j) tridiagonal LDL^T
    // fields
    cplx* X;                       // forward fields (exTE | hxTM), padded nodal layout
    cplx* Lam;                     // adjoint fields
    cplx* R;                       // residual / right-hand side
    // receivers
    const int* rxIdn;              // [nRx] forward interpolation node `id` (0-based upper node)
    const double* rxDy1;           // [nRx]
    const double* rxDy2;           // [nRx]
    const int* rxKL;               // [nRx] linearInterp (sensUtils.jl:133-161)
    const int* rxKR;
    const double* rxWL;
    const double* rxWR;
    // (nRx counts the receiver FUNCTIONALS: with tipper data (nTip = number of receivers) functional r < nRx - nTip is receiver r's
    //  impedance and functional nRx - nTip + r its tipper T = Hz/Hy, TE systems only; the tables above repeat for the latter)
    cplx* Zrx;                     // [S][nRx] Z, or T for a tipper functional
    int* rxN0;                     // [S][nRx] derivative window start
    cplx* rxD;                     // [S][nRx][11]: d0[4], d1[4], dq[3]
    cplx* rxCoef;                  // [S][nRx] sum of conj(W^T W r) over the data of (s, rx)
    int nTip = 0;                  // number of tipper functionals (0: no tipper data, the tables below are not read)
    const int* rxCL = nullptr;     // [nRx] linRxMap2 (linearInterp on the cell centres): cells of Hz ...
    const int* rxCR = nullptr;
    const double* rxVL = nullptr;  // ... and their weights
    const double* rxVR = nullptr;
    // data
    const int* predSys;            // [nData] system of the p-th masked entry of the full table
    const int* predRx;             // [nData] receiver of it
    const int* datSys;             // [nData] system addressed by (freqID, dtID) of datum p
    const int* datRx;              // [nData] rxID-1
    const int* predKind;           // [nData] what the p-th masked table entry is: 0 impedance, 1 apparent resistivity, 2 phase (degrees),
                                   //   3 tipper T, 4 Re T, 5 Im T
    const int* datKind;            // [nData] the same for the component dtID of datum p addresses
    const cplx* obs;               // [nData]
    const double* dataW;           // [nData]
    cplx* pred;                    // [nData]
    cplx* vbar;                    // [nData] conj(W^T W (pred-obs))
    double* misfitPart;            // [nData] 0.5*|W(pred-obs)|^2
    double* gPartG;                // [2][GRAD_NG][nCell] P-terms by mode and frequency group (GPU launch)
    const int* srStart;            // [S*nRx+1] CSR of data per (s, rx)
    const int* srList;             // [nData]
    // boundary / gradient work arrays
    cplx* srcB;                    // [S][4]: source on (0,zid), (ny,zid), (0,zid+1), (ny,zid+1)
    cplx* wL;                      // [S][nz]  weights on left-boundary nodes iz = 1..nz
    cplx* wR;                      // [S][nz]
    cplx* colw;                    // [S][ny]
    cplx* gL;                      // [S][nz]  dBC^T w, left column cells
    cplx* gR;                      // [S][nz]
    cplx* gMn;                     // [S][nz]  last row of the mean-profile sensitivity
    cplx* dBC;                     // [S][2][nz rows][nz cols]  d(edge column field at row j+1)/d sigma_c, left / right profile
    cplx* bcsL;                    // [S][nz]  sensitivity-version boundary fields (TM term)
    cplx* bcsR;                    // [S][nz]
    cplx* bcsB;                    // [S]      mean-profile bottom value
    cplx* fwdTab;                  // [S][FWD_NQ][nz][ny+1] per-layer terms of the forward 1-D columns (layer_forward)
    cplx* sensTab;                 // [S][3][5][nz+1]  per-layer terms of the sensitivity profiles
    cplx* sensEu;                  // [S][3][nz+1]     up-going amplitude per row (scratch in stage 2)
    cplx* sensEd;                  // [S][3][nz+1]
    cplx* sensMix;                 // [S][3][4][nz]
    cplx* sensDz1;                 // [S][3][nz]       d z1 / d sigma_c
    cplx* sensZ1;                  // [S][3]
    int* sensDead;                 // [S][3]           cut-off row or nz+1
    double* qPart;                 // [S][ny] Q-term (explicit sigma-dependence of the data functional) per system
    double* gPart;                 // [2][nCell] P-term partial sums per mode
    double* grad;                  // [nAC]
    // matrix-free Jacobian products at a linearisation point (hmcmt_jvp / hmcmt_jtvp, kernels_jvp.h)
    const double* tanV = nullptr;  // [nAC] direction v of J v
    double* dSig = nullptr;        // [nCell] delta sigma on all cells
    cplx* dbcL = nullptr;          // [S][nz]  tangent of the Dirichlet values, left-boundary nodes iz = 1..nz
    cplx* dbcR = nullptr;          // [S][nz]
    cplx* dbcB = nullptr;          // [S][ny+1] bottom nodes iy = 1..ny-1 (the corners belong to the sides)
    const cplx* dF = nullptr;      // [S][NZP][NYP] tangent field (interior nodes)
    const cplx* uData = nullptr;   // [nData] the caller's data vector u of J^T u
    cplx* jv = nullptr;            // [nData] J v in the layout of pred
    const double* tanScale = nullptr;  // [2] {2^-e, 2^e}: the power of two the product's input was normalised by (null: none)
};

HD long nidx(const View& v, int iy, int iz) { return (long)iz * v.NYP + iy; }

// --- sigma = A*exp(m) + bg  (HMCSampler.jl:292-293, HMCUtility.jl:69-77)
HD void item_sigma(const View& v, int cell) {
    int a = v.cell2act[cell];
    v.sigma[cell] = v.bg[cell] + (a >= 0 ? exp(v.m[a]) : 0.0);
}

// --- lateral means of one cell row (arithmetic: MT1DSensitivity.jl:313; geometric: FDM background)
HD void item_rowmean(const View& v, int kz) {
    double sa = 0.0, sl = 0.0;
    for (int ky = 0; ky < v.ny; ++ky) {
        double s = v.sigma[(long)kz * v.ny + ky];
        sa += s;
        sl += log(s);
    }
    v.sigMeanA[kz] = sa / v.ny;
    v.sigMeanG[kz] = exp(sl / v.ny);
}

// --- 5-point stencil of  Grad' diag(AveCF*F*q) Grad  and node mass AveCN*F*s at one node
//     (MT2DFwdSolver.jl:124-135,150-161; MT2DOperators.jl:35-48,118-130).
//     mode 0 (TE): q = 1/mu0, s = sigma ; mode 1 (TM): q = 1/sigma, s = mu0.
HD double cellq(const View& v, int mode, int ky, int kz) {
    return mode == 0 ? 1.0 / MU0 : 1.0 / v.sigma[(long)kz * v.ny + ky];
}
HD double cells(const View& v, int mode, int ky, int kz) {
    return mode == 0 ? v.sigma[(long)kz * v.ny + ky] : MU0;
}
HD double coupY(const View& v, int mode, int iy, int iz) {   // edge (iy,iz)-(iy+1,iz), 1<=iz<=nz-1
    return -(0.5 / v.yLen[iy]) * (v.zLen[iz - 1] * cellq(v, mode, iy, iz - 1) + v.zLen[iz] * cellq(v, mode, iy, iz));
}
HD double coupZ(const View& v, int mode, int iy, int iz) {   // edge (iy,iz)-(iy,iz+1), 1<=iy<=ny-1
    return -(0.5 / v.zLen[iz]) * (v.yLen[iy - 1] * cellq(v, mode, iy - 1, iz) + v.yLen[iy] * cellq(v, mode, iy, iz));
}
HD void item_coef(const View& v, int mode, int iy, int iz, bool doK, bool doM) {
    const long o = (long)mode * v.vstride + nidx(v, iy, iz);
    const bool rowI = iz >= 1 && iz <= v.nz - 1, colI = iy >= 1 && iy <= v.ny - 1;
    if (doK) {
        double cy = 0.0, cz = 0.0, dk = 0.0;
        if (rowI && iy <= v.ny - 1) cy = coupY(v, mode, iy, iz);
        if (colI && iz <= v.nz - 1) cz = coupZ(v, mode, iy, iz);
        if (rowI && colI)
            dk = -(coupY(v, mode, iy, iz) + coupY(v, mode, iy - 1, iz) + coupZ(v, mode, iy, iz) + coupZ(v, mode, iy, iz - 1));
        v.cY[o] = cy; v.cZ[o] = cz; v.dK[o] = dk;
    }
    if (doM) {
        double d = 0.0;
        if (rowI && colI) {
            double ya = v.yLen[iy - 1], yb = v.yLen[iy], za = v.zLen[iz - 1], zb = v.zLen[iz];
            d = 0.25 * (ya * za * cells(v, mode, iy - 1, iz - 1) + yb * za * cells(v, mode, iy, iz - 1) +
                        ya * zb * cells(v, mode, iy - 1, iz) + yb * zb * cells(v, mode, iy, iz));
        }
        v.dM[o] = d;
    }
}

// --- background (laterally averaged) tridiagonal in z for the fast-diagonalisation
//     preconditioner: P = Ty (x) Mz_q + My (x) (Tz_q + i w Mz_s)   
// (values; item_fdm_z stores them, k_pivot also computes them straight into its LDS copy)
HD void fdm_z_values(const View& v, int mode, int iz, double& mzq, double& dgz, double& ofz, double& mzs) {
    if (iz < 1 || iz > v.nz - 1) { mzq = 0; dgz = 0; ofz = 0; mzs = 0; return; }
    double qa, qb, sa, sb;
    // the lateral mean of the background is the geometric mean of sigma for both modes (the arithmetic mean of the coefficient the
    // operator is linear in was tried in round 3 and removed: DESIGN section 9)
    const double* sTE = v.sigMeanG;
    if (mode == 0) { qa = qb = 1.0 / MU0; sa = sTE[iz - 1]; sb = sTE[iz]; }
    else { qa = 1.0 / v.sigMeanG[iz - 1]; qb = 1.0 / v.sigMeanG[iz]; sa = sb = MU0; }
    double za = v.zLen[iz - 1], zb = v.zLen[iz];
    mzq = 0.5 * (za * qa + zb * qb);
    mzs = 0.5 * (za * sa + zb * sb);
    dgz = qa / za + qb / zb;
    ofz = (iz <= v.nz - 2) ? -(qb / zb) : 0.0;
}
HD void item_fdm_z(const View& v, int mode, int iz) {
    const long o = (long)mode * v.NZP + iz;
    fdm_z_values(v, mode, iz, v.mzq[o], v.dgz[o], v.ofz[o], v.mzs[o]);
}

// --- inverse pivots of the (s, j) tridiagonal  d_iz = lam_j*mzq + dgz + i w mzs  in TWISTED form:
//     rows 1..mid are eliminated top-down, rows n..mid+1 bottom-up (two independent recurrences the
//     solve kernels run interleaved, halving their dependent chain); the factor that couples the two
//     halves at rows mid, mid+1 is stored in the unused boundary row iz = 0.
// View.twist selects it at run time: the fused forward kernel (k_fdm_fwd) runs the two halves in the two lane
//     halves of its sweeping wave and halves its serial chain; the stand-alone tridiagonal kernels, which read
//     global memory, are instruction-issue-bound and do not gain (20 us vs 16 us), so they use twist = 0
//     (mid = n: the classic Thomas factorisation) unless they have to follow the fused kernel's pivots.
HD int twist_mid(int n, int twist) { return twist ? (n + 1) / 2 : n; }   // rows 1..mid | mid+1..n   (n = nz-1 >= 2)
// (mzq, dgz, ofz, mzs: the mode's four coefficient rows -- the GPU kernel passes copies staged in LDS: read from global
// memory they cost the serial loop one memory round trip per step)
// ip32 (optional): complex64 copy of the pivots for the mixed-precision FDM stage, written along
HD void item_pivot_tab(const View& v, int s, int j, const double* mzq, const double* dgz, const double* ofz, const double* mzs,
                       float* ip32 = nullptr) {
    const double w = v.omega[s], lam = v.lam[j];
    cplx* ip = v.invp + (long)s * v.vstride + j;
    const int n = v.nz - 1, mid = twist_mid(n, v.twist);
    // the two recurrences are independent: one loop advances both (two dependent chains of complex reciprocals in
    // flight instead of one after the other: k_pivot 58 -> us)
    cplx pt = cplx{0, 0}, pb = cplx{0, 0};
    for (int t = 0; t < mid; ++t) {
        const int it = 1 + t, ib = n - t;
        {                                                  // d'_iz = d_iz - of_{iz-1}^2 / d'_{iz-1}
            cplx d = cplx{lam * mzq[it] + dgz[it], w * mzs[it]};
            if (it > 1) d -= (ofz[it - 1] * ofz[it - 1]) * pt;
            pt = crecip_plain(d);
            ip[(long)it * v.NYP] = pt;
            if (ip32) { ip32[2 * (long)it * v.NYP] = (float)pt.re; ip32[2 * (long)it * v.NYP + 1] = (float)pt.im; }
        }
        if (ib >= mid + 1) {                               // d''_iz = d_iz - of_iz^2 / d''_{iz+1}
            cplx d = cplx{lam * mzq[ib] + dgz[ib], w * mzs[ib]};
            if (ib < n) d -= (ofz[ib] * ofz[ib]) * pb;
            pb = crecip_plain(d);
            ip[(long)ib * v.NYP] = pb;
            if (ip32) { ip32[2 * (long)ib * v.NYP] = (float)pb.re; ip32[2 * (long)ib * v.NYP + 1] = (float)pb.im; }
        }
    }
    // middle coupling of the two normalised halves: x_mid + c x_{mid+1} = y'_mid, x_{mid+1} + c' x_mid = y''_{mid+1}
    // with c = o*ip_mid, c' = o*ip_{mid+1}; store 1/(1 - c c') in the unused boundary row iz = 0
    const double o = ofz[mid];
    const cplx jn = (mid + 1 <= n) ? crecip(cplx{1.0, 0.0} - (o * o) * (pt * pb)) : cplx{1.0, 0.0};   // (pt, pb: the pivots of rows mid, mid+1)
    ip[0] = jn;
    if (ip32) { ip32[0] = (float)jn.re; ip32[1] = (float)jn.im; }
}
HD void item_pivot(const View& v, int s, int j) {
    const int mode = s >= v.nFreq;
    item_pivot_tab(v, s, j, v.mzq + (long)mode * v.NZP, v.dgz + (long)mode * v.NZP, v.ofz + (long)mode * v.NZP,
                   v.mzs + (long)mode * v.NZP);
}

// --- per-layer terms of the 1-D column under boundary node column `col` (0 = left edge, ny = right
//     edge, else the width-weighted mean of the two adjacent cell columns, mt2DTE.jl:127-131)
HD double bc_column_sigma(const View& v, int j, int col) {
    if (col == 0) return v.sigma[(long)j * v.ny];
    if (col == v.ny) return v.sigma[(long)j * v.ny + v.ny - 1];
    const double ya = v.yLen[col - 1], yb = v.yLen[col];
    return (v.sigma[(long)j * v.ny + col - 1] * ya + v.sigma[(long)j * v.ny + col] * yb) / (ya + yb);
}
HD void item_bc_layers(const View& v, int s, int j, int col) {
    if (!v.sysOn[s]) return;
    const bool lastLayer = j + 1 >= v.nz;
    const double sig = bc_column_sigma(v, j, col), sigNext = lastLayer ? sig : bc_column_sigma(v, j + 1, col);
    cplx t[FWD_NQ];
    layer_forward(sig, sigNext, lastLayer, v.omega[s], v.zLen[j], t);
    const long ls = v.ny + 1, qs = (long)v.nz * ls;
    cplx* T = v.fwdTab + (long)s * FWD_NQ * qs + (long)j * ls + col;
    for (int q = 0; q < FWD_NQ; ++q) T[q * qs] = t[q];
}

// The per-layer tables depend on the frequency and the column profile, not on the polarisation: the GPU computes them
// once per frequency (slot f of fwdTab = the TE system's) for the frequencies with at least one polarisation in the data
HD void item_bc_layers_f(const View& v, int f, int j, int col) {
    if (!v.sysOn[f] && !v.sysOn[v.nFreq + f]) return;
    const bool lastLayer = j + 1 >= v.nz;
    const double sig = bc_column_sigma(v, j, col), sigNext = lastLayer ? sig : bc_column_sigma(v, j + 1, col);
    cplx t[FWD_NQ];
    layer_forward(sig, sigNext, lastLayer, v.omega[f], v.zLen[j], t);
    const long ls = v.ny + 1, qs = (long)v.nz * ls;
    cplx* T = v.fwdTab + (long)f * FWD_NQ * qs + (long)j * ls + col;
    for (int q = 0; q < FWD_NQ; ++q) T[q * qs] = t[q];
}

// --- Dirichlet values of the forward problem written into X's boundary nodes
//     (getBoundaryMT2DTE/TM, mt2DTE.jl:100-134, mt2DTM.jl:100-134).  col = 0..ny.
HD void item_bc_forward(const View& v, int s, int col) {
    if (!v.sysOn[s]) return;
    const bool tm = s >= v.nFreq;
    cplx* X = v.X + (long)s * v.vstride;
    X[nidx(v, col, 0)] = cplx{1.0, 0.0};                  // top row incl. corners
    const long ls = v.ny + 1, qs = (long)v.nz * ls;
    const cplx* T = v.fwdTab + (long)s * FWD_NQ * qs + col;
    if (col == 0 || col == v.ny) bc1d_forward_tab(v.omega[s], v.nz, T, qs, ls, tm, X + nidx(v, col, 1), v.NYP);
    else X[nidx(v, col, v.nz)] = bc1d_forward_tab(v.omega[s], v.nz, T, qs, ls, tm, nullptr, 0);
}

// --- y = K u + i w D u at one interior node (u on the padded nodal grid incl. boundary values)
HD cplx stencil_apply(const View& v, int s, const cplx* u, int iy, int iz) {
    const int mode = s >= v.nFreq;
    const long mo = (long)mode * v.vstride, o = nidx(v, iy, iz);
    const double *cY = v.cY + mo, *cZ = v.cZ + mo;
    cplx c = u[o];
    cplx acc = cplx{v.dK[mo + o] * c.re - v.omega[s] * v.dM[mo + o] * c.im,
                    v.dK[mo + o] * c.im + v.omega[s] * v.dM[mo + o] * c.re};
    acc += cY[o] * u[o + 1];
    acc += cY[o - 1] * u[o - 1];
    acc += cZ[o] * u[o + v.NYP];
    acc += cZ[o - v.NYP] * u[o - v.NYP];
    return acc;
}

// --- rhs = -Aio*bc (mt2DTE.jl:44): u = X with zero interior, so K u picks the boundary terms
HD void item_rhs(const View& v, int s, int iy, int iz) {
    const long o = (long)s * v.vstride + nidx(v, iy, iz);
    const bool interior = iz >= 1 && iz <= v.nz - 1 && iy >= 1 && iy <= v.ny - 1;
    if (!interior) { v.R[o] = cplx{0, 0}; return; }
    const int mode = s >= v.nFreq;
    const long mo = (long)mode * v.vstride, n = nidx(v, iy, iz);
    const cplx* X = v.X + (long)s * v.vstride;
    cplx acc = cplx{0, 0};
    if (iy == v.ny - 1) acc += v.cY[mo + n] * X[n + 1];
    if (iy == 1) acc += v.cY[mo + n - 1] * X[n - 1];
    if (iz == v.nz - 1) acc += v.cZ[mo + n] * X[n + v.NYP];
    if (iz == 1) acc += v.cZ[mo + n - v.NYP] * X[n - v.NYP];
    v.R[o] = -acc;
}

// --- tipper and its derivative at one tipper functional of one system (zero for TM systems, like an absent polarisation)
HD void item_rx_tipper(const View& v, int s, int r, bool wantDeriv) {
    const long k = (long)s * v.nRx + r;
    if (!v.sysOn[s] || s >= v.nFreq) {
        v.Zrx[k] = cplx{0, 0};
        if (wantDeriv) {
            v.rxN0[k] = 0;
            for (int i = 0; i < 11; ++i) v.rxD[k * 11 + i] = cplx{0, 0};
        }
        return;
    }
    const cplx* F0 = v.X + (long)s * v.vstride + nidx(v, 0, v.zid);
    cplx* D = wantDeriv ? v.rxD + k * 11 : nullptr;
    v.Zrx[k] = rx_tipper_deriv(v.omega[s], v.ny, F0, F0 + v.NYP, v.yLen, v.sigma + (long)v.zid * v.ny, v.zLen[v.zid],
                               v.rxKL[r], v.rxKR[r], v.rxWL[r], v.rxWR[r], v.rxCL[r], v.rxCR[r], v.rxVL[r], v.rxVR[r],
                               &v.rxN0[k], D);
}

// --- impedance and its derivative at one receiver of one system
HD void item_rx(const View& v, int s, int r, bool wantDeriv) {
    if (r >= v.nRx - v.nTip) { item_rx_tipper(v, s, r, wantDeriv); return; }
    if (!v.sysOn[s]) {                                    // polarisation absent from the data set
        v.Zrx[(long)s * v.nRx + r] = cplx{0, 0};
        if (wantDeriv) {
            v.rxN0[(long)s * v.nRx + r] = 0;
            for (int i = 0; i < 11; ++i) v.rxD[((long)s * v.nRx + r) * 11 + i] = cplx{0, 0};
        }
        return;
    }
    const bool tm = s >= v.nFreq;
    const cplx* F0 = v.X + (long)s * v.vstride + nidx(v, 0, v.zid);
    const cplx* F1 = F0 + v.NYP;
    const double* sig1 = v.sigma + (long)v.zid * v.ny;
    const double dz1 = v.zLen[v.zid];
    v.Zrx[(long)s * v.nRx + r] = rx_impedance(tm, v.omega[s], v.ny, F0, F1, v.yLen, sig1, dz1,
                                               v.rxIdn[r], v.rxDy1[r], v.rxDy2[r]);
    if (wantDeriv) {
        cplx* D = v.rxD + ((long)s * v.nRx + r) * 11;
        rx_impedance_deriv(tm, v.omega[s], v.ny, F0, F1, v.yLen, sig1, dz1, v.rxKL[r], v.rxKR[r],
                           v.rxWL[r], v.rxWR[r], &v.rxN0[(long)s * v.nRx + r], D, D + 4, D + 8);
    }
}

// --- residual, misfit terms and conj(W'W r) per datum (HMCSampler.jl:298-304, compJacTMatVec.jl:160)
//     DataType Rho_Pha: the data are rho_a = |Z|^2/(w mu0) and phi = atan2(Im Z, Re Z) in degrees (compMTRespTE,
//     mt2DTE.jl:253-255; compMTRespTM, mt2DTM.jl:236-238), real.  Their sensitivities are the impedance's times
//     2 conj(Z)/(w mu0) and -i (180/pi) conj(Z)/|Z|^2 (dataFuncSens.jl:137-141, :307-311); the residual weights being
//     real, the whole adjoint machinery stays the impedance one with vbar = weight x that factor.
HD void item_resid(const View& v, int p) {
    const int sp = v.predSys[p];
    const cplx z = v.Zrx[(long)sp * v.nRx + v.predRx[p]];
    const int kind = v.predKind[p];
    cplx val = z;
    if (kind == 1) val = cplx{cabs2(z) / (v.omega[sp] * MU0), 0.0};
    else if (kind == 2) val = cplx{atan2(z.im, z.re) * (180.0 / 3.14159265358979323846), 0.0};
    else if (kind == 4) val = cplx{z.re, 0.0};
    else if (kind == 5) val = cplx{z.im, 0.0};
    v.pred[p] = val;
    const cplx res = v.dataW[p] * (val - v.obs[p]);
    v.misfitPart[p] = 0.5 * cabs2(res);
    const cplx wr = v.dataW[p] * res;
    const int dk = v.datKind[p];
    if (dk == 0) { v.vbar[p] = conj(wr); return; }
    // tipper (z is T): T conj(wr), Re T wr.re, Im T -i wr.re -- Re(vbar dT) is the datum's term of the gradient
    if (dk == 3) { v.vbar[p] = conj(wr); return; }
    if (dk == 4) { v.vbar[p] = cplx{wr.re, 0.0}; return; }
    if (dk == 5) { v.vbar[p] = cplx{0.0, -wr.re}; return; }
    const int sd = v.datSys[p];
    const cplx zs = v.Zrx[(long)sd * v.nRx + v.datRx[p]];
    if (dk == 1) v.vbar[p] = (wr.re * 2.0 / (v.omega[sd] * MU0)) * conj(zs);
    else {
        const cplx c = conj(zs);                                   // -i conj(Z) = (Im conj Z, -Re conj Z)
        v.vbar[p] = (wr.re * (180.0 / 3.14159265358979323846) / cabs2(zs)) * cplx{c.im, -c.re};
    }
}

// --- per (s, rx): sum of vbar over the data addressing that receiver of that system
HD void item_rxcoef(const View& v, int s, int r) {
    const long k = (long)s * v.nRx + r;
    cplx c = cplx{0, 0};
    for (int t = v.srStart[k]; t < v.srStart[k + 1]; ++t) c += v.vbar[v.srList[t]];
    v.rxCoef[k] = c;
}

// --- adjoint source sVec = L^T conj(v) on node rows zid, zid+1 (compJacTMatVec.jl:208, :279):
//     interior part -> R, boundary part (iy = 0 / ny) -> srcB
HD void item_src(const View& v, int s, int row, int iy) {
    const int iz = v.zid + row;
    cplx acc = cplx{0, 0};
    for (int r = 0; r < v.nRx; ++r) {
        const long k = (long)s * v.nRx + r;
        const int o = iy - v.rxN0[k];
        if (o >= 0 && o < 4) acc += v.rxCoef[k] * v.rxD[k * 11 + row * 4 + o];
    }
    const bool interior = iz >= 1 && iz <= v.nz - 1 && iy >= 1 && iy <= v.ny - 1;
    if (interior) v.R[(long)s * v.vstride + nidx(v, iy, iz)] = acc;
    else if (iy == 0) v.srcB[(long)s * 4 + row * 2 + 0] = acc;
    else if (iy == v.ny) v.srcB[(long)s * 4 + row * 2 + 1] = acc;
}

// --- boundary weights w_b = s_b - (K lambda)_b  (compJacTMatVec.jl:240-242, :312-316)
HD cplx srcB_at(const View& v, int s, int side, int iz) {
    if (iz == v.zid) return v.srcB[(long)s * 4 + side];
    if (iz == v.zid + 1) return v.srcB[(long)s * 4 + 2 + side];
    return cplx{0, 0};
}
HD void item_wside(const View& v, int s, int iz) {          // iz = 1..nz
    const int mode = s >= v.nFreq;
    const long mo = (long)mode * v.vstride;
    const cplx* L = v.Lam + (long)s * v.vstride;
    cplx wl = srcB_at(v, s, 0, iz), wr = srcB_at(v, s, 1, iz);
    if (iz <= v.nz - 1) {
        wl -= v.cY[mo + nidx(v, 0, iz)] * L[nidx(v, 1, iz)];
        wr -= v.cY[mo + nidx(v, v.ny - 1, iz)] * L[nidx(v, v.ny - 1, iz)];
    }
    v.wL[(long)s * v.nz + iz - 1] = wl;
    v.wR[(long)s * v.nz + iz - 1] = wr;
}
HD cplx wbottom(const View& v, int s, int iy) {             // iy = 1..ny-1
    const int mode = s >= v.nFreq;
    const long mo = (long)mode * v.vstride;
    const cplx* L = v.Lam + (long)s * v.vstride;
    return -(v.cZ[mo + nidx(v, iy, v.nz - 1)] * L[nidx(v, iy, v.nz - 1)]);
}
HD void item_colw(const View& v, int s, int ky) {           // MT1DSensitivity.jl:315-328
    cplx c = cplx{0, 0};
    if (ky >= 1) c += wbottom(v, s, ky) * (v.yLen[ky] / (v.yLen[ky - 1] + v.yLen[ky]));
    if (ky + 1 <= v.ny - 1) c += wbottom(v, s, ky + 1) * (v.yLen[ky] / (v.yLen[ky] + v.yLen[ky + 1]));
    v.colw[(long)s * v.ny + ky] = c;
}

// --- 1-D sensitivities (getBCDerivMatrix, MT1DSensitivity.jl:253-333) in three stages.
//     prof 0: left edge column, 1: right edge column, 2: lateral-mean profile (:313-314)
HD void item_sens_layers(const View& v, int s, int prof, int j) {      // j = 0..nz (nz = half-space copy)
    if (!v.sysOn[s]) return;
    const int jj = j < v.nz ? j : v.nz - 1;
    const double sig = prof == 0 ? v.sigma[(long)jj * v.ny] : (prof == 1 ? v.sigma[(long)jj * v.ny + v.ny - 1] : v.sigMeanA[jj]);
    cplx t[5];
    layer_sens(sig, v.omega[s], v.zLen[jj], t);
    const long n1 = v.nz + 1;
    cplx* T = v.sensTab + ((long)s * 3 + prof) * 5 * n1 + j;
    for (int q = 0; q < 5; ++q) T[q * n1] = t[q];
}
HD void item_sens_profile(const View& v, int s, int prof) {
    if (!v.sysOn[s]) return;
    const bool tm = s >= v.nFreq;
    const long n1 = v.nz + 1, sp = (long)s * 3 + prof;
    const cplx* T = v.sensTab + sp * 5 * n1;
    cplx* fout = nullptr;
    long fstride = 1;
    if (tm) {                                             // `bc` of getBCderivTM (compJacTMatVec.jl:309,315)
        if (prof == 0) fout = v.bcsL + (long)s * v.nz;
        else if (prof == 1) fout = v.bcsR + (long)s * v.nz;
        else { fout = v.bcsB + s; fstride = 0; }          // only the bottom value of the mean profile
    }
    v.sensDead[sp] = sens_profile(v.omega[s], v.nz, v.zLen, tm, T, T + n1, T + 2 * n1, T + 3 * n1, T + 4 * n1,
                                  v.sensEu + sp * n1, v.sensEd + sp * n1, v.sensMix + sp * 4 * v.nz,
                                  v.sensDz1 + sp * v.nz, v.sensZ1 + sp, fout, fstride);
}
// dBC^T w, one derivative column c of one profile
HD void item_bcsens(const View& v, int s, int prof, int c) {
    const long o = (long)s * v.nz + c;
    if (!v.sysOn[s]) {
        if (prof == 0) v.gL[o] = cplx{0, 0}; else if (prof == 1) v.gR[o] = cplx{0, 0}; else v.gMn[o] = cplx{0, 0};
        return;
    }
    const bool tm = s >= v.nFreq;
    const long n1 = v.nz + 1, sp = (long)s * 3 + prof;
    const cplx* T = v.sensTab + sp * 5 * n1;
    const cplx* w = prof == 0 ? v.wL + (long)s * v.nz : (prof == 1 ? v.wR + (long)s * v.nz : nullptr);
    const cplx g = bc1d_sens_column(v.omega[s], v.nz, v.zLen, tm, c, T, T + n1, T + 2 * n1, T + 3 * n1,
                                    v.sensEu + sp * n1, v.sensEd + sp * n1, v.sensMix + sp * 4 * v.nz,
                                    v.sensDz1 + sp * v.nz, v.sensZ1[sp], v.sensDead[sp], w, 1);
    if (prof == 0) v.gL[o] = g; else if (prof == 1) v.gR[o] = g; else v.gMn[o] = g;
}

// The same in two steps, so that the serial recurrences are off the critical path (they depend on sigma only):
//   item_bcsens_pre       side stream, beside the solves: the w-independent entries dF(row, c) of the left / right
//                         profile into v.dBC (the mean profile needs its last row only: v.gMn directly)
//   item_bcsens_contract  after the adjoint solve: g[c] = sum over rows of dF(row, c) w[row], rows in the order of
//                         item_bcsens' accumulation (the rows beyond the cut-off hold zeros)
HD void item_bcsens_pre(const View& v, int s, int prof, int c) {
    const long o = (long)s * v.nz + c;
    if (!v.sysOn[s]) { if (prof == 2) v.gMn[o] = cplx{0, 0}; return; }
    const bool tm = s >= v.nFreq;
    const long n1 = v.nz + 1, sp = (long)s * 3 + prof;
    const cplx* T = v.sensTab + sp * 5 * n1;
    cplx* out = prof < 2 ? v.dBC + ((long)s * 2 + prof) * v.nz * v.nz + c : nullptr;
    const cplx g = bc1d_sens_column(v.omega[s], v.nz, v.zLen, tm, c, T, T + n1, T + 2 * n1, T + 3 * n1,
                                    v.sensEu + sp * n1, v.sensEd + sp * n1, v.sensMix + sp * 4 * v.nz,
                                    v.sensDz1 + sp * v.nz, v.sensZ1[sp], v.sensDead[sp], nullptr, 1, out, v.nz);
    if (prof == 2) v.gMn[o] = g;
}
HD void item_bcsens_contract(const View& v, int s, int prof, int c) {     // prof 0 / 1
    const long o = (long)s * v.nz + c;
    cplx acc = cplx{0.0, 0.0};
    if (v.sysOn[s]) {
        const cplx* D = v.dBC + ((long)s * 2 + prof) * v.nz * v.nz + c;
        const cplx* w = (prof == 0 ? v.wL : v.wR) + (long)s * v.nz;
        // (batches of 8 rows requested together; the additions stay in row order)
        int j = 0;
        for (; j + 8 <= v.nz; j += 8) {
            cplx d[8], ww[8];
            HMCMT_UNROLL
            for (int t = 0; t < 8; ++t) { d[t] = D[(long)(j + t) * v.nz]; ww[t] = w[j + t]; }
            HMCMT_UNROLL
            for (int t = 0; t < 8; ++t) acc += d[t] * ww[t];
        }
        for (; j < v.nz; ++j) acc += D[(long)j * v.nz] * w[j];
    }
    if (prof == 0) v.gL[o] = acc; else v.gR[o] = acc;
}

// --- TM field with the sensitivity-version boundary values (compJacTMatVec.jl:307,315):
//     h~ = forward solution on interior nodes, getBCderivTM's bc on boundary nodes
HD cplx tm_field_sens(const View& v, int s, int iy, int iz) {
    if (iz == 0) return cplx{1.0, 0.0};
    if (iy == 0) return v.bcsL[(long)s * v.nz + iz - 1];
    if (iy == v.ny) return v.bcsR[(long)s * v.nz + iz - 1];
    if (iz == v.nz) return v.bcsB[s];
    return v.X[(long)s * v.vstride + nidx(v, iy, iz)];
}

// --- P-terms of J^T v for one cell, summed over the frequencies of one mode
HD double gradcell_freqs(const View& v, int mode, int cell, int f0, int f1) {
    const int ky = cell % v.ny, kz = cell / v.ny;
    const double area = v.yLen[ky] * v.zLen[kz];
    double acc = 0.0;
#pragma unroll 4
    for (int f = f0; f < f1; ++f) {
        const int s = mode * v.nFreq + f;
        if (!v.sysOn[s]) continue;
        const cplx* L = v.Lam + (long)s * v.vstride;
        if (mode == 0) {
            // -i w (1/4 area) sum over the 4 corner nodes e*lambda (compJacTMatVec.jl:83,235)
            const cplx* E = v.X + (long)s * v.vstride;
            cplx sum = cplx{0, 0};
            for (int dz = 0; dz < 2; ++dz)
                for (int dy = 0; dy < 2; ++dy) {
                    long n = nidx(v, ky + dy, kz + dz);
                    sum += E[n] * L[n];
                }
            // Re[-i w a sum] = w a Im(sum)
            acc += v.omega[s] * 0.25 * area * sum.im;
        } else {
            // (area/sig^2) * 1/2 * sum over the 4 edges (grad h~)(grad lambda)
            // (compJacTMatVec.jl:97-99,306-307,314-315); mesh-boundary edges have grad lambda = 0
            cplx h00 = tm_field_sens(v, s, ky, kz), h10 = tm_field_sens(v, s, ky + 1, kz);
            cplx h01 = tm_field_sens(v, s, ky, kz + 1), h11 = tm_field_sens(v, s, ky + 1, kz + 1);
            cplx l00 = L[nidx(v, ky, kz)], l10 = L[nidx(v, ky + 1, kz)];
            cplx l01 = L[nidx(v, ky, kz + 1)], l11 = L[nidx(v, ky + 1, kz + 1)];
            const double iy2 = 1.0 / (v.yLen[ky] * v.yLen[ky]), iz2 = 1.0 / (v.zLen[kz] * v.zLen[kz]);
            cplx sum = ((h10 - h00) * (l10 - l00) + (h11 - h01) * (l11 - l01)) * iy2 +
                       ((h01 - h00) * (l01 - l00) + (h11 - h10) * (l11 - l10)) * iz2;
            const double sg = v.sigma[cell];
            acc += 0.5 * area / (sg * sg) * sum.re;
        }
    }
    return acc;
}
HD void item_gradcell(const View& v, int mode, int cell) {
    v.gPart[(long)mode * v.nCell + cell] = gradcell_freqs(v, mode, cell, 0, v.nFreq);
}
// the same over one of GRAD_NG groups of frequencies (the GPU's launch: 4x the threads of a latency-bound kernel);
// partial sums [mode][group][cell], added up by the final assembly
constexpr int GRAD_NG = 4;
HD void item_gradcell_group(const View& v, int mode, int grp, int cell) {
    const int per = (v.nFreq + GRAD_NG - 1) / GRAD_NG, f0 = grp * per, f1 = f0 + per < v.nFreq ? f0 + per : v.nFreq;
    v.gPartG[((long)mode * GRAD_NG + grp) * v.nCell + cell] = gradcell_freqs(v, mode, cell, f0, f1);
}

// --- Q-term of one system for one receiver-layer cell: Re sum_r conj(v_r) dZ_r/dsigma_c
//     (compJacTMatVec.jl:209, :280)
HD void item_qterm(const View& v, int s, int ky) {
    double g = 0.0;
    if (v.sysOn[s])
        for (int r = 0; r < v.nRx; ++r) {
            const long k = (long)s * v.nRx + r;
            const int o = ky - v.rxN0[k];
            if (o >= 0 && o < 3) g += (v.rxCoef[k] * v.rxD[k * 11 + 8 + o]).re;
        }
    v.qPart[(long)s * v.ny + ky] = g;
}

// --- final assembly of the gradient w.r.t. m = ln(sigma) for one active cell:
//     P-terms + boundary terms + Q-terms, real part, chain rule (compJacTMatVec.jl:244,318,325-327;
//     HMCSampler.jl:306)
// boundary term of one system for one cell (branch-free select, not `continue`, so that the loads of several systems
// are in flight)
HD double gradfinal_sys(const View& v, int s, int ky, int kz) {
    if (v.dbg & 2) return 0.0;
    const long o = (long)s * v.nz + kz;
    cplx b = v.gMn[o] * v.colw[(long)s * v.ny + ky];
    if (ky == 0) b += v.gL[o];
    if (ky == v.ny - 1) b += v.gR[o];
    return v.sysOn[s] ? b.re : 0.0;
}
HD void item_gradfinal(const View& v, int a) {
    const int cell = v.act[a];
    const int ky = cell % v.ny, kz = cell / v.ny;
    double g = v.gPart[cell] + v.gPart[(long)v.nCell + cell];
    // branch-free over the systems (select, not `continue`) so that the loads of several systems are in flight
#pragma unroll 8
    for (int s = 0; s < v.S; ++s) g += gradfinal_sys(v, s, ky, kz);
    if (kz == v.zid)
        for (int s = 0; s < v.S; ++s) g += v.qPart[(long)s * v.ny + ky];
    v.grad[a] = exp(v.m[a]) * g;
}

// --- one entry of the explicit Jacobian by the adjoint route (compJacTMat.jl; J itself: compJacMat.jl:206-314):
//     dZ/dsigma of cell (ky, kz) for system s, where v.Lam is the solution for ONE receiver's functional row as the
//     source (unit coefficient) and srcB / colw / gL / gR are that solve's boundary arrays.  The terms of
//     gradcell_freqs + gradfinal_sys + item_qterm for one system, kept complex: P-term, boundary term, Q-term (qJ:
//     [S][ny] complex, the receiver layer's cells only).
HD cplx jac_cell(const View& v, int s, int ky, int kz, const cplx* qJ) {
    const double area = v.yLen[ky] * v.zLen[kz];
    const cplx* L = v.Lam + (long)s * v.vstride;
    cplx j;
    if (s < v.nFreq) {
        // -i w (1/4 area) sum over the 4 corner nodes e*lambda
        const cplx* E = v.X + (long)s * v.vstride;
        cplx sum = cplx{0, 0};
        for (int dz = 0; dz < 2; ++dz)
            for (int dy = 0; dy < 2; ++dy) {
                long n = nidx(v, ky + dy, kz + dz);
                sum += E[n] * L[n];
            }
        const double f = v.omega[s] * 0.25 * area;
        j = cplx{f * sum.im, -(f * sum.re)};
    } else {
        cplx h00 = tm_field_sens(v, s, ky, kz), h10 = tm_field_sens(v, s, ky + 1, kz);
        cplx h01 = tm_field_sens(v, s, ky, kz + 1), h11 = tm_field_sens(v, s, ky + 1, kz + 1);
        cplx l00 = L[nidx(v, ky, kz)], l10 = L[nidx(v, ky + 1, kz)];
        cplx l01 = L[nidx(v, ky, kz + 1)], l11 = L[nidx(v, ky + 1, kz + 1)];
        const double iy2 = 1.0 / (v.yLen[ky] * v.yLen[ky]), iz2 = 1.0 / (v.zLen[kz] * v.zLen[kz]);
        cplx sum = ((h10 - h00) * (l10 - l00) + (h11 - h01) * (l11 - l01)) * iy2 +
                   ((h01 - h00) * (l01 - l00) + (h11 - h10) * (l11 - l10)) * iz2;
        const double sg = v.sigma[(long)kz * v.ny + ky];
        j = (0.5 * area / (sg * sg)) * sum;
    }
    const long o = (long)s * v.nz + kz;
    j += v.gMn[o] * v.colw[(long)s * v.ny + ky];
    if (ky == 0) j += v.gL[o];
    if (ky == v.ny - 1) j += v.gR[o];
    if (kz == v.zid) j += qJ[(long)s * v.ny + ky];
    return j;
}
// --- the datum's row from the impedance's (item_resid's data kinds): 0 impedance dZ; 1 apparent resistivity
//     (2/(w mu0)) Re(conj(Z) dZ); 2 phase in degrees (180/pi) Im(conj(Z) dZ)/|Z|^2 -- real for kinds 1, 2.  For a tipper
//     functional dz is dT: 3 TZY dT, 4 Re dT, 5 Im dT
HD cplx jac_datum(int kind, cplx z, double omega, cplx dz) {
    if (kind == 0 || kind == 3) return dz;
    if (kind == 4) return cplx{dz.re, 0.0};
    if (kind == 5) return cplx{dz.im, 0.0};
    const cplx c = conj(z) * dz;
    if (kind == 1) return cplx{(2.0 / (omega * MU0)) * c.re, 0.0};
    return cplx{(180.0 / 3.14159265358979323846) * c.im / cabs2(z), 0.0};
}

// ==============================================================================================
// Tangent-linear route J v (compJacMat.jl:206-314 applied to a vector): the exact transposes of jac_cell's P-term,
// item_wside / item_colw + item_bcsens_contract + gradfinal_sys (boundary terms) and item_src / item_qterm (data side).
// ==============================================================================================
// --- delta sigma on every cell from v on the active cells: wrt 0 d sigma = v, 1 d sigma = exp(m) v (m = ln sigma)
HD void item_dsigma(const View& v, int cell, int wrt) {
    const int a = v.cell2act[cell];
    double d = 0.0;
    if (a >= 0) d = wrt ? exp(v.m[a]) * v.tanV[a] : v.tanV[a];
    v.dSig[cell] = d;
}
// --- tangent of the boundary values, dbc = dBC dsigma (MT1DSensitivity.jl:272-328): one term of the sum over the layers c
//     side node iz (1..nz) of profile prof (0 left, 1 right): row iz-1 of v.dBC times dsigma of the first / last cell column
HD cplx dbc_side_term(const View& v, int s, int prof, int iz, int c) {
    const cplx d = v.dBC[(((long)s * 2 + prof) * v.nz + (iz - 1)) * v.nz + c];
    return v.dSig[(long)c * v.ny + (prof ? v.ny - 1 : 0)] * d;
}
//     bottom node iy (1..ny-1): the mean profile's last row times the width-weighted dsigma of the two columns beside the node
//     (the transpose of item_colw, MT1DSensitivity.jl:315-328)
HD cplx dbc_bottom_term(const View& v, int s, int iy, int c) {
    const double ya = v.yLen[iy - 1], yb = v.yLen[iy];
    const double ds = (ya / (ya + yb)) * v.dSig[(long)c * v.ny + iy - 1] + (yb / (ya + yb)) * v.dSig[(long)c * v.ny + iy];
    return ds * v.gMn[(long)s * v.nz + c];
}
// (serial forms, layers in order: the host instantiation; the GPU kernel spreads a row over a wavefront)
HD void item_dbc_side(const View& v, int s, int prof, int iz) {
    cplx acc = cplx{0, 0};
    if (v.sysOn[s])
        for (int c = 0; c < v.nz; ++c) acc += dbc_side_term(v, s, prof, iz, c);
    (prof ? v.dbcR : v.dbcL)[(long)s * v.nz + iz - 1] = acc;
}
HD void item_dbc_bottom(const View& v, int s, int iy) {
    cplx acc = cplx{0, 0};
    if (v.sysOn[s])
        for (int c = 0; c < v.nz; ++c) acc += dbc_bottom_term(v, s, iy, c);
    v.dbcB[(long)s * (v.ny + 1) + iy] = acc;
}
// tangent of the Dirichlet value at a boundary node: top row 0, corners with the sides
HD cplx dbc_at(const View& v, int s, int iy, int iz) {
    if (iz == 0) return cplx{0, 0};
    if (iy == 0) return v.dbcL[(long)s * v.nz + iz - 1];
    if (iy == v.ny) return v.dbcR[(long)s * v.nz + iz - 1];
    if (iz == v.nz) return v.dbcB[(long)s * (v.ny + 1) + iy];
    return cplx{0, 0};
}
// --- tangent right-hand side b = -(dA/dsigma . dsigma) F - Aio dbc at one node of the padded grid (zero off the interior):
//     TE  -i w e_n 1/4 sum over the 4 cells around n of area_c dsigma_c                 (jac_cell's TE term, transposed)
//     TM  sum over the 4 cells c around n of (1/2 area_c dsigma_c / sigma_c^2) ((h~_n - h~_y)/dy_c^2 + (h~_n - h~_z)/dz_c^2),
//         h~_y / h~_z the cell's other node on n's row / column, h~ = tm_field_sens    (jac_cell's TM term, transposed)
//     and -c_{n->b} dbc_b for the Dirichlet neighbours b of n (item_rhs with dbc for the boundary values)
HD cplx tangent_rhs(const View& v, int s, int iy, int iz) {
    const bool interior = iz >= 1 && iz <= v.nz - 1 && iy >= 1 && iy <= v.ny - 1;
    if (!interior || !v.sysOn[s]) return cplx{0, 0};
    cplx b = cplx{0, 0};
    if (s < v.nFreq) {
        double q = 0.0;
        for (int dz = -1; dz <= 0; ++dz)
            for (int dy = -1; dy <= 0; ++dy)
                q += v.yLen[iy + dy] * v.zLen[iz + dz] * v.dSig[(long)(iz + dz) * v.ny + iy + dy];
        const cplx e = v.X[(long)s * v.vstride + nidx(v, iy, iz)];
        const double f = v.omega[s] * 0.25 * q;
        b = cplx{f * e.im, -(f * e.re)};
    } else {
        const cplx hn = tm_field_sens(v, s, iy, iz);
        for (int dz = -1; dz <= 0; ++dz)
            for (int dy = -1; dy <= 0; ++dy) {
                const int ky = iy + dy, kz = iz + dz;
                const double ly = v.yLen[ky], lz = v.zLen[kz], sg = v.sigma[(long)kz * v.ny + ky];
                const cplx hy = tm_field_sens(v, s, dy ? iy - 1 : iy + 1, iz), hz = tm_field_sens(v, s, iy, dz ? iz - 1 : iz + 1);
                const double w = 0.5 * ly * lz * v.dSig[(long)kz * v.ny + ky] / (sg * sg);
                b += w * ((hn - hy) * (1.0 / (ly * ly)) + (hn - hz) * (1.0 / (lz * lz)));
            }
    }
    const int mode = s >= v.nFreq;
    const long mo = (long)mode * v.vstride, n = nidx(v, iy, iz);
    cplx acc = cplx{0, 0};
    if (iy == v.ny - 1) acc += v.cY[mo + n] * dbc_at(v, s, v.ny, iz);
    if (iy == 1) acc += v.cY[mo + n - 1] * dbc_at(v, s, 0, iz);
    if (iz == v.nz - 1) acc += v.cZ[mo + n] * dbc_at(v, s, iy, v.nz);
    return b - acc;
}
HD void item_tangent_rhs(const View& v, int s, int iy, int iz) {
    v.R[(long)s * v.vstride + nidx(v, iy, iz)] = iy <= v.ny ? tangent_rhs(v, s, iy, iz) : cplx{0, 0};
}
// --- data side: dZ of functional r of system s (item_src / item_qterm transposed; the tangent field on the side nodes
//     iy = 0, ny is dbc -- the srcB positions), then every datum of (s, r) by jac_datum, scattered to data order
HD cplx tangent_field_at(const View& v, int s, int iy, int iz) {
    const bool interior = iz >= 1 && iz <= v.nz - 1 && iy >= 1 && iy <= v.ny - 1;
    if (interior) return v.dF[(long)s * v.vstride + nidx(v, iy, iz)];
    if (iz >= 1 && (iy == 0 || iy == v.ny)) return dbc_at(v, s, iy, iz);
    return cplx{0, 0};
}
HD cplx tangent_dz(const View& v, int s, int r) {
    const long k = (long)s * v.nRx + r;
    const int n0 = v.rxN0[k];
    const cplx* D = v.rxD + k * 11;
    cplx acc = cplx{0, 0};
    for (int row = 0; row < 2; ++row)
        for (int o = 0; o < 4; ++o) {
            const int iy = n0 + o;
            if (iy >= 0 && iy <= v.ny) acc += D[row * 4 + o] * tangent_field_at(v, s, iy, v.zid + row);
        }
    for (int o = 0; o < 3; ++o) {
        const int ky = n0 + o;
        if (ky >= 0 && ky < v.ny) acc += v.dSig[(long)v.zid * v.ny + ky] * D[8 + o];
    }
    return acc;
}
HD void item_tangent_data(const View& v, int s, int r) {
    if (!v.sysOn[s]) return;
    const long k = (long)s * v.nRx + r;
    if (v.srStart[k] == v.srStart[k + 1]) return;
    const double up = v.tanScale ? v.tanScale[1] : 1.0;       // (the solve ran on 2^-e dsigma: exact in binary, undone here)
    const cplx dz = up * tangent_dz(v, s, r), z = v.Zrx[k];
    for (int t = v.srStart[k]; t < v.srStart[k + 1]; ++t) {
        const int p = v.srList[t];
        v.jv[p] = jac_datum(v.datKind[p], z, v.omega[s], dz);
    }
}
// --- J^T u for a free data vector u (compJacTMatVec.jl:8 with datVec = u): item_resid's vbar with u in the place of
//     W^T W (pred - obs); Re(vbar dZ) is the datum's term of Re(J^T conj(u))
HD void item_vbar_free(const View& v, int p) {
    const cplx wr = v.uData[p];
    const int dk = v.datKind[p];
    if (dk == 0 || dk == 3) { v.vbar[p] = conj(wr); return; }
    if (dk == 4) { v.vbar[p] = cplx{wr.re, 0.0}; return; }
    if (dk == 5) { v.vbar[p] = cplx{0.0, -wr.re}; return; }
    const int sd = v.datSys[p];
    const cplx zs = v.Zrx[(long)sd * v.nRx + v.datRx[p]];
    if (dk == 1) v.vbar[p] = (wr.re * 2.0 / (v.omega[sd] * MU0)) * conj(zs);
    else {
        const cplx c = conj(zs);
        v.vbar[p] = (wr.re * (180.0 / 3.14159265358979323846) / cabs2(zs)) * cplx{c.im, -c.re};
    }
}
// --- final assembly of J^T u for one active cell: item_gradfinal without the residual's chain rule unless wrt = ln sigma
HD double jtvp_cell(const View& v, int a, int wrt, const double* gPartG, int ngroups, double up = 1.0) {
    const int cell = v.act[a];
    const int ky = cell % v.ny, kz = cell / v.ny;
    double g = 0.0;
    for (int q = 0; q < ngroups; ++q) g += gPartG[(long)q * v.nCell + cell];
    for (int s = 0; s < v.S; ++s) g += gradfinal_sys(v, s, ky, kz);
    if (kz == v.zid)
        for (int s = 0; s < v.S; ++s) g += v.qPart[(long)s * v.ny + ky];
    g *= up;                                                  // (up: the power of two vbar was normalised by, undone)
    return wrt ? exp(v.m[a]) * g : g;
}

// ----------------------------------------------------------------------------------------------
// the device-resident HMC chain (hmcmt_chain_*, kernels_chain.h): per-parameter bodies
// ----------------------------------------------------------------------------------------------
// The reductions keep the leapfrog kernels' layout: CHAIN_NB workgroups of CHAIN_NT threads, parameter a belongs to partial sum
// chain_part_of(a); the partial sums are added in index order (item_chain_total), so the bits repeat.
constexpr int CHAIN_NB = 64;       // == LFNB (kernels_path.h)
constexpr int CHAIN_NT = 256;
constexpr double CHAIN_ZCLIP = 2.5;   // getMomentumVector clips the normals at +-2.5 (HMCSampler.jl:444-447)
HD int chain_part_of(int a) { return (a / CHAIN_NT) % CHAIN_NB; }
// momentum of parameter a for the diagonal mass: p = sqrtM * clip(z) = clip(z) / sqrt(invM); returns its term of p' M^-1 p
HD double chain_clip(double zc) { return zc > CHAIN_ZCLIP ? CHAIN_ZCLIP : (zc < -CHAIN_ZCLIP ? -CHAIN_ZCLIP : zc); }
// ... from the clipped normal zc (shared with the seeded draw, item_chain_draw_momentum: the same operations, so the same bits)
HD double chain_momentum_of(double zc, const double* invM, double* p, int a) {
    const double pa = zc / sqrt(invM[a]);
    p[a] = pa;
    return pa * (invM[a] * pa);
}
HD double item_chain_momentum(const double* z, const double* invM, double* p, int a) { return chain_momentum_of(chain_clip(z[a]), invM, p, a); }
HD double item_chain_clip(const double* z, int a) { return chain_clip(z[a]); }
// parameter a's term of p' M^-1 p: x = M^-1 p given (M = Wm, from the mass solve), or the diagonal invM
HD double item_chain_kinetic(const double* p, const double* x, const double* invM, int a) {
    return x ? p[a] * x[a] : p[a] * (invM[a] * p[a]);
}
// the final stage of a reduction: the partial sums in index order
HD double item_chain_total(const double* part) {
    double acc = 0.0;
    for (int b = 0; b < CHAIN_NB; ++b) acc += part[b];
    return acc;
}
// The chain's own random numbers (hmcmt_chain_seed, hmcmt_chain_sample; hmcmt_rng_* are these functions on the host): Philox4x32-10
// (Salmon, Moraes, Dror, Shaw, SC'11), a counter-based generator -- a draw is a pure function of (seed, stream, t, c0), so a chain's
// generator state is three integers and any host reproduces it.
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (c0, stream, t & 0xffffffff, t >> 32)   t: the draw's index, one per sample from 0; stream: the chain's number
//   c0      = the active-cell index a for the momentum's normal of cell a; RNG_C0_SCALARS for the sample's L and u.  nAC is an int32,
//             so a cell index never reaches 0xFFFFFFFF and the two kinds of block never meet.
constexpr uint32_t RNG_C0_SCALARS = 0xFFFFFFFFu;
// one block: ten rounds of two plain 32 x 32 -> 64 products, the key stepped by the Weyl constants behind each round
HD void item_philox4x32(const uint32_t* c, const uint32_t* k, uint32_t* out) {
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0;
        c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
HD void item_rng_block(uint64_t seed, uint32_t stream, uint64_t t, uint32_t c0, uint32_t* out) {
    const uint32_t c[4] = {c0, stream, (uint32_t)t, (uint32_t)(t >> 32)}, k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    item_philox4x32(c, k, out);
}
// a uniform from the upper 26 bits of two words: U = (2 k + 1) 2^-53 with the 52-bit k -- exact in fp64 and strictly inside (0, 1),
// so that log never sees 0
HD double item_rng_u52(uint32_t hi, uint32_t lo) {
    const uint64_t k = ((uint64_t)(hi >> 6) << 26) | (uint64_t)(lo >> 6);
    return (double)(2 * k + 1) * 0x1p-53;
}
// the standard normal of cell a in draw t: ONE block per cell and the cosine branch of Box-Muller (the sine is discarded on purpose:
// a thread owns a cell as in k_chain_momentum, so the partial sums of K0 keep their order); |z| <= sqrt(2 * 53 ln 2) = 8.57
HD double item_rng_normal(uint64_t seed, uint32_t stream, uint64_t t, int a) {
    uint32_t x[4];
    item_rng_block(seed, stream, t, (uint32_t)a, x);
    const double u1 = item_rng_u52(x[0], x[1]), u2 = item_rng_u52(x[2], x[3]);
    const double r = sqrt(-2.0 * log(u1)), c = cos(TWO_PI * u2);
    return r * c;
}
// the scalars of draw t: the accept test's uniform u and the trajectory length L in Lmin .. Lmax by multiply-shift of one word --
// value v has probability floor or ceil of 2^32 / span over 2^32 with span = Lmax - Lmin + 1, a bias of at most span / 2^32
HD void item_rng_scalars(uint64_t seed, uint32_t stream, uint64_t t, int Lmin, int Lmax, int* L, double* u) {
    uint32_t x[4];
    item_rng_block(seed, stream, t, RNG_C0_SCALARS, x);
    *u = item_rng_u52(x[0], x[1]);
    *L = Lmin + (int)(((uint64_t)x[2] * (uint64_t)((int64_t)Lmax - (int64_t)Lmin + 1)) >> 32);
}
// the seeded draw of cell a: the clipped normal, and for the diagonal mass item_chain_momentum behind it
HD double item_chain_draw_clip(uint64_t seed, uint32_t stream, uint64_t t, int a) { return chain_clip(item_rng_normal(seed, stream, t, a)); }
HD double item_chain_draw_momentum(uint64_t seed, uint32_t stream, uint64_t t, const double* invM, double* p, int a) {
    return chain_momentum_of(item_chain_draw_clip(seed, stream, t, a), invM, p, a);
}
// Welford's update of the running mean and the sum of squared deviations with sample m; count includes this sample.
// A cell that holds the same value in every sample keeps m2 == 0 exactly (d == 0 from the second sample on; the first
// sample gives mean = m, m - mean = 0).
HD void item_chain_welford(const double* m, double* mean, double* m2, double count, int a) {
    const double x = m[a], d = x - mean[a];
    const double mu = mean[a] + d / count;
    mean[a] = mu;
    m2[a] += d * (x - mu);
}
// Warm-up adaptation (hmcmt_chain_adapt_*, include/hmcmt.h has the semantics).  The dual averaging of the step size (Nesterov's, in
// Stan's form) is scalar host work in double; the window's variance is item_chain_welford on the window's own buffers, and
// item_adapt_mass turns it into the diagonal of M^-1.  x = ln dt throughout.
struct AdaptDA {
    double mu = 0, s_bar = 0, x_bar = 0, x = 0;
    long long t = 0;               // updates since the last restart
};
// a restart around the step size dt: at the begin call and behind every mass update
HD void item_adapt_restart(AdaptDA& d, double dt) {
    d.mu = log(10.0 * dt);
    d.s_bar = d.x_bar = 0.0;
    d.x = log(dt);
    d.t = 0;
}
// one update with the acceptance probability alpha of the step just decided, in exactly this order; returns x
HD double item_adapt_update(AdaptDA& d, double alpha, double delta, double gamma, double t0, double kappa) {
    d.t += 1;
    const double t = (double)d.t;
    const double eta = 1.0 / (t + t0);
    d.s_bar = (1.0 - eta) * d.s_bar + eta * (delta - alpha);
    d.x = d.mu - d.s_bar * sqrt(t) / gamma;
    const double x_eta = pow(t, -kappa);
    d.x_bar = (1.0 - x_eta) * d.x_bar + x_eta * d.x;
    return d.x;
}
// dt = exp(x) clipped into [dt_min, dt_max] where set (0: no bound on that side); x is held to +-700 first, so that dt and 10 dt
// stay finite and positive whatever the acceptances were
HD double item_adapt_dt(double x, double dt_min, double dt_max) {
    double dt = exp(x > 700.0 ? 700.0 : (x < -700.0 ? -700.0 : x));
    if (dt_min > 0.0 && dt < dt_min) dt = dt_min;
    if (dt_max > 0.0 && dt > dt_max) dt = dt_max;
    return dt;
}
// Stan's window schedule, steps counted from 0.  The first window ends at step init + base - 1 (*size = base).  `end` is the step whose
// window just closed and *size that window's length: returns the step the next window ends at and doubles *size, or -1 when `end` was
// the last one, W - term - 1.  A window that would leave less than its own double in front of the terminal buffer runs up to it.
HD long long item_adapt_next_window(long long end, long long* size, long long W, long long term) {
    const long long last = W - term - 1;
    if (end == last) return -1;
    *size *= 2;
    long long next = end + *size;
    if (next != last && next + 2 * *size >= W - term) next = last;
    return next;
}
// cell a's entry of diag(M^-1) from a window of n >= 2 samples: the sample variance m2 / (n - 1) shrunk towards 1e-3;
// nm1 = n - 1, w = n / (n + 5) and f = 1e-3 * 5 / (n + 5) are formed by the caller as doubles.  m2 == 0 gives f exactly.
HD double item_adapt_mass(const double* m2, double nm1, double w, double f, int a) {
    return (m2[a] / nm1) * w + f;
}
// Histograms of the committed models (hmcmt_chain_hist_*).  The counters lie BIN-MAJOR, counts[b * ntarget + r]: row r belongs to
// thread r alone, and the rows of a wavefront -- neighbouring cells, whose values fall into the same or adjacent bins -- touch a few
// cache lines per commit where a target-major array would touch one line per lane; the quantile scan reads the same way.
constexpr int CHAIN_HIST_MAXBINS = 4096;
// the bin of value m: one subtraction, then one product (nothing to contract), clamped into the edge bins
HD int item_chain_hist_bin(double m, double lo, double scale, int nbins) {
    const double t = (m - lo) * scale;
    return t < 0 ? 0 : (t >= (double)nbins ? nbins - 1 : (int)t);
}
HD void item_chain_hist(const double* m, const long long* target, unsigned int* counts, long long ntarget, int nbins, double lo,
                        double scale, long long r) {
    const int b = item_chain_hist_bin(m[target[r]], lo, scale, nbins);
    counts[(long long)b * ntarget + r] += 1u;
}
// the x-th sample of row r, x = q * N in [0, N], linear inside its bin: the first bin with count_b > 0 and cum_b >= x.  *bin: that bin
HD double item_chain_quantile(const unsigned int* counts, long long ntarget, int nbins, double lo, double w, double x, long long r,
                              int* bin) {
    unsigned long long cum = 0;
    int b = 0, last = -1;
    unsigned long long cumLast = 0;
    for (; b < nbins; ++b) {
        const unsigned int c = counts[(long long)b * ntarget + r];
        if (c == 0) continue;
        if ((double)(cum + c) >= x) break;
        last = b; cumLast = cum;
        cum += c;
    }
    if (b == nbins) {                 // (x beyond the row's sum: cannot happen for q <= 1 -- the last occupied bin then)
        if (last < 0) { *bin = -1; return lo; }
        b = last; cum = cumLast;
    }
    *bin = b;
    const double c = (double)counts[(long long)b * ntarget + r];
    return lo + w * ((double)b + (x - (double)cum) / c);
}
// Lagged autocovariances of the committed models (hmcmt_chain_acov_*).  Every array with a lag or a ring slot lies LAG-MAJOR,
// a[k * ntarget + j]: the lanes of a wavefront are neighbouring targets j of one lag and touch adjacent doubles.  Counted commits are
// t = 0, 1, ...; y_t = m[target] - x0 with x0 the value at t = 0 (one subtraction).  Per target: tot = sum y_t (serial adds),
// S_k = sum_{t >= k} fma(y_t, y_{t-k}, .), H_k = sum_{t < k} y_t, and a ring of K + 1 slots, slot t mod (K + 1) = y_t: the slot written
// at commit t held y_{t-K-1}, which no lag of this commit reads.
constexpr int CHAIN_ACOV_MAXLAG = 1023;
constexpr int CHAIN_ACOV_RUN = 8;     // lags per thread of k_chain_acov: y_t, the pivot and the ring index stay in registers
// commit t of target j for the lags k0 <= k < k1 (k1 <= K + 1); target == nullptr: row j is cell j.  The owner of lag 0 also owns
// x0, tot and the ring slot of this commit; at t = 0 nobody reads x0 (y_0 = 0 by definition).
HD void item_chain_acov(const double* m, const long long* target, double* x0, double* tot, double* S, double* H, double* ring,
                        long long ntarget, int K, long long t, long long j, int k0, int k1) {
    const double x = m[target ? target[j] : j];
    const double y = t == 0 ? 0.0 : x - x0[j];
    const int nslot = K + 1;
    int slot = (int)((t + nslot - (k0 % nslot)) % nslot);          // slot of y_{t-k0}
    for (int k = k0; k < k1; ++k) {
        const long long i = (long long)k * ntarget + j;
        if (k == 0) {
            if (t == 0) x0[j] = x;
            tot[j] += y;
            ring[(long long)slot * ntarget + j] = y;
            S[i] = fma(y, y, S[i]);
        } else if (t >= k) {
            S[i] = fma(y, ring[(long long)slot * ntarget + j], S[i]);
        } else {
            H[i] += y;                                             // (t < k: y_t is one of the first k samples)
        }
        slot = slot == 0 ? K : slot - 1;
    }
}
// c_k, k = 0 .. K, of target j from the state after N >= 1 commits, and mean = x0 + ybar (each output may be nullptr): the owner of
// the target walks its lags with T_k, the sum of the last k samples, running newest first from the ring: T_k = T_{k-1} + y_{N-k}.
HD void item_chain_acov_out(const double* x0, const double* tot, const double* S, const double* H, const double* ring, long long ntarget,
                            int K, long long N, long long j, double* mean, double* acov) {
    const double tt = tot[j], ybar = tt / (double)N;
    if (mean) mean[j] = x0[j] + ybar;
    if (!acov) return;
    int slot = (int)((N - 1) % (K + 1));                           // slot of y_{N-1}
    double T = 0.0;
    for (int k = 0; k <= K; ++k) {
        const long long i = (long long)k * ntarget + j;
        if (k >= N) { acov[i] = 0.0; continue; }
        if (k > 0) {
            T += ring[(long long)slot * ntarget + j];
            slot = slot == 0 ? K : slot - 1;
        }
        const double A = tt - H[i], B = tt - T;
        acov[i] = (S[i] - ybar * (A + B) + (double)(N - k) * (ybar * ybar)) / (double)N;
    }
}
// Geyer's initial positive sequence on acov[(K + 1)][ntarget] of N >= 1 commits: Gamma_m = (c_2m + c_2m+1) / c_0 summed while > 0;
// tau = -1 + 2 sum; window = +pairs summed if a non-positive pair ended the sum, -pairs if the lags ran out.  cap = N max(1, log10 N)
// and capTau = 1 / max(1, log10 N) come from the host (one log10 for all targets).  Each of tau, ess, window may be nullptr.
HD void item_chain_ess(const double* acov, long long ntarget, int K, long long N, double cap, double capTau, long long j, double* tau,
                       double* ess, int* window) {
    const double c0 = acov[j];
    double t, e;
    int w;
    if (!(c0 > 0.0)) {                                             // a constant cell
        t = (double)N; e = 1.0; w = 0;
    } else {
        const int kmax = (int)(N - 1 < (long long)K ? N - 1 : (long long)K);
        const int npairs = kmax >= 1 ? (kmax - 1) / 2 + 1 : 0;
        double sum = 0.0;
        int M = 0;
        bool ended = false;
        for (int p = 0; p < npairs; ++p) {
            const double G = (acov[(long long)(2 * p) * ntarget + j] + acov[(long long)(2 * p + 1) * ntarget + j]) / c0;
            if (!(G > 0.0)) { ended = true; break; }
            sum += G;
            ++M;
        }
        t = -1.0 + 2.0 * sum;
        w = ended ? M : -M;
        const double r = (double)N / t;
        e = (t <= capTau || r > cap) ? cap : r;
    }
    if (tau) tau[j] = t;
    if (ess) ess[j] = e;
    if (window) window[j] = w;
}
// Cross moments of the committed models (hmcmt_chain_cov_*).  Every array has the CELL INDEX FASTEST: the lanes of a wavefront are
// neighbouring cells a of one row or slot and touch adjacent doubles.  Counted commits are t = 0, 1, ...; y_t[a] = m[a] - x0[a] with
// x0 the value at t = 0 (one subtraction; y_0 = 0 by definition).  Per cell: tot = sum y_t (serial adds), q = fma(y_t, y_t, q).  Per
// row r with cell rho = row[r]: S[r][a] = fma(y_t[rho], y_t[a], S[r][a]) over t in commit order.  The commit only parks y_t in the next
// of B slots pend[b][a]; a flush applies the parked commits to S in slot order, so every S[r][a] sees the same fmas in the same
// order whatever B is.
constexpr int CHAIN_COV_BATCH_MAX = 16;
constexpr int CHAIN_COV_BATCH_DEFAULT = 8;
constexpr int CHAIN_COV_TILE_COLS = 256;   // k_chain_cov_flush: cells of a workgroup, one per thread
constexpr int CHAIN_COV_TILE_ROWS = 32;    // ... and the rows it walks; the row panel in LDS is TILE_ROWS x BATCH_MAX doubles (4 KiB)
// commit t of cell a into the slot `slot` of pend
HD void item_chain_cov_commit(const double* m, double* x0, double* tot, double* q, double* pend, long long n, long long t, int slot,
                              long long a) {
    const double x = m[a];
    if (t == 0) x0[a] = x;
    const double y = t == 0 ? 0.0 : x - x0[a];
    tot[a] += y;
    q[a] = fma(y, y, q[a]);
    pend[(long long)slot * n + a] = y;
}
// one element of S through a flush of NB parked commits: prow[b] = pend[b][rho], ycol[b] = pend[b][a], in slot order
template <int NB>
HD double item_chain_cov_flush(const double* prow, const double* ycol, double s) {
#pragma unroll
    for (int b = 0; b < NB; ++b) s = fma(prow[b], ycol[b], s);
    return s;
}
// the read-out of N >= 1 commits (dN = (double)N).  Each formula is product, division, subtraction, division: nothing that a
// compiler could contract into an fma, so the host and the device give the same bits
HD double item_chain_cov_value(double s, double totr, double tota, double dN) {
    const double p = totr * tota;
    const double c = p / dN;
    const double d = s - c;
    return d / dN;
}
// element (r, a): cov[r][a]; the owner of row 0 also writes mean[a] and var[a] (each output may be nullptr; row == nullptr: row r is
// cell r)
HD void item_chain_cov_out(const double* x0, const double* tot, const double* q, const double* S, const long long* row, long long n,
                           double dN, long long r, long long a, double* mean, double* var, double* cov) {
    const double ta = tot[a];
    if (r == 0) {
        if (mean) mean[a] = x0[a] + ta / dN;
        if (var) var[a] = item_chain_cov_value(q[a], ta, ta, dN);
    }
    if (cov) cov[r * n + a] = item_chain_cov_value(S[r * n + a], tot[row ? row[r] : r], ta, dN);
}
// element (r, a) of the correlation: cov / sqrt(var_rho var_a) clamped into [-1, 1]; 0 unless both variances are positive
HD void item_chain_corr(const double* tot, const double* q, const double* S, const long long* row, long long n, double dN, long long r,
                        long long a, double* corr) {
    const long long rho = row ? row[r] : r;
    const double tr = tot[rho], ta = tot[a];
    const double vr = item_chain_cov_value(q[rho], tr, tr, dN), va = item_chain_cov_value(q[a], ta, ta, dN);
    double c = 0.0;
    if (vr > 0.0 && va > 0.0) {
        const double vv = vr * va;
        c = item_chain_cov_value(S[r * n + a], tr, ta, dN) / sqrt(vv);
        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    }
    corr[r * n + a] = c;
}

// ----------------------------------------------------------------------------------------------
// the low-rank-plus-diagonal mass (hmcmt_set_mass_lowrank, kernels_mass.h: k_mass_lr_project, k_mass_lr_expand)
// ----------------------------------------------------------------------------------------------
// M^-1 = S (I + U (Lambda - I) U') S,  M = F F',  F = S^-1 (I + U (Lambda^-1/2 - I) U');  S = diag(s), U [rank][n] direction-contiguous.
// One application is y = post .* (x' + U' (c .* (U x'))): x' = s .* x, post = s, c = lambda - 1 for M^-1 x; x' = x, post = 1 / s,
// c = lambda^-1/2 - 1 for F x.  The projection t = U x' is reduced in a fixed order: a thread walks its cells upwards with fma, the
// 64 lanes of a wave add up in wave_sum's tree, the four waves as item_mass_lr_block, the CHAIN_NB workgroups in index order.
constexpr int MASS_LR_RANK_MAX = 32;
constexpr int MASS_LR_CHUNK = 8;       // directions a thread accumulates side by side (registers, indexed at compile time)
// x'[a]: op 0 (M^-1 x) scales by s, op 1 (F x) does not
HD double item_mass_lr_pre(const double* s, const double* x, int op, long long a) { return op == 0 ? s[a] * x[a] : x[a]; }
// cell a's terms of the projections k0 .. k0 + nk - 1 (nk <= MASS_LR_CHUNK) onto acc[0 .. MASS_LR_CHUNK)
HD void item_mass_lr_acc(const double* U, long long n, int k0, int nk, double xp, long long a, double (&acc)[MASS_LR_CHUNK]) {
#pragma unroll
    for (int q = 0; q < MASS_LR_CHUNK; ++q)
        if (q < nk) acc[q] = fma(U[(long long)(k0 + q) * n + a], xp, acc[q]);
}
// a workgroup's partial sum from its four waves' sums
HD double item_mass_lr_block(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }
// w_k = c_k t_k, t_k the workgroups' partial sums in index order
HD double item_mass_lr_weight(const double* part, const double* c, int k) { return c[k] * item_chain_total(part + (long long)k * CHAIN_NB); }
// y[a] = post[a] (x'[a] + sum_k U[k][a] w_k), k upwards
HD double item_mass_lr_expand(const double* s, const double* x, const double* U, const double* w, long long n, int rank, int op, long long a) {
    double acc = item_mass_lr_pre(s, x, op, a);
    for (int k = 0; k < rank; ++k) acc = fma(U[(long long)k * n + a], w[k], acc);
    return op == 0 ? s[a] * acc : acc / s[a];
}

// ----------------------------------------------------------------------------------------------
// the No-U-turn sampler of the device chain (hmcmt_chain_nuts_*, kernels_nuts.h: k_nuts_leaf, k_nuts_final; include/hmcmt.h has the
// algorithm): the draws, one cell's share of a leaf's sums, and the scalar state machine of the host
// ----------------------------------------------------------------------------------------------
constexpr int NUTS_DEPTH_MAX = 10;     // == HMCMT_NUTS_DEPTH_MAX
constexpr int NUTS_CK_MAX = 9;         // checkpoint slots: popcount(i >> 1) of an even leaf i < 2^(NUTS_DEPTH_MAX - 1) is at most 8
constexpr int NUTS_GROUP = 4;          // due checkpoints a thread takes per pass over the cells (registers, indexed at compile time)
constexpr int NUTS_NACC = 3 + 2 * NUTS_GROUP;       // accumulators of a pass: p.x, the merged tree's pair, two per checkpoint
constexpr int NUTS_NQ = 3 + 2 * NUTS_CK_MAX;        // sums of a leaf: q = 0 p.x; 1, 2 x.rho' and x_other.rho' of the merged tree;
                                                    //   3 + 2c, 4 + 2c x_ck.span and x.span of the c-th due checkpoint
// scalars of one leaf, device side: what the evaluation left, the sample's K0, then the NUTS_NQ sums
enum { NS_D1 = 0, NS_M1 = 1, NS_FLAG = 2, NS_K0 = 3, NS_SUM = 4, NUTS_SCAL = NS_SUM + NUTS_NQ };
constexpr uint32_t RNG_C0_NUTS_LEAF = 0x80000000u, RNG_C0_NUTS_DIR = 0xC0000000u;
// the sample's draws beside the momentum: kind 0, doubling j -- its direction and the uniform of its merge; kind 1, the sample's l-th
// leaf -- the uniform of its selection inside the subtree
HD void item_rng_nuts(uint64_t seed, uint32_t stream, uint64_t t, int kind, uint32_t index, int* forward, double* u) {
    uint32_t x[4];
    item_rng_block(seed, stream, t, (kind == 0 ? RNG_C0_NUTS_DIR : RNG_C0_NUTS_LEAF) + index, x);
    *u = item_rng_u52(x[0], x[1]);
    *forward = kind == 0 ? (int)(x[2] >> 31) : 0;
}

// One leaf's pass over the cells.  Momenta and x = M^-1 p are in the forward-time sign: the moving end stores sign * p (the backward
// end integrates the same map on -p), and so does the other end with signOther.
struct NutsLeaf {
    int n;
    int first;                     // leaf 0 of its subtree: rhoS = p, else rhoS += p
    int merged;                    // the subtree's last leaf: rhoNext = rho + rhoS and the two products of the merged tree
    int ndue;                      // due checkpoints of this pass (<= NUTS_GROUP), the first of them is the leaf's q0-th
    int q0;
    double sign, signOther;
    const double* p;               // [n] the moving end's stored momentum
    const double* x;               // [n] M^-1 of it, or nullptr: the diagonal invM
    const double* invM;            // [n]
    double* rhoS;                  // [n] the subtree's momentum sum
    double *ckP, *ckX, *ckR;       // an even leaf's checkpoint (p, x, rhoS), nullptr on an odd leaf
    const double *dueP[NUTS_GROUP], *dueX[NUTS_GROUP], *dueR[NUTS_GROUP];
    const double* rho;             // [n] the tree's momentum sum
    double* rhoNext;               // [n]
    const double *pOther, *xOther; // the end that stands still (xOther nullptr: the diagonal invM)
    double* part;                  // [NUTS_NQ][CHAIN_NB]
};
// cell a of a leaf's pass.  FIRST: the pass that updates rhoS, writes the checkpoint and forms p.x and the merged tree's pair; the
// further passes of a leaf with more than NUTS_GROUP due checkpoints only read.  acc[0 .. 3) belong to FIRST, acc[3 + 2c], acc[4 + 2c]
// to the pass's c-th checkpoint; every term enters by one fma.
template <int NCK, bool FIRST>
HD void item_nuts_cell(const NutsLeaf& L, int a, double (&acc)[NUTS_NACC]) {
    const double ps = L.p[a];
    const double p = L.sign * ps, x = L.sign * (L.x ? L.x[a] : L.invM[a] * ps);
    double rs;
    if (FIRST) {
        rs = L.first ? p : L.rhoS[a] + p;
        L.rhoS[a] = rs;
        if (L.ckP) { L.ckP[a] = p; L.ckX[a] = x; L.ckR[a] = rs; }
        acc[0] = fma(p, x, acc[0]);
        if (L.merged) {
            const double po = L.pOther[a];
            const double xo = L.signOther * (L.xOther ? L.xOther[a] : L.invM[a] * po);
            const double rn = L.rho[a] + rs;
            L.rhoNext[a] = rn;
            acc[1] = fma(x, rn, acc[1]);
            acc[2] = fma(xo, rn, acc[2]);
        }
    } else {
        rs = L.rhoS[a];
    }
#pragma unroll
    for (int c = 0; c < NCK; ++c) {
        const double span = (rs - L.dueR[c][a]) + L.dueP[c][a];
        acc[3 + 2 * c] = fma(L.dueX[c][a], span, acc[3 + 2 * c]);
        acc[4 + 2 * c] = fma(x, span, acc[4 + 2 * c]);
    }
}
// row of `part` that accumulator q of a pass lands in
HD int item_nuts_row(const NutsLeaf& L, int q) { return q < 3 ? q : q + 2 * L.q0; }

// The checkpoints of leaf i of a subtree: an even leaf stores slot popcount(i >> 1); an odd leaf checks *ndue = (trailing ones of i)
// slots, from *slot = popcount(i >> 1) downwards -- the spans [i + 1 - 2^s, i], s = 1 .. ndue, each once.
HD void item_nuts_checkpoints(int i, int* slot, int* ndue) {
    int k = 0;
    for (int v = i >> 1; v; v >>= 1) k += v & 1;
    int t = 0;
    for (int v = i; v & 1; v >>= 1) ++t;
    *slot = k;
    *ndue = t;
}

HD double item_nuts_logaddexp(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    return a > b ? a + log1p(exp(b - a)) : b + log1p(exp(a - b));
}
// The tree of one sample, host scalars.  Times are signed leapfrog steps from the start state.
struct NutsTree {
    int maxDepth = 0;
    double H0 = 0;
    int depth = 0, nleaves = 0, stop = -1;         // stop < 0: growing
    uint32_t dirs = 0;
    long long selected = 0, tMinus = 0, tPlus = 0;
    double logW = 0, alphaSum = 0;
    // the doubling at hand
    int forward = 0, i = 0;                        // i: the next leaf of the subtree
    long long selS = 0;
    double logWs = -INFINITY;
};
HD void item_nuts_begin(NutsTree& T, int maxDepth, double H0) {
    T = NutsTree{};
    T.maxDepth = maxDepth;
    T.H0 = H0;
}
HD void item_nuts_doubling(NutsTree& T, int forward) {
    T.forward = forward;
    if (forward) T.dirs |= 1u << T.depth;
    T.i = 0;
    T.logWs = -INFINITY;
}
// Leaf T.i of the doubling with energy H, its uniform u and its sums (NUTS_NQ, rows as in NutsLeaf).  Returns 0 the subtree goes on,
// 1 it is complete (item_nuts_merge follows), -1 the sample has stopped (T.stop); *take: the leaf is the subtree's selection.
HD int item_nuts_leaf(NutsTree& T, double H, double u, const double* sums, bool* take) {
    const double delta = T.H0 - H;
    const int i = T.i;
    *take = false;
    ++T.nleaves;
    if (!std::isfinite(delta) || -delta > 1000.0) { T.stop = 3; return -1; }
    T.alphaSum += delta > 0 ? 1.0 : exp(delta);
    T.logWs = item_nuts_logaddexp(T.logWs, delta);
    if (i == 0 || u < exp(delta - T.logWs)) {
        *take = true;
        T.selS = T.forward ? T.tPlus + i + 1 : T.tMinus - i - 1;
    }
    int slot, ndue;
    item_nuts_checkpoints(i, &slot, &ndue);
    if (i & 1)
        for (int c = 0; c < ndue; ++c)
            if (!(sums[3 + 2 * c] > 0.0) || !(sums[4 + 2 * c] > 0.0)) { T.stop = 1; return -1; }
    T.i = i + 1;
    return T.i == (1 << T.depth) ? 1 : 0;
}
// The completed subtree joins the tree: u is the doubling's uniform, sums the last leaf's.  *take: the subtree's selection becomes the
// tree's.  Returns 0 the tree doubles again, -1 the sample has stopped.
HD int item_nuts_merge(NutsTree& T, double u, const double* sums, bool* take) {
    const double d = T.logWs - T.logW;
    *take = u < exp(d < 0 ? d : 0.0);
    if (*take) T.selected = T.selS;
    T.logW = item_nuts_logaddexp(T.logW, T.logWs);
    if (T.forward) T.tPlus += 1LL << T.depth; else T.tMinus -= 1LL << T.depth;
    ++T.depth;
    if (!(sums[1] > 0.0) || !(sums[2] > 0.0)) { T.stop = 2; return -1; }
    if (T.depth == T.maxDepth) { T.stop = 0; return -1; }
    return 0;
}


// ---- initial guess extrapolated along the model path (kernels_fused.h: k_extrap_prepare, k_extrap) ----
#if !defined(__HIPCC__)
using std::min;                    // (the host instantiation of tests/emul: hipcc has its own overloads)
#endif
constexpr int EXT_NP = 6;          // fields kept per solve kind: the current one + EXT_NP-1 earlier ones (Lagrange order <= EXT_NP-1)
constexpr int EXT_NBLK = 32;       // blocks of the partial-sum pass
constexpr int EXT_NS = 2 * EXT_NP; // partial sums per block: <d_j,d1> (j = 0..NP-1), <d_j,d_j> (j = 0, 2..NP-1), <m_k,m_k>
constexpr int EXT_KEEP = EXT_NP, EXT_COUNT = EXT_NP + 1, EXT_HEAD = EXT_NP + 2, EXT_MHEAD = EXT_NP + 3, EXT_PART = EXT_NP + 4;
// ext = {w_0..w_{NP-1}, keep, count, head of the field ring, head of the model ring, partial sums [NBLK][NS], ticket}
constexpr int EXT_TICKET = EXT_PART + EXT_NS * EXT_NBLK, EXT_LEN = EXT_TICKET + 1;

// The weights from the summed partials (one thread).
// coldUnlessSmooth (the adjoint solve): without at least three collinear points the weights are all zero -- the adjoint's
// right-hand side is the weighted residual, which changes by O(1) from step to step, so its previous solution is no
// better a guess than zero (measured on the sampler's trajectories: 0-4 iterations WORSE than a cold start) unless the
// model path is smooth enough for the extrapolation proper.  Returns keep (the model is a repeat: nothing moves).
HD bool extrap_weights(const double* a, double* ext, int maxNp, int coldUnlessSmooth) {
    const int count = (int)ext[EXT_COUNT];
    const double d1d1 = a[1], d0d0 = a[EXT_NP], mkmk = a[EXT_NS - 1];
    const bool keep = count >= 1 && d0d0 <= 1e-28 * mkmk;
    double wts[EXT_NP];                                       // weights of x_k, x_{k-1}, ...
    for (int i = 0; i < EXT_NP; ++i) wts[i] = i == 0 ? 1.0 : 0.0;
    if (coldUnlessSmooth && !keep) wts[0] = 0.0;
    if (!keep && count >= 2 && d1d1 > 0) {
        const double alpha = fmin(2.0, fmax(-1.0, a[0] / d1d1));
        wts[0] = 1.0 + alpha; wts[1] = -alpha;
        // "times" of the models on the line through the last step: 0, -1, -1-g2, -1-g2-g3, ...; a further point is used
        // while its step is nearly collinear with the last one and of comparable length
        double tau[EXT_NP];
        tau[0] = 0.0; tau[1] = -1.0;
        int np = 2;
        if (d0d0 > 0 && a[0] / sqrt(d0d0 * d1d1) > 0.95 && alpha > 0.5 && alpha < 2.0) {
            for (int j = 2; j < EXT_NP; ++j) {
                const double djdj = a[EXT_NP + j - 1], g = a[j] / d1d1;
                if (!(count >= j + 1 && djdj > 0 && a[j] / sqrt(djdj * d1d1) > 0.95 && g > 0.5 && g < 2.0)) break;
                tau[j] = tau[j - 1] - g;
                np = j + 1;
            }
        }
        np = min(maxNp, np);
        if (coldUnlessSmooth && np <= 2) wts[0] = wts[1] = 0.0;
        if (np > 2) {
            for (int i = 0; i < EXT_NP; ++i) {
                double l = i < np ? 1.0 : 0.0;
                for (int j = 0; j < np; ++j)
                    if (j != i && i < np) l *= (alpha - tau[j]) / (tau[i] - tau[j]);
                wts[i] = l;
            }
        }
    }
    for (int i = 0; i < EXT_NP; ++i) ext[i] = wts[i];
    ext[EXT_KEEP] = keep ? 1.0 : 0.0;
    if (!keep) {
        ext[EXT_COUNT] = (double)min(count + 1, EXT_NP);
        // both histories are rings: the heads move back by one, the model ring's onto the slot k_extrap_prepare has just
        // filled with the new model, the field ring's onto its oldest entry, which receives the solution that is about to
        // be replaced by the new guess (k_extrap)
        ext[EXT_HEAD] = (double)(((int)ext[EXT_HEAD] + EXT_NP - 2) % (EXT_NP - 1));
        ext[EXT_MHEAD] = (double)(((int)ext[EXT_MHEAD] + EXT_NP) % (EXT_NP + 1));
    }
    return keep;
}

// ----------------------------------------------------------------------------------------------
// low-rank mass in the warm-up (hmcmt_chain_adapt_lowrank; kernels_chain.h: k_adapt_lr_store, k_adapt_lr_mean, k_adapt_lr_gram,
// k_adapt_lr_lift, k_adapt_lr_sign; include/hmcmt.h has the algorithm)
// ----------------------------------------------------------------------------------------------
// A window stores n <= ADAPT_LR_NMAX pairs (draw, full potential gradient), rows X[i][.], G[i][.] of nAC cells.  With s = sqrt(invM)
// and W = [Zd; Zg], Zd = (X - mean_X) / s / sqrt(n - 1), Zg = (G - mean_G) s / sqrt(n - 1), the device forms K = W W' ([2n][2n]) and,
// from the host's B ([2n][r]), U = B' W.  Every sum has one owner and one order: the means add the rows upwards and divide once;
// K[i][j] is ONE fma chain over the cells upwards from 0 (the workgroup that owns the tile walks all cells); U[k][a] is one fma chain
// over the rows upwards.  Nothing here can be contracted differently by two compilers: the products stand inside fma, the rest are
// single operations.
constexpr int ADAPT_LR_NMIN = 4, ADAPT_LR_NMAX = 128;       // pairs per window: below NMIN the window falls back to the diagonal
constexpr int ADAPT_LR_TILE = 16;                          // a workgroup owns ADAPT_LR_TILE x ADAPT_LR_TILE outputs of K
constexpr int ADAPT_LR_STRIP = 64;                         // cells of the two row blocks staged through LDS per pass
// thinning: the window's length is known when it opens; its i-th step is stored when i % stride == 0
HD long long item_adapt_lr_stride(long long length, long long maxSamples) { return length <= maxSamples ? 1 : (length + maxSamples - 1) / maxSamples; }
HD bool item_adapt_lr_due(long long i, long long stride) { return i % stride == 0; }
// cell a's entry of the full potential gradient g_data + lambda Wm (m - m_ref): the CSR row arithmetic of k_lf_momentum_max
HD double item_adapt_lr_grad(const double* gdata, double lambda, const long long* wmRow, const long long* wmCol, const double* wmVal,
                             const double* m, const double* mref, long long a) {
    double acc = 0.0;
    for (long long t = wmRow[a]; t < wmRow[a + 1]; ++t) {
        const long long j = wmCol[t];
        acc += wmVal[t] * (m[j] - mref[j]);
    }
    return gdata[a] + lambda * acc;
}
// cell a's mean over the n stored rows, in row order
HD double item_adapt_lr_mean(const double* R, long long nAC, int n, long long a) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += R[(long long)i * nAC + a];
    return acc / (double)n;
}
// W[i][a], i < 2n: the centred draw over s (i < n) or the centred gradient times s; sq = sqrt(n - 1) as a double
HD double item_adapt_lr_w(const double* X, const double* G, const double* meanX, const double* meanG, const double* s, long long nAC, int n,
                          double sq, int i, long long a) {
    if (i < n) return ((X[(long long)i * nAC + a] - meanX[a]) / s[a]) / sq;
    return ((G[(long long)(i - n) * nAC + a] - meanG[a]) * s[a]) / sq;
}
// one term of K[i][j] and of U[k][a]
HD double item_adapt_lr_dot(double wi, double wj, double acc) { return fma(wi, wj, acc); }
// U[k][a] = sum_i B[i][k] W[i][a], i upwards
HD double item_adapt_lr_lift(const double* X, const double* G, const double* meanX, const double* meanG, const double* s, const double* B,
                             long long nAC, int n, double sq, int r, int k, long long a) {
    double acc = 0.0;
    for (int i = 0; i < 2 * n; ++i) acc = item_adapt_lr_dot(B[(long long)i * r + k], item_adapt_lr_w(X, G, meanX, meanG, s, nAC, n, sq, i, a), acc);
    return acc;
}
// the sign convention's comparison: does (|v|, a) beat (best, at)?  The larger magnitude wins, the lower index a tie
HD bool item_adapt_lr_beats(double v, long long a, double best, long long at) { return v > best || (v == best && a < at); }

// ---- the host's share of a window end, in double (the emulation of tests/emul runs these very functions) ---------------------------
// Cyclic Jacobi for a symmetric A [n][n] (row-major, destroyed): d[k] ascending, Vt[k][.] the unit eigenvector of d[k].  Rows sweep
// (p, q), p < q upwards; a rotation is skipped where |a_pq| <= 2^-53 sqrt|a_pp a_qq| or |a_pq| <= 1e-40 |A|_F; the sweeps end with
// the first one that rotates nothing, after ADAPT_LR_SWEEPS_MAX at the latest.  Returns the sweeps taken: ADAPT_LR_SWEEPS_MAX says not converged.
constexpr int ADAPT_LR_SWEEPS_MAX = 64;
inline int item_jacobi_eig(int n, double* A, double* Vt, double* d) {
    double frob = 0.0;
    for (long long e = 0; e < (long long)n * n; ++e) frob += A[e] * A[e];
    const double floorAbs = 1e-40 * sqrt(frob), eps = 1.1102230246251565e-16;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Vt[(long long)i * n + j] = i == j ? 1.0 : 0.0;
    int sweep = 0;
    for (; sweep < ADAPT_LR_SWEEPS_MAX; ++sweep) {
        long long rotated = 0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double* Ap = A + (long long)p * n;
                double* Aq = A + (long long)q * n;
                const double apq = Ap[q], app = Ap[p], aqq = Aq[q];
                if (!(fabs(apq) > eps * sqrt(fabs(app * aqq))) || !(fabs(apq) > floorAbs)) { Ap[q] = Aq[p] = (fabs(apq) > floorAbs ? apq : 0.0); continue; }
                ++rotated;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = Ap[k], akq = Aq[k];
                    Ap[k] = c * akp - s * akq;
                    Aq[k] = s * akp + c * akq;
                }
                Ap[p] = app - t * apq; Aq[q] = aqq + t * apq; Ap[q] = Aq[p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    if (k == p || k == q) continue;
                    A[(long long)k * n + p] = Ap[k];
                    A[(long long)k * n + q] = Aq[k];
                }
                double* Vp = Vt + (long long)p * n;
                double* Vq = Vt + (long long)q * n;
                for (int k = 0; k < n; ++k) {
                    const double vp = Vp[k], vq = Vq[k];
                    Vp[k] = c * vp - s * vq;
                    Vq[k] = s * vp + c * vq;
                }
            }
        if (rotated == 0) break;
    }
    // ascending, the lower index first among equals (insertion sort: n <= 256)
    for (int i = 0; i < n; ++i) d[i] = A[(long long)i * n + i];
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && d[j] < d[j - 1]; --j) {
            const double td = d[j]; d[j] = d[j - 1]; d[j - 1] = td;
            for (int k = 0; k < n; ++k) { const double tv = Vt[(long long)j * n + k]; Vt[(long long)j * n + k] = Vt[(long long)(j - 1) * n + k]; Vt[(long long)(j - 1) * n + k] = tv; }
        }
    return sweep;
}
inline void item_adapt_lr_matmul(int m, const double* A, const double* B, double* C) {      // C = A B, all [m][m]
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) C[(size_t)i * m + j] = 0.0;
    for (int i = 0; i < m; ++i)
        for (int k = 0; k < m; ++k) {
            const double a = A[(size_t)i * m + k];
            for (int j = 0; j < m; ++j) C[(size_t)i * m + j] += a * B[(size_t)k * m + j];
        }
}
struct AdaptLrEstimate {
    int m = 0, r = 0, fallback = 0;            // dimensions kept of K, directions selected, 1: no estimate (the window ends on the diagonal)
    double thetaMin = 0, thetaMax = 0;         // over all m
    std::vector<double> thetaAll;              // [m] ascending
    std::vector<double> theta;                 // [r] by |ln theta| descending
    std::vector<double> B;                     // [2n][r]: U = B' W
};
// The window end's host maths in three parts, so that the emulation can put another Sigma between the first and the last (the
// exact-answer test's counter-example); item_adapt_lr_estimate is the three in a row and what the library calls.
// 1. From K = W W' ([2n][2n]) of n pairs: the m eigenvalues D_i > 1e-10 D_max kept, T = D^-1/2 V' ([m][2n]: T W has orthonormal rows),
//    and the two covariances projected on them, Cd = Pd Pd' + gamma I and Cg = Pg Pg' + gamma I with [Pd Pg] = T K.  Returns m, 0: none.
inline int item_adapt_lr_project(int n, const double* K, double gamma, std::vector<double>& T, std::vector<double>& Cd, std::vector<double>& Cg) {
    const int N2 = 2 * n;
    if (n < ADAPT_LR_NMIN) return 0;
    for (size_t e = 0; e < (size_t)N2 * N2; ++e)
        if (!std::isfinite(K[e])) return 0;
    std::vector<double> A(K, K + (size_t)N2 * N2), Vt((size_t)N2 * N2), d((size_t)N2);
    if (item_jacobi_eig(N2, A.data(), Vt.data(), d.data()) >= ADAPT_LR_SWEEPS_MAX) return 0;
    const double dmax = d[N2 - 1];
    if (!(dmax > 0.0)) return 0;
    int first = 0;
    while (first < N2 && !(d[first] > 1e-10 * dmax)) ++first;
    const int m = N2 - first;
    T.assign((size_t)m * N2, 0.0);                          // T = D^-1/2 V'
    for (int k = 0; k < m; ++k) {
        const double f = 1.0 / sqrt(d[first + k]);
        for (int i = 0; i < N2; ++i) T[(size_t)k * N2 + i] = Vt[(size_t)(first + k) * N2 + i] * f;
    }
    std::vector<double> P((size_t)m * N2);                 // P = T K = [Pd Pg]
    for (int k = 0; k < m; ++k)
        for (int j = 0; j < N2; ++j) {
            double acc = 0.0;
            for (int i = 0; i < N2; ++i) acc += T[(size_t)k * N2 + i] * K[(size_t)i * N2 + j];
            P[(size_t)k * N2 + j] = acc;
        }
    Cd.assign((size_t)m * m, 0.0); Cg.assign((size_t)m * m, 0.0);
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) {
            double sd = 0.0, sg = 0.0;
            for (int j = 0; j < n; ++j) {
                sd += P[(size_t)a * N2 + j] * P[(size_t)b * N2 + j];
                sg += P[(size_t)a * N2 + n + j] * P[(size_t)b * N2 + n + j];
            }
            Cd[(size_t)a * m + b] = sd + (a == b ? gamma : 0.0);
            Cg[(size_t)a * m + b] = sg + (a == b ? gamma : 0.0);
        }
    return m;
}
inline void item_adapt_lr_symmetrise(int m, std::vector<double>& S) {
    for (int a = 0; a < m; ++a)
        for (int b = a + 1; b < m; ++b) S[(size_t)a * m + b] = S[(size_t)b * m + a] = 0.5 * (S[(size_t)a * m + b] + S[(size_t)b * m + a]);
}
// 2. Sigma = Cg^-1/2 (Cg^1/2 Cd Cg^1/2)^1/2 Cg^-1/2, the symmetric positive definite solution of Sigma Cg Sigma = Cd, and its
//    eigenpairs: th ascending, Yt[k][.] the eigenvector of th[k].  Evaluated in the eigenbasis of Cg = Q Gamma Q', where the powers of Cg
//    are diagonal scalings: Cg's eigenvalues reach from gamma up, and a product with a dense Cg^+-1/2 would round its small ones away.
//    false: an eigensolver that did not converge, an eigenvalue that is not finite and positive.
inline bool item_adapt_lr_sigma(int m, const std::vector<double>& Cd, const std::vector<double>& Cg, std::vector<double>& Yt, std::vector<double>& th) {
    std::vector<double> Sig((size_t)m * m), t1((size_t)m * m), t2((size_t)m * m);
    std::vector<double> Qt((size_t)m * m), g((size_t)m), QtT((size_t)m * m), Zt((size_t)m * m), e((size_t)m);
    Yt.assign((size_t)m * m, 0.0); th.assign((size_t)m, 0.0);
    t1 = Cg;
    if (item_jacobi_eig(m, t1.data(), Qt.data(), g.data()) >= ADAPT_LR_SWEEPS_MAX) return false;
    for (int k = 0; k < m; ++k) {
        if (!(g[k] > 0.0) || !std::isfinite(g[k])) return false;
        g[k] = sqrt(g[k]);
    }
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) QtT[(size_t)a * m + b] = Qt[(size_t)b * m + a];
    item_adapt_lr_matmul(m, Qt.data(), Cd.data(), t1.data());
    item_adapt_lr_matmul(m, t1.data(), QtT.data(), t2.data());                // Q' Cd Q
    item_adapt_lr_symmetrise(m, t2);
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) t2[(size_t)a * m + b] = g[a] * t2[(size_t)a * m + b] * g[b];
    if (item_jacobi_eig(m, t2.data(), Zt.data(), e.data()) >= ADAPT_LR_SWEEPS_MAX) return false;
    for (int k = 0; k < m; ++k) {
        if (!(e[k] > 0.0) || !std::isfinite(e[k])) return false;
        e[k] = sqrt(e[k]);
    }
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) {
            double acc = 0.0;
            for (int k = 0; k < m; ++k) acc += Zt[(size_t)k * m + a] * e[k] * Zt[(size_t)k * m + b];
            Sig[(size_t)a * m + b] = acc / g[a] / g[b];
        }
    item_adapt_lr_symmetrise(m, Sig);
    if (item_jacobi_eig(m, Sig.data(), t1.data(), th.data()) >= ADAPT_LR_SWEEPS_MAX) return false;   // rows of t1: eigenvectors in Cg's eigenbasis
    item_adapt_lr_matmul(m, t1.data(), Qt.data(), Yt.data());                 // ... and back: Y = Q Yq
    return true;
}
// 3. The selection -- theta > cutoff or theta < 1 / cutoff, by |ln theta| descending, the lower index first among equals, at most rank --
//    and the coefficients B = T' Y_sel of the selected directions.
inline AdaptLrEstimate item_adapt_lr_select(int n, int m, const std::vector<double>& T, const std::vector<double>& Yt, const std::vector<double>& th,
                                            int rank, double cutoff) {
    AdaptLrEstimate E;
    E.fallback = 1;
    const int N2 = 2 * n;
    for (int k = 0; k < m; ++k)
        if (!(th[k] > 0.0) || !std::isfinite(th[k])) return E;
    std::vector<int> sel;
    for (int k = 0; k < m; ++k)
        if (th[k] > cutoff || th[k] < 1.0 / cutoff) sel.push_back(k);
    for (size_t i = 1; i < sel.size(); ++i)
        for (size_t j = i; j > 0 && fabs(log(th[sel[j]])) > fabs(log(th[sel[j - 1]])); --j) { const int t = sel[j]; sel[j] = sel[j - 1]; sel[j - 1] = t; }
    if ((int)sel.size() > rank) sel.resize((size_t)rank);
    const int r = (int)sel.size();
    E.m = m; E.r = r; E.fallback = 0;
    E.thetaMin = th[0]; E.thetaMax = th[m - 1];
    E.thetaAll = th;
    E.theta.resize((size_t)r);
    E.B.assign((size_t)N2 * r, 0.0);
    for (int c = 0; c < r; ++c) {
        E.theta[c] = th[sel[c]];
        for (int i = 0; i < N2; ++i) {
            double acc = 0.0;
            for (int j = 0; j < m; ++j) acc += T[(size_t)j * N2 + i] * Yt[(size_t)sel[c] * m + j];
            E.B[(size_t)i * r + c] = acc;
        }
    }
    for (double v : E.B)
        if (!std::isfinite(v)) { E = AdaptLrEstimate{}; E.fallback = 1; return E; }
    return E;
}
inline AdaptLrEstimate item_adapt_lr_estimate(int n, const double* K, int rank, double cutoff, double gamma) {
    AdaptLrEstimate none;
    none.fallback = 1;
    std::vector<double> T, Cd, Cg, Yt, th;
    const int m = item_adapt_lr_project(n, K, gamma, T, Cd, Cg);
    if (m == 0 || !item_adapt_lr_sigma(m, Cd, Cg, Yt, th)) return none;
    return item_adapt_lr_select(n, m, T, Yt, th, rank, cutoff);
}

// ----------------------------------------------------------------------------------------------
// the row sketch of the committed models (hmcmt_chain_sketch_*, hmcmt_chain_pca; kernels_chain.h: k_chain_sketch_commit,
// k_chain_sketch_gram, k_chain_sketch_shrink, k_chain_sketch_mean, k_chain_sketch_lift; include/hmcmt.h has the algorithm)
// ----------------------------------------------------------------------------------------------
// Frequent directions: B [2 ell + 1][nAC], cell index fastest.  Counted commit t puts y_t = m - x0 (one subtraction) into row `fill`;
// at fill == 2 ell the device forms K = B B' (rows 0 .. 2 ell - 1), the host turns its eigenpairs into T [ell][2 ell]
// (item_chain_sketch_shrink) and the device replaces B by T B.  Row 2 ell is staging of the read-out (sqrt(N) ybar).  Every sum has
// one owner and one order: K[i][j] is one fma chain over the cells upwards, (T B)[i][a] one fma chain over j upwards.
constexpr int CHAIN_SKETCH_ELL_MIN = 2, CHAIN_SKETCH_ELL_MAX = 64;
constexpr int CHAIN_SKETCH_ELL_DEFAULT = 32;
constexpr int CHAIN_SKETCH_COLS = 64;      // k_chain_sketch_shrink: cells of a workgroup, one per thread (one wavefront); its LDS holds
                                           //   2 ell x CHAIN_SKETCH_COLS doubles, 64 KiB at ell = 64
static_assert(2 * CHAIN_SKETCH_ELL_MAX * CHAIN_SKETCH_COLS * sizeof(double) <= 65536, "k_chain_sketch_shrink's columns fit the 64 KiB of dynamic LDS a launch gets by default");
constexpr int CHAIN_SKETCH_CHUNK = 8;      // output rows a thread of the shrink accumulates side by side (registers, indexed at compile time)
// commit t (the count before it) of cell a: the sums of hmcmt_chain_cov and the row of this commit
HD void item_chain_sketch_commit(const double* m, double* x0, double* tot, double* q, double* brow, long long t, int pivotGiven, long long a) {
    const double x = m[a];
    if (t == 0 && !pivotGiven) x0[a] = x;
    const double y = x - x0[a];
    tot[a] += y;
    q[a] = fma(y, y, q[a]);
    brow[a] = y;
}
// row gi of the Gram kernel's operand: rows 0 .. nrows - 1 of B, then the extra row (the read-out's mean row)
HD const double* item_chain_sketch_row(const double* B, const double* extra, long long nAC, int nrows, int gi) {
    return gi < nrows ? B + (long long)gi * nAC : extra;
}
// K[i][j] over all cells upwards (what the tiled kernel computes strip by strip)
HD double item_chain_sketch_gram(const double* ri, const double* rj, long long nAC) {
    double acc = 0.0;
    for (long long a = 0; a < nAC; ++a) acc = item_adapt_lr_dot(ri[a], rj[a], acc);
    return acc;
}
// (T B)[i][a] from cell a's column col[j * stride], j < n2 upwards
HD double item_chain_sketch_shrink(const double* Trow, const double* col, long long stride, int n2) {
    double acc = 0.0;
    for (int j = 0; j < n2; ++j) acc = fma(Trow[j], col[(long long)j * stride], acc);
    return acc;
}
// the read-out's mean row: sqrt(N) ybar[a], sqN = sqrt((double)N) (a division and a product: nothing to contract)
HD double item_chain_sketch_mean(double tot, double dN, double sqN) {
    const double ybar = tot / dN;
    return sqN * ybar;
}
// U[k][a] = sum_i coef[i][k] W[i][a], i < nw upwards; W = the filled rows and the mean row
HD double item_chain_sketch_lift(const double* B, const double* extra, const double* coef, long long nAC, int nrows, int nw, int r, int k, long long a) {
    double acc = 0.0;
    for (int i = 0; i < nw; ++i) acc = item_adapt_lr_dot(coef[(long long)i * r + k], item_chain_sketch_row(B, extra, nAC, nrows, i)[a], acc);
    return acc;
}
// The host's share of a shrink, in double.  K [2 ell][2 ell] (destroyed) -> T [ell][2 ell] and delta: with the eigenvalues descending
// d_0 >= d_1 >= ..., delta = max(d_ell, 0), c_i = d_i > delta ? sqrt((d_i - delta) / d_i) : 0, T[i][j] = c_i V[j][i].  false: K is not
// finite or the eigensolver did not converge.
inline bool item_chain_sketch_shrink_T(int ell, double* K, std::vector<double>& T, double* delta) {
    const int n2 = 2 * ell;
    for (size_t e = 0; e < (size_t)n2 * n2; ++e)
        if (!std::isfinite(K[e])) return false;
    std::vector<double> Vt((size_t)n2 * n2), d((size_t)n2);
    if (item_jacobi_eig(n2, K, Vt.data(), d.data()) >= ADAPT_LR_SWEEPS_MAX) return false;
    const double dl = d[n2 - 1 - ell];                      // (d is ascending: the descending d_i is d[n2 - 1 - i])
    *delta = dl > 0.0 ? dl : 0.0;
    T.assign((size_t)ell * n2, 0.0);
    for (int i = 0; i < ell; ++i) {
        const double di = d[n2 - 1 - i];
        const double c = di > *delta ? sqrt((di - *delta) / di) : 0.0;
        for (int j = 0; j < n2; ++j) T[(size_t)i * n2 + j] = c * Vt[(size_t)(n2 - 1 - i) * n2 + j];
    }
    return true;
}
// The host's share of hmcmt_chain_pca.  G [nw][nw] = W W' with the mean row LAST (destroyed).  G = Q Lambda Q' keeps the m values
// Lambda_i > 1e-10 Lambda_max; S = Lambda^1/2 Q' J Q Lambda^1/2, J = diag(1, ..., 1, -1), symmetrised; S = Z Theta Z'; the
// min(rank, #theta > 0) largest theta descending, the lower index first among equals; coef [nw][r] = Q Lambda^-1/2 Z_sel.
// Returns r >= 0, or -1: G is not finite, an eigensolver did not converge.
inline int item_chain_sketch_pca(int nw, double* G, int rank, std::vector<double>& theta, std::vector<double>& coef) {
    for (size_t e = 0; e < (size_t)nw * nw; ++e)
        if (!std::isfinite(G[e])) return -1;
    std::vector<double> Qt((size_t)nw * nw), lam((size_t)nw);
    if (item_jacobi_eig(nw, G, Qt.data(), lam.data()) >= ADAPT_LR_SWEEPS_MAX) return -1;
    theta.clear(); coef.clear();
    const double lmax = lam[nw - 1];
    if (!(lmax > 0.0)) return 0;
    int first = 0;
    while (first < nw && !(lam[first] > 1e-10 * lmax)) ++first;
    const int m = nw - first;
    std::vector<double> sq((size_t)m), S((size_t)m * m), Zt((size_t)m * m), th((size_t)m);
    for (int a = 0; a < m; ++a) sq[a] = sqrt(lam[first + a]);
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b) {
            double acc = 0.0;
            for (int i = 0; i < nw; ++i) {
                const double p = Qt[(size_t)(first + a) * nw + i] * Qt[(size_t)(first + b) * nw + i];
                acc += i == nw - 1 ? -p : p;
            }
            S[(size_t)a * m + b] = sq[a] * acc * sq[b];
        }
    item_adapt_lr_symmetrise(m, S);
    if (item_jacobi_eig(m, S.data(), Zt.data(), th.data()) >= ADAPT_LR_SWEEPS_MAX) return -1;
    int r = 0;
    while (r < m && r < rank && th[m - 1 - r] > 0.0) ++r;
    std::vector<int> sel((size_t)r);
    for (int c = 0; c < r; ++c) sel[c] = m - 1 - c;
    for (int c = 1; c < r; ++c)                              // (equal theta: the lower index first)
        for (int j = c; j > 0 && th[sel[j]] == th[sel[j - 1]] && sel[j] < sel[j - 1]; --j) { const int t = sel[j]; sel[j] = sel[j - 1]; sel[j - 1] = t; }
    theta.resize((size_t)r);
    coef.assign((size_t)nw * (r > 1 ? r : 1), 0.0);
    for (int c = 0; c < r; ++c) {
        theta[c] = th[sel[c]];
        for (int i = 0; i < nw; ++i) {
            double acc = 0.0;
            for (int a = 0; a < m; ++a) acc += Qt[(size_t)(first + a) * nw + i] / sq[a] * Zt[(size_t)sel[c] * m + a];
            coef[(size_t)i * r + c] = acc;
        }
    }
    for (double v : coef)
        if (!std::isfinite(v)) return -1;
    return r;
}

// ----------------------------------------------------------------------------------------------
// the MAP optimiser (hmcmt_map_*, kernels_map.h, host_map.h; include/hmcmt.h has the algorithm): projected L-BFGS in the compact form
// ----------------------------------------------------------------------------------------------
// The ring holds H slots: rows [0, H) the s of the slots, rows [H, 2 H) their y, n doubles each.  Pair i of `count`, oldest first, sits in
// slot (head + i) % H; S'Y and Y'Y ([H][H]) are indexed by SLOT.  Projection row q < count is s_q, row count + q is y_q.  Every sum has one
// owner and one order (a thread walks its cells upwards with fma, wave_sum's tree, the four waves as item_mass_lr_block, the CHAIN_NB
// workgroups in index order); every product that feeds a sum stands inside fma, the rest are single operations.
constexpr int MAP_HISTORY_MAX = 32;                        // == HMCMT_MAP_HISTORY_MAX
constexpr int MAP_ROWS_MAX = 2 * MAP_HISTORY_MAX;
// rows of the partial sums [MAP_PART_ROWS][CHAIN_NB]: the projections, then the pass's own
enum { MAP_P_X0 = MAP_ROWS_MAX, MAP_P_X1, MAP_P_X2, MAP_P_X3, MAP_P_X4, MAP_P_MAX, MAP_P_NB, MAP_PART_ROWS };
// what the coefficient step leaves [MAP_COEF]: gamma (H0, or the step scale without pairs), the flag "not a descent direction" (the pairs were
// set aside), g'd, |pg|inf, |pg|2^2, |B|, the pairs the expansion uses, then a [H] and w = -gamma p [H] by pair
enum { MC_GAMMA = 0, MC_FLAG, MC_GTD, MC_PGINF, MC_PG2, MC_NB, MC_USED, MC_A = 8, MC_W = MC_A + MAP_HISTORY_MAX, MAP_COEF = MC_W + MAP_HISTORY_MAX };
// what a trial's pass leaves [MAP_SCAL]: D, M, g's, s'y, s's, y'y and, of the TRIAL state, |pg|2^2, |pg|inf, |B|
enum { MS_D = 0, MS_M, MS_GTS, MS_STY, MS_STS, MS_YTY, MS_PG2, MS_PGINF, MS_NB, MAP_SCAL };
struct MapRing { const double* rows; long long n; int H, head, count; };
HD int item_map_slot(const MapRing& R, int i) { return (R.head + i) % R.H; }
HD const double* item_map_row(const MapRing& R, int q) {
    return q < R.count ? R.rows + (long long)item_map_slot(R, q) * R.n : R.rows + (long long)(R.H + item_map_slot(R, q - R.count)) * R.n;
}
// cell a is in the active set B: on a bound with the gradient pushing outwards
HD bool item_map_bound(double m, double g, double lo, double hi) { return (m <= lo && g > 0.0) || (m >= hi && g < 0.0); }
HD double item_map_pg(const double* m, const double* g, double lo, double hi, long long a) { return item_map_bound(m[a], g[a], lo, hi) ? 0.0 : g[a]; }
// cell a's terms of the projections q0 .. q0 + nq - 1 (nq <= MASS_LR_CHUNK) of the vector whose entry there is x
HD void item_map_proj_acc(const MapRing& R, int q0, int nq, double x, long long a, double (&acc)[MASS_LR_CHUNK]) {
#pragma unroll
    for (int q = 0; q < MASS_LR_CHUNK; ++q)
        if (q < nq) acc[q] = fma(item_map_row(R, q0 + q)[a], x, acc[q]);
}
// The coefficient algebra of one direction (Byrd, Nocedal, Schnabel 1994, eq. 3.13 with H0 = gamma I): R = the upper triangle of S'Y,
// Dg its diagonal; p = R^-1 S'pg, a = R^-T ((Dg + gamma Y'Y) p - gamma Y'pg), H pg = gamma pg + S a - gamma Y p.  t [2 count]: S'pg then
// Y'pg.  g'd = -pg'H pg, since d is -H pg off B and pg is 0 on B.  Without pairs, or when g'd is not negative with pairs (the flag),
// d = -pg min(1, 1 / |pg|inf).  Serial on purpose: two triangular solves of at most 32 unknowns are dependency chains.
HD void item_map_coef(const MapRing& R, const double* SY, const double* YY, const double* t, double pg2, double pginf, double nb, double* out) {
    const int c = R.count, H = R.H;
    for (int i = 0; i < MAP_COEF; ++i) out[i] = 0.0;
    out[MC_PGINF] = pginf; out[MC_PG2] = pg2; out[MC_NB] = nb;
    const double g0 = pginf > 1.0 ? 1.0 / pginf : 1.0;
    bool ok = false;
    if (c > 0) {
        const int nn = item_map_slot(R, c - 1);
        const double gamma = SY[nn * H + nn] / YY[nn * H + nn];
        double p[MAP_HISTORY_MAX], a[MAP_HISTORY_MAX];
        for (int i = c - 1; i >= 0; --i) {
            const int si = item_map_slot(R, i);
            double acc = t[i];
            for (int j = i + 1; j < c; ++j) acc = fma(-SY[si * H + item_map_slot(R, j)], p[j], acc);
            p[i] = acc / SY[si * H + si];
        }
        for (int i = 0; i < c; ++i) {
            const int si = item_map_slot(R, i);
            double z = -t[c + i];
            for (int j = 0; j < c; ++j) z = fma(YY[si * H + item_map_slot(R, j)], p[j], z);
            a[i] = fma(gamma, z, SY[si * H + si] * p[i]);
        }
        for (int i = 0; i < c; ++i) {
            const int si = item_map_slot(R, i);
            double acc = a[i];
            for (int j = 0; j < i; ++j) acc = fma(-SY[item_map_slot(R, j) * H + si], a[j], acc);
            a[i] = acc / SY[si * H + si];
        }
        double h = gamma * pg2;
        for (int i = 0; i < c; ++i) h = fma(a[i], t[i], h);
        for (int i = 0; i < c; ++i) { out[MC_A + i] = a[i]; out[MC_W + i] = -(gamma * p[i]); h = fma(out[MC_W + i], t[c + i], h); }
        ok = -h < 0.0 && gamma > 0.0 && gamma <= 1.7976931348623157e308;
        if (ok) { out[MC_GAMMA] = gamma; out[MC_GTD] = -h; out[MC_USED] = (double)c; }
        else out[MC_FLAG] = 1.0;
    }
    if (!ok) { out[MC_GAMMA] = g0; out[MC_GTD] = -(g0 * pg2); out[MC_USED] = 0.0; }
}
// d[a] = -(gamma pg + sum_i s_i a_i + sum_i y_i w_i), pairs upwards, S before Y; exactly 0 on B
HD double item_map_dir(const MapRing& R, const double* coef, double pg, bool bound, long long a) {
    if (bound) return 0.0;
    const int used = (int)coef[MC_USED];
    double acc = coef[MC_GAMMA] * pg;
    for (int i = 0; i < used; ++i) acc = fma(item_map_row(R, i)[a], coef[MC_A + i], acc);
    for (int i = 0; i < used; ++i) acc = fma(item_map_row(R, R.count + i)[a], coef[MC_W + i], acc);
    return -acc;
}
// the trial's entry: clip(m + alpha d)
HD double item_map_clip(double m, double alpha, double d, double lo, double hi) {
    const double t = fma(alpha, d, m);
    return t < lo ? lo : (t > hi ? hi : t);
}
// One cell of a trial's pass behind its evaluation: the full gradient g1 = g_data + lambda Wm (m1 - m_ref) (item_adapt_lr_grad) is written,
// and with s = m1 - m0, y = g1 - g0 (0 where there is no state yet: g0 == nullptr) the terms of g0's, s'y, s's, y'y and of the trial
// state's |pg|2^2 are added to acc[0 .. 5); returns the trial state's pg[a] (*bound: cell a is in its B)
HD double item_map_trial(const double* m0, const double* g0, const double* m1, double g1, double lo, double hi, long long a, double (&acc)[5], bool* bound) {
    if (g0) {
        const double s = m1[a] - m0[a], y = g1 - g0[a];
        acc[0] = fma(g0[a], s, acc[0]); acc[1] = fma(s, y, acc[1]); acc[2] = fma(s, s, acc[2]); acc[3] = fma(y, y, acc[3]);
    }
    *bound = item_map_bound(m1[a], g1, lo, hi);
    const double pg = *bound ? 0.0 : g1;
    acc[4] = fma(pg, pg, acc[4]);
    return pg;
}

}  // namespace hmcmt
