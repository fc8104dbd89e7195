/* hmcmt.h -- C ABI of libhmcmt_hip.so: the MI355X-native hot path of CUG-EMI/HMCMT2D.
 *
 * One context = one GPU = one HMC chain's worth of state.  A context is NOT thread-safe;
 * distinct contexts are independent.  All pointers are caller-owned; the library copies what it
 * needs during hmcmt_create and never retains host pointers.  Complex arrays are interleaved
 * (re, im) doubles: the memory layout of Julia's ComplexF64, numpy complex128 and C's
 * `double _Complex`.  Index arrays are 1-based int64, exactly as the reference stores them.
 *
 * Every function returns 0 on success or a negative HMCMT_E* code; it never throws or aborts.
 * hmcmt_last_error() gives the message of the last failure.  There is NO host compute path:
 * without a HIP device hmcmt_create fails with HMCMT_ENODEV.
 *
 * What each entry point replaces in the reference (/root/reference, all under HMCMT/src/):
 *
 *   hmcmt_create / hmcmt_destroy
 *       the per-run set-up the reference redoes inside every call: setupTensorMesh2D!
 *       (MTFwdSolver/MT2DOperators.jl:16-27), getBoundaryIndex (MT2DFwdSolver.jl:227-248),
 *       preSetRxFieldSens (MTSensitivity/sensUtils.jl:17-52), compDataWeightMat / activeCell
 *       plumbing (HMCStruct/HMCStruct.jl:99-125).
 *   hmcmt_grad   == compDataGradient(mtMesh, mtData, invParam, hmcprior)
 *       (HMCSampler/HMCSampler.jl:277-330): m = ln(sigma) on active cells ->
 *       (predData, dataMisfit, dataGrad); internally MT2DFwdSolver (MT2DFwdSolver.jl:74-216),
 *       compMT2DTE/TM (mt2DTE.jl:19-83, mt2DTM.jl:18-83), compJacTMatVec
 *       (MTSensitivity/compJacTMatVec.jl:8-327) and the MUMPS/UMFPACK factor+solve they call
 *       (MUMPS/src/MUMPSfuncs.jl:32,128; mt2DTE.jl:47-55).
 *   hmcmt_forward == MT2DFwdSolver + compDataMisfit as used by getHamiltonian
 *       (HMCSampler.jl:358-397, :498-507).
 *   hmcmt_leapfrog == proposeLeapfrog (HMCSampler.jl:206-269) with the trajectory kept on the
 *       device, plus the Hamiltonian terms getHamiltonian needs at the proposal.
 *   hmcmt_get_fields: exTE / hxTM of MT2DFwdData (MT2DFwdSolver.jl:44-53), reference node order.
 *   hmcmt_jacobian == compJacMat / compJacTMat (MTSensitivity/compJacMat.jl, compJacTMat.jl), explicit rows.
 *   hmcmt_linearize + hmcmt_jvp / hmcmt_jtvp / hmcmt_gn_hessvec: compJacMat(m) * v without J, compJacTMatVec with a free
 *       datVec (MTSensitivity/compJacTMatVec.jl:8), and the Gauss-Newton product Re(J^H W^2 J) v built from the two.
 */
#ifndef HMCMT_H
#define HMCMT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMCMT_OK          0
#define HMCMT_EINVAL     -1   /* bad argument (message says which) */
#define HMCMT_ENODEV     -2   /* no usable HIP device */
#define HMCMT_EHIP       -3   /* HIP runtime error */
#define HMCMT_ENOCONV   -10   /* an iterative solve hit maxit (cf. MUMPS -10 "singular", MUMPSfuncs.jl:59-73) */
#define HMCMT_EBREAKDOWN -11  /* Krylov breakdown / non-finite values (a NaN model would hang the reference, HMCSampler.jl:546-548) */
#define HMCMT_ENOMEM    -13   /* device allocation failed (cf. MUMPS -13) */

#define HMCMT_PRECOND_JACOBI 0
#define HMCMT_PRECOND_FDM    1   /* fast diagonalisation with a laterally averaged background */
#define HMCMT_PRECOND_FDM_JACOBI 2 /* damped point-Jacobi / FDM / point-Jacobi, symmetric product form (default) */

typedef struct hmcmt_ctx hmcmt_ctx;

typedef struct hmcmt_options {
    int32_t precond;      /* HMCMT_PRECOND_* ; default FDM_JACOBI */
    int32_t maxit;        /* iteration cap per solve; default 2000 (FDM) */
    double  tol;          /* stop when ||P^-1 r|| <= tol*||x|| (error estimate); default 1e-11 */
    int32_t check_every;  /* host convergence poll interval in iterations of the classic (non-default) solver loops; default 2.
                             The default path looks at a mapped counter once per iteration without waiting */
    int32_t verify;       /* 1: also compute true relative residuals ||b-Ax||/||b|| after each solve */
    int32_t warm_start;   /* initial guess of both solves: 0 zero, 1 the previous evaluation's fields, 2 (default) those
                             fields extrapolated along the model path from up to the last six evaluations (Lagrange
                             extrapolation over the nearly collinear part of the history; leapfrog trajectories are nearly
                             straight lines at nearly constant speed).  The adjoint solve starts from zero unless at least
                             three collinear points exist */
    int32_t fdm_precision;/* 0 (default): bf16 transforms (fp32 accumulate) + complex64 tridiagonal inside the
                             preconditioner; 1: fp64 throughout.  x, r, p and all inner products are fp64 either way */
} hmcmt_options;

typedef struct hmcmt_stats {
    int32_t iters_fwd_max, iters_adj_max;   /* max over systems of the last call */
    int32_t iters_fwd_sum, iters_adj_sum;   /* sum over systems */
    double  err_est_max;                    /* max over systems of ||P^-1 r||/||x|| at exit */
    double  true_res_max;                   /* max ||b-Ax||/||b|| (with options.verify, and in the guarded evaluations: hmcmt_guard) */
    int32_t status;                         /* 0 or HMCMT_ENOCONV / HMCMT_EBREAKDOWN */
    int32_t nsystems;                       /* 2*nFreq */
    int32_t fallback_solves;                /* solves of the last call (0..2) whose stragglers were restarted with the fp64
                                               preconditioner because the device's stagnation watch fired (a system that did
                                               not improve its error estimate 10-fold within 30 iterations) */
    int32_t smoother_sweeps;                /* damped Jacobi sweeps on each side of the FDM stage in the last call: 10 * (forward
                                               solve) + (adjoint solve), e.g. 11 or 22; chosen per solve unless HMCMT_SWEEPS is
                                               set (was `reserved_`: same offset, same size) */
} hmcmt_stats;

void hmcmt_default_options(hmcmt_options* opts);

/* Builds a context on HIP device `device_id`.
 *   ny, nz            cells in y / z (nz INCLUDES the air layers, TensorMesh2D.gridSize)
 *   yLen[ny], zLen[nz], origin[2]      TensorMesh2D fields (HMCFileIO.jl:45-60)
 *   freqs[nFreq]; rxY[nRx], rxZ[nRx]   MTData.freqs, columns of MTData.rxLoc
 *   compMode[nComp]   component code per entry of MTData.dataComp: 1 ZXY, 2 ZYX (DataType Impedance, complex data);
 *                     3 RhoXY, 4 PhsXY, 5 RhoYX, 6 PhsYX (DataType Rho_Pha: apparent resistivity |Z|^2/(w mu0) in Ohm-m and
 *                     phase in degrees, mt2DTE.jl:253-255 -- real data: obs / pred keep the complex layout with zero
 *                     imaginary parts).  The two families cannot be mixed.  The tipper T = Hz/Hy of the TE mode
 *                     (dataFuncSens.jl:44-112): 7 TZY (Impedance family, complex T), 8 RealTZY / 9 ImagTZY (Rho_Pha family,
 *                     Re T / Im T), listed after every other component; the response table per (freq, rx) is then the
 *                     impedance / rho-phase entries followed by the tipper entries.  A tipper-only set solves TE systems only.
 *                     HMCMT_EINVAL: a code outside 1..9, a tipper component of the other family or before a non-tipper one
 *   freqID/rxID/dtID[nData]  1-based, MTData fields; dataID[nComp*nRx*nFreq] mask, dt fastest
 *   obs[nData] complex, dataW[nData] = diag of InvDataModel.dataW
 *   activeIdx[nAC]    1-based cell id of each active cell (= activeCell.rowval), bgModel[ny*nz]
 *   opts              NULL for defaults
 * Limits: the one-launch-per-solve kernel runs meshes up to 415 cells wide (two column parts per row block beyond 207; nz up to
 * 225 rows at that width, more on narrower meshes: DESIGN 5.0, "Envelope"), all others four to six launches per iteration
 * (DESIGN 5.1).  options.fdm_precision = 1 needs ny + 1 <= 448 nodes (HMCMT_EINVAL otherwise: the fp64 eigen-transform of the
 * preconditioner holds 28 column tiles); wider meshes run the default mixed-precision path WITHOUT its fp64 safety net (a
 * stagnating solve then fails its evaluation with HMCMT_ENOCONV instead of being restarted);
 * hmcmt_persist_info tells which. */
int hmcmt_create(hmcmt_ctx** ctx, int32_t device_id,
                 int64_t ny, int64_t nz, const double* yLen, const double* zLen, const double* origin,
                 int64_t nFreq, const double* freqs,
                 int64_t nRx, const double* rxY, const double* rxZ,
                 int64_t nComp, const int64_t* compMode,
                 int64_t nData, const int64_t* freqID, const int64_t* rxID, const int64_t* dtID,
                 const uint8_t* dataID, const double* obs, const double* dataW,
                 int64_t nAC, const int64_t* activeIdx, const double* bgModel,
                 const hmcmt_options* opts);
int hmcmt_destroy(hmcmt_ctx* ctx);
const char* hmcmt_last_error(const hmcmt_ctx* ctx);   /* ctx may be NULL: create-time error */

int hmcmt_set_options(hmcmt_ctx* ctx, const hmcmt_options* opts);
int hmcmt_get_stats(const hmcmt_ctx* ctx, hmcmt_stats* out);
/* per-system iteration counts of the last call: iters[2*S] (forward, then adjoint) */
int hmcmt_get_iters(const hmcmt_ctx* ctx, int32_t* iters);

/* Host-buffer entry points (synchronous). pred: complex[nData]; grad: [nAC].
 * A model identical (bit for bit) to one of the last two evaluated through these entry points is answered from their
 * stored results without touching the GPU (a sampler re-evaluates the proposal's model and, after a rejection, the
 * previous start model); hmcmt_get_stats then reports zero iterations.  Dropped by hmcmt_set_options and when
 * options.verify is set. */
int hmcmt_grad(hmcmt_ctx* ctx, const double* m, double* pred, double* misfit, double* grad);
int hmcmt_forward(hmcmt_ctx* ctx, const double* m, double* pred, double* misfit);

/* Device-buffer entry points: all pointers are DEVICE pointers on the context's GPU; work is
 * enqueued on the context's stream and complete when the call returns. */
int hmcmt_grad_device(hmcmt_ctx* ctx, const double* d_m, double* d_pred, double* d_misfit, double* d_grad);
int hmcmt_forward_device(hmcmt_ctx* ctx, const double* d_m, double* d_pred, double* d_misfit);

/* Asynchronous variant for a device-resident caller (a leapfrog loop whose next model is computed on the device from
 * this gradient, bench.py): returns when the evaluation is ENQUEUED; the outputs are ordered on the context's stream.
 * The call still blocks at its two convergence polls, but not on the gradient assembly behind the adjoint solve, so
 * the host issues the next evaluation's boundary-value stage while the device finishes this one.  A solve that gives
 * up (iteration cap, breakdown) is seen at its poll and returned by the call itself -- nothing is built on it: no
 * adjoint solve on a failed forward solve, no gradient from a failed adjoint solve; the statistics of a successful
 * asynchronous evaluation are collected by the next evaluation on the context or by hmcmt_wait; between hmcmt_grad_device_async and hmcmt_wait only further
 * hmcmt_grad_device_async calls are allowed on the context. */
int hmcmt_grad_device_async(hmcmt_ctx* ctx, const double* d_m, double* d_pred, double* d_misfit, double* d_grad);
/* waits for everything enqueued on the context; returns the status of the last asynchronous evaluation */
int hmcmt_wait(hmcmt_ctx* ctx);

/* One leapfrog trajectory on the device (proposeLeapfrog, HMCSampler.jl:206-269; the mass of hmcmt_set_mass).
 *   m0, p0 [nAC]      current model / momentum (host)
 *   invM [nAC]        diagonal of M^-1 (HMCMT_MASS_DIAGONAL)
 *   mref [nAC]        prior reference model; Wm in CSR (rowptr[nAC+1], colind, val; 0-based int64)
 *   dt, L, regParam, lnSigMin, lnSigMax     as in HMCPrior
 * Outputs (host): m1, p1 [nAC]; pred complex[nData] and misfit at the proposal (what the next
 * getHamiltonian call would recompute, HMCSampler.jl:364); mnorm = 0.5*lambda*(m-mref)'Wm(m-mref);
 * nfevals = number of gradient evaluations performed (L+1). */
int hmcmt_set_prior(hmcmt_ctx* ctx, const double* mref, const int64_t* wm_rowptr,
                    const int64_t* wm_colind, const double* wm_val, const double* invM);
int hmcmt_leapfrog(hmcmt_ctx* ctx, const double* m0, const double* p0, double dt, int32_t L,
                   double regParam, double lnSigMin, double lnSigMax,
                   double* m1, double* p1, double* pred, double* misfit, double* mnorm,
                   int32_t* nfevals);

/* Mass matrix of hmcmt_leapfrog / hmcmt_leapfrog_device (runHMCSampler's choice by masstype, HMCSampler.jl:80-86).
 *   HMCMT_MASS_DIAGONAL  the invM of hmcmt_set_prior (default; every hmcmt_set_prior call returns to it)
 *   HMCMT_MASS_WM        M = Wm of hmcmt_set_prior (setMassMatrix(invParam), HMCSampler.jl:478-489): momentum p = L z with
 *                        L = chol(Wm).L in the natural order of the active cells, position step dm = dt Wm^-1 p (then the step
 *                        clamp and the reflection, which flips p), kinetic energy 0.5 p'Wm^-1 p.  hmcmt_set_mass factors Wm
 *                        (banded Cholesky on the host, bandwidth from the CSR; kept on the device, and kept for a later
 *                        hmcmt_set_prior with the same Wm): HMCMT_EINVAL if Wm is not positive definite.  Wm^-1 is a fast
 *                        diagonalisation in fp64 when the active cells fill a box below the air (Wm then separates,
 *                        kernels_mass.h), fp64 PCG on Wm otherwise (relative residual 1e-13, HMCMT_ENOCONV at its cap).
 *   HMCMT_MASS_LOWRANK   a diagonal plus a low-rank correction, set by hmcmt_set_mass_lowrank (hmcmt_set_mass refuses the kind):
 *                          M^-1 = S (I + U (Lambda - I) U') S,   M = F F',   F = S^-1 (I + U (Lambda^-1/2 - I) U')
 *                        with S = diag(sqrt(invM)), U nAC x rank with orthonormal columns and Lambda = diag(lambda) > 0 -- the
 *                        metric for a posterior whose covariance is about M^-1: a few strongly correlated directions (U, with
 *                        variances lambda in units of the scales) over per-cell scales.  Momentum p = F z, position step
 *                        dm = dt M^-1 p, kinetic energy 0.5 p'M^-1 p, on the route of HMCMT_MASS_WM; hmcmt_mass_apply gives
 *                        M^-1 x and F x.  One application is two fp64 kernels (kernels_mass.h), nothing waits.
 * hmcmt_mass_apply: y = M^-1 x (HMCMT_MASS_OP_INV) or y = L x (HMCMT_MASS_OP_SQRT; F x under HMCMT_MASS_LOWRANK) for the mass matrix that was set (for
 *   HMCMT_MASS_DIAGONAL: invM .* x and x ./ sqrt(invM)); x, y [nAC], host (on_device = 0, synchronous) or device pointers
 *   (on_device = 1, enqueued on the context's stream, complete on return).
 * hmcmt_set_mass_lowrank: invM [nAC] = s^2 (NULL: the diagonal in force, the invM of hmcmt_set_prior unless the chain replaced it),
 *   1 <= rank <= HMCMT_MASS_RANK_MAX, U [rank][nAC] (direction k contiguous), lambda [rank]; all host.  Like hmcmt_set_mass it needs
 *   a prior, waits for the stream and ENDS a running chain with its accumulators and adaptation.  HMCMT_EINVAL, with nothing
 *   changed, for a NULL U or lambda, a rank outside the range, a non-finite or non-positive invM or lambda entry, a non-finite U entry
 *   (all checked before anything is enqueued) and for max |U'U - I| > 1e-8 (checked on the device; a U from a QR or SVD sits near
 *   1e-12).  HMCMT_ENOMEM leaves the context on HMCMT_MASS_DIAGONAL.  The call keeps buffers of its own and never writes the prior's
 *   invM: hmcmt_set_mass(HMCMT_MASS_DIAGONAL) afterwards is the diagonal mass as it was, bit for bit; hmcmt_set_prior and
 *   hmcmt_set_mass release the buffers, a kept factor of Wm stays.  hmcmt_chain_set_mass_diag and an adaptation with adapt_mass are
 *   HMCMT_EINVAL under this mass, hmcmt_chain_set_dt and a step-size-only adaptation work.  hmcmt_mass_info reports the kind and 0 in
 *   its other fields. */
#define HMCMT_MASS_DIAGONAL 0
#define HMCMT_MASS_WM       1
#define HMCMT_MASS_LOWRANK  2
#define HMCMT_MASS_RANK_MAX 32
#define HMCMT_MASS_OP_INV   0
#define HMCMT_MASS_OP_SQRT  1
int hmcmt_set_mass(hmcmt_ctx* ctx, int32_t kind);
int hmcmt_set_mass_lowrank(hmcmt_ctx* ctx, const double* invM, int32_t rank, const double* U, const double* lambda);
int hmcmt_mass_apply(hmcmt_ctx* ctx, int32_t op, const double* x, double* y, int32_t on_device);

/* The same trajectory on DEVICE vectors: d_m, d_p [nAC] are updated in place (start model / momentum -> proposal), nothing
 * crosses PCIe.  start_grad says where the data gradient at the start model comes from:
 *   0  evaluate it (first trajectory of a chain, or a start model the context has not seen);
 *   1  the start model is the END model of the previous trajectory on this context (the proposal was accepted,
 *      HMCSampler.jl:155-163): its gradient is still on the device -- L new evaluations instead of L + 1;
 *   2  the start model is the START model of the previous trajectory (the proposal was rejected, :164-168).
 * d_pred complex[nData], d_misfit, d_mnorm (device, each may be NULL) receive the proposal's predicted data, data
 * misfit and 0.5*lambda*(m-mref)'Wm(m-mref).  Returns when the whole trajectory is enqueued and the solver status of
 * every evaluation -- the last one included: the call waits for its two solves' records, not for the gradient assembly,
 * the final momentum update and the Hamiltonian terms queued behind them -- has been checked; hmcmt_wait completes it
 * (and reports a non-finite model met on the way).  nfevals counts as the reference does (L + 1). */
int hmcmt_leapfrog_device(hmcmt_ctx* ctx, double* d_m, double* d_p, double dt, int32_t L, double regParam,
                          double lnSigMin, double lnSigMax, int32_t start_grad, double* d_pred, double* d_misfit,
                          double* d_mnorm, int32_t* nfevals);

/* The HMC chain on the device: one sample of runHMCSampler's loop (HMCSampler.jl:132-186) per hmcmt_chain_step, with the chain's
 * state -- current and proposal model, momentum, their predicted data -- and streaming posterior moments (Welford: what
 * getPosteriorModel, HMCSampler.jl:605-642, computes from the sample history) kept in device memory.  Random numbers stay with the
 * caller: standard normals for every momentum, one uniform per sample.  Per sample the host sends nAC normals and receives one record.
 *   hmcmt_chain_begin     after hmcmt_set_prior (and hmcmt_set_mass if M = Wm is wanted; HMCMT_EINVAL without a prior).  Uploads
 *                         m_start[nAC], runs one forward evaluation there (D0 = data misfit, the predicted data), computes
 *                         M0 = 0.5*regParam*(m-mref)'Wm(m-mref), zeroes moments and counters.  The chain's buffers are its own,
 *                         allocated here: HMCMT_ENOMEM leaves the context usable, without a chain.  A chain that is running is replaced
 *                         (its buffers are kept and zeroed: a second begin allocates nothing).
 *                         dt, regParam, lnSigMin, lnSigMax as in hmcmt_leapfrog; the first `burnin` samples stay out of the moments
 *                         (getPosteriorModel's burnin+1:nsamples).  D0, M0 may be NULL
 *   hmcmt_chain_momentum  getMomentumVector + getKineticEnergy (HMCSampler.jl:407-447): p = sqrtM * clip(z, +-2.5) for the mass that
 *                         is set -- z ./ sqrt(invM), or L z for HMCMT_MASS_WM -- and K = 0.5 p'M^-1 p (K may be NULL).  z: host [nAC]
 *   hmcmt_chain_step      copies the current model into the proposal buffer, runs the trajectory of L steps there (start gradient: evaluated
 *                         on the first step, else the one the previous decision left on the device), forms [K0, K1, D1, M1], waits once,
 *                         decides on the host -- accept iff hdif > 0 || u < exp(hdif), hdif = (D + M + K0) - (D1 + K1 + M1) -- and
 *                         enqueues the commit without waiting for it: current <-> proposal on acceptance, then the moments' update with the
 *                         chain's current model (also after a rejection: the sample repeats).  m_out [nAC] / pred_out complex[nData]
 *                         (host, each may be NULL): the chain's current model / predicted data AFTER the decision; with both NULL
 *                         nothing of O(nAC) or O(nData) leaves the device.  Needs a momentum set since the last step
 *   hmcmt_chain_state     current model [nAC], momentum buffer [nAC] (after a step: the proposal's momentum), current predicted data
 *                         complex[nData] -> host; each may be NULL
 *   hmcmt_chain_moments   count = samples in the moments, mean[nAC], m2[nAC] = sum of squared deviations from the mean (each may be
 *                         NULL); on_device = 0: host buffers, = 1: device pointers; complete on return.  The reference's standard
 *                         deviation is sqrt(max(m2/count, eps))
 *   hmcmt_chain_set_energy   replaces the D and M the chain holds for its current model -- what the next accept test adds to K0.  For a
 *                         host that restores a chain whose terms it has kept, and for the reference's own start: runHMCSampler computes the
 *                         first Hamiltonian at its homogeneous start model but runs the first trajectory from the file's model
 *                         (HMCSampler.jl:88 against :100-112), and a chain that is to take the reference's decisions does the same
 *   hmcmt_chain_end       releases the chain's buffers (hmcmt_destroy does it too)
 * record.nfevals: the gradient evaluations the step performed -- L + 1 when it evaluated its start gradient, L when it reused one
 *   (hmcmt_leapfrog_device's count, less the reused gradient).
 * State rules.  A chain call evaluates: it ends a linearisation point (hmcmt_linearize).  Any other evaluating call, hmcmt_leapfrog* or
 *   hmcmt_set_options on the context between two steps is allowed: the context counts its evaluations, the chain compares the count with
 *   the one it left, and the next step then evaluates its start gradient again instead of trusting the one on the device (nfevals = L + 1).
 *   hmcmt_set_prior / hmcmt_set_mass END the chain: later chain calls return HMCMT_EINVAL until a new hmcmt_chain_begin.  Between
 *   hmcmt_grad_device_async and hmcmt_wait every chain call returns HMCMT_EINVAL.
 * A step whose trajectory fails (HMCMT_ENOCONV, HMCMT_EBREAKDOWN, a non-finite model) returns that code; the chain stays exactly where
 *   it was -- current model, predicted data, D, M, counters, moments --, the momentum counts as consumed, the next step evaluates its
 *   start gradient.  Whether that is a rejection is the caller's decision.
 * HMCMT_EINVAL also: no chain, no momentum since the last step, L < 1, a NULL or non-finite argument.
 * A chain is bitwise repeatable: the same history of the context and the same inputs give the same bits in every record and moment. */
typedef struct hmcmt_chain_record {
    int32_t accepted;      /* 1 / 0 */
    int32_t nfevals;       /* gradient evaluations of this step */
    double  K0, K1;        /* kinetic energy at the start / at the proposal */
    double  D1, M1;        /* data misfit and 0.5*lambda*(m-mref)'Wm(m-mref) at the proposal */
    double  D, M;          /* the chain's current state AFTER the decision */
    double  hdif;          /* H(start) - H(proposal), what the accept test saw */
    int64_t nsamples;      /* samples committed so far */
    int64_t nmoments;      /* ... those behind the burn-in: in the moments */
} hmcmt_chain_record;
int hmcmt_chain_begin(hmcmt_ctx* ctx, const double* m_start, double dt, double regParam, double lnSigMin, double lnSigMax,
                      int64_t burnin, double* D0, double* M0);
int hmcmt_chain_momentum(hmcmt_ctx* ctx, const double* z, double* K);
int hmcmt_chain_step(hmcmt_ctx* ctx, int32_t L, double u, hmcmt_chain_record* rec, double* m_out, double* pred_out);
int hmcmt_chain_set_energy(hmcmt_ctx* ctx, double D, double M);
int hmcmt_chain_state(hmcmt_ctx* ctx, double* m_cur, double* p_cur, double* pred_cur);
int hmcmt_chain_moments(hmcmt_ctx* ctx, int64_t* count, double* mean, double* m2, int32_t on_device);
int hmcmt_chain_end(hmcmt_ctx* ctx);

/* Marginal posteriors from the chain's commit (optional; nothing above changes when they are off).  Two accumulators, each fed by the
 * commits that fall behind the burn-in -- the samples of the moments, a rejection's repeat included -- from its own begin call on, each
 * with its own count.  A begin call may come at any point between two steps; only later commits count.
 *   hmcmt_chain_hist_begin   per-cell histograms of m = ln sigma (the reference's sitePPD, HMCSampler.jl:646-680): target[ntarget] are
 *                         0-based indices into the active cells, repeats allowed (two depths in one cell are two rows), ntarget >= 1,
 *                         1 <= nbins <= 4096, lo < hi finite.  Every counted commit adds 1 to ONE bin of every target's row:
 *                             t = (m[target] - lo) * scale,  scale = (double)nbins / (hi - lo)   (one subtraction, then one product)
 *                             b = t < 0 ? 0 : t >= nbins ? nbins - 1 : (int)t
 *                         -- values outside [lo, hi) are CLAMPED into the edge bins, so every row sums to the count.  Allocates
 *                         ntarget * nbins zeroed uint32 counters and the target list on the device; on HMCMT_ENOMEM the chain goes on
 *                         without a histogram.  A second call replaces the first histogram
 *   hmcmt_chain_hist      count = commits in the histogram, counts[ntarget][nbins] (target-major; each may be NULL); on_device = 0: host
 *                         buffer, = 1: device pointer; complete on return
 *   hmcmt_chain_hist_quantiles   out[nq][ntarget] (host, or a device pointer with on_device = 1) for q[nq] (host), every q in [0, 1],
 *                         computed on the device from the counters.  With N = count and x = q * (double)N: b is the first bin with
 *                         count_b > 0 whose inclusive cumulative count cum_b >= x, and the value is
 *                             lo + w * (b + (x - cum_{b-1}) / count_b),  w = (hi - lo) / nbins
 *                         -- linear inside the bin.  HMCMT_EINVAL when N = 0
 *   hmcmt_chain_data_moments_begin / hmcmt_chain_data_moments   Welford mean and m2 of the chain's current predicted data: 2 nData
 *                         doubles each, re and im interleaved as in pred_out (real data types: exact zeros in the imaginary slots);
 *                         count, mean, m2 may each be NULL, on_device as above
 * hmcmt_chain_begin (also over a running chain), hmcmt_chain_end, hmcmt_set_prior and hmcmt_set_mass end both accumulators and release
 * their buffers; a step that fails touches neither.  HMCMT_EINVAL: NULL context, target, q or out, a size, range or index outside
 * the above, no chain, no accumulator begun, a call between hmcmt_grad_device_async and hmcmt_wait.  Counts, quantiles and data
 * moments repeat bitwise (every counter row and every datum has one owner thread: no atomics). */
extern int hmcmt_chain_hist_begin(hmcmt_ctx* ctx, int64_t ntarget, const int64_t* target, int32_t nbins, double lo, double hi);
extern int hmcmt_chain_hist(hmcmt_ctx* ctx, int64_t* count, uint32_t* counts, int32_t on_device);
extern int hmcmt_chain_hist_quantiles(hmcmt_ctx* ctx, int32_t nq, const double* q, double* out, int32_t on_device);
extern int hmcmt_chain_data_moments_begin(hmcmt_ctx* ctx);
extern int hmcmt_chain_data_moments(hmcmt_ctx* ctx, int64_t* count, double* mean, double* m2, int32_t on_device);

/* Effective sample size from the chain's commit (optional, a third accumulator under the rules above: fed by the commits behind the
 * burn-in from its begin call on, a rejection's repeat included, with its own count N; nothing above changes when it is off).
 *   hmcmt_chain_acov_begin   per-cell lagged autocovariances of m = ln sigma for the lags 0 .. K = maxlag, 1 <= maxlag <= 1023.
 *                         target[ntarget] are 0-based active-cell indices, repeats allowed (rows of their own); target = NULL with
 *                         ntarget = 0: every active cell, in order.  Counted commits are t = 0, 1, ...; per target, with the pivot
 *                         x0 = the value at t = 0 and y_t = m[target] - x0 (one subtraction), the device holds
 *                             tot = sum y_t (serial adds),  S_k = sum_{t >= k} y_t y_{t-k} (S_k = fma(y_t, y_{t-k}, S_k)),
 *                             H_k = sum_{t < k} y_t (serial adds),  and a ring of the last K + 1 values y
 *                         -- about (3 (K + 1) + 2) * 8 bytes per target, zeroed here.  On HMCMT_ENOMEM the chain goes on without the
 *                         accumulator.  A second call replaces the first accumulator
 *   hmcmt_chain_acov      count = N, mean[ntarget], acov[(K + 1)][ntarget] (LAG-MAJOR, the device's layout; each may be NULL);
 *                         on_device as for hmcmt_chain_hist; complete on return.  With ybar = tot / N, T_k the sum of the last k
 *                         values y added newest first, A_k = tot - H_k and B_k = tot - T_k:
 *                             c_k = (S_k - ybar (A_k + B_k) + (N - k) ybar^2) / N  for k < N,  c_k = 0 for k >= N,  mean = x0 + ybar
 *                         -- the biased estimator c_k = (1/N) sum_{t=k}^{N-1} (x_t - xbar)(x_{t-k} - xbar); a cell that never moved
 *                         gives c_k == 0.0 exactly.  HMCMT_EINVAL when N = 0 and mean or acov is asked for
 *   hmcmt_chain_ess       tau[ntarget], ess[ntarget], window[ntarget] (each may be NULL), computed on the device by Geyer's initial
 *                         positive sequence: Gamma_m = (c_2m + c_2m+1) / c_0 for m = 0 .. floor((min(K, N - 1) - 1) / 2), summed while
 *                         Gamma_m > 0, M pairs; tau = -1 + 2 sum Gamma_m (reported raw); ess = min(N / tau, N max(1, log10 N)), the
 *                         cap also when tau <= 1 / max(1, log10 N); window = M if a non-positive pair ended the sum, -M if the lags
 *                         ran out first (tau is then a lower bound).  A cell with c_0 > 0 false is constant: tau = N, ess = 1,
 *                         window = 0.  HMCMT_EINVAL when N = 0
 * hmcmt_chain_begin (also over a running chain), hmcmt_chain_end, hmcmt_set_prior and hmcmt_set_mass end the accumulator and release
 * its buffers; a step that fails touches nothing.  HMCMT_EINVAL: NULL context, a size, lag or index outside the above, no chain, no
 * accumulator begun, a call between hmcmt_grad_device_async and hmcmt_wait.  Results repeat bitwise (every (target, lag) has one
 * owner thread: no atomics). */
extern int hmcmt_chain_acov_begin(hmcmt_ctx* ctx, int64_t ntarget, const int64_t* target, int32_t maxlag);
extern int hmcmt_chain_acov(hmcmt_ctx* ctx, int64_t* count, double* mean, double* acov, int32_t on_device);
extern int hmcmt_chain_ess(hmcmt_ctx* ctx, double* tau, double* ess, int32_t* window, int32_t on_device);

/* Posterior covariance and correlation from the chain's commit (optional, a fourth accumulator under the rules above: fed by the
 * commits behind the burn-in from its begin call on, a rejection's repeat included, with its own count N; nothing above changes
 * when it is off, and every record, model, moment, histogram and autocovariance keeps its bits when it is on).
 *   hmcmt_chain_cov_begin  cross moments of m = ln sigma between the cells row[nrow] (0-based active-cell indices, repeats allowed
 *                         and rows of their own) and every active cell; row = NULL with nrow = 0: every active cell in order, the
 *                         full matrix.  batch = 1 .. HMCMT_COV_BATCH_MAX commits are parked before one kernel folds them into S
 *                         (0: the default, 8); the results do not depend on it, bit for bit.  Counted commits are t = 0, 1, ...;
 *                         per cell a, with the pivot x0[a] = the value at t = 0 and y_t[a] = m[a] - x0[a] (one subtraction), the
 *                         device holds
 *                             tot[a] = sum y_t[a] (serial adds),  q[a] = fma(y_t[a], y_t[a], q[a]),
 *                             S[r][a] = fma(y_t[row[r]], y_t[a], S[r][a])  in commit order,  and the y of up to `batch` commits
 *                         -- about 8 (nrow + batch + 3) nAC bytes, zeroed here.  On HMCMT_ENOMEM the chain goes on without the
 *                         accumulator.  A second call replaces the first accumulator
 *   hmcmt_chain_cov       count = N, mean[nAC], var[nAC], cov[nrow][nAC] (row-major; each may be NULL); on_device as for
 *                         hmcmt_chain_acov; complete on return.  With N as a double and rho = row[r]:
 *                             mean[a] = x0[a] + tot[a] / N,   var[a] = (q[a] - (tot[a] tot[a]) / N) / N,
 *                             cov[r][a] = (S[r][a] - (tot[rho] tot[a]) / N) / N
 *                         -- the biased estimator (1/N) sum (x_rho - xbar_rho)(x_a - xbar_a), the convention of c_0 above.
 *                         cov[r][row[r]] == var[row[r]] bitwise; with the full matrix cov equals its transpose bitwise; a cell that
 *                         never moved gives exact zeros in its row and column.  HMCMT_EINVAL when N = 0 and an array is asked for
 *   hmcmt_chain_corr      corr[nrow][nAC] = cov[r][a] / sqrt(var[rho] var[a]) clamped into [-1, 1], computed on the device; 0.0
 *                         where var[rho] > 0 && var[a] > 0 is false; corr[r][row[r]] == 1.0 for a cell that moved.  HMCMT_EINVAL
 *                         when N = 0
 * hmcmt_chain_begin (also over a running chain), hmcmt_chain_end, hmcmt_set_prior and hmcmt_set_mass end the accumulator and release
 * its buffers; a step that fails touches nothing.  HMCMT_EINVAL: NULL context, a size, batch or index outside the above, no chain, no
 * accumulator begun, a call between hmcmt_grad_device_async and hmcmt_wait.  Results repeat bitwise (every S[r][a] has one owner
 * thread: no atomics). */
#define HMCMT_COV_BATCH_MAX 16
extern int hmcmt_chain_cov_begin(hmcmt_ctx* ctx, int64_t nrow, const int64_t* row, int32_t batch);
extern int hmcmt_chain_cov(hmcmt_ctx* ctx, int64_t* count, double* mean, double* var, double* cov, int32_t on_device);
extern int hmcmt_chain_corr(hmcmt_ctx* ctx, double* corr, int32_t on_device);

/* Posterior principal components from the chain's commit by a row sketch (optional, a fifth accumulator under the rules above: fed
 * by the commits behind the burn-in from its begin call on, a rejection's repeat included, with its own count N; nothing above
 * changes when it is off, and every record, model, moment, histogram, autocovariance and cross moment keeps its bits when it is on).
 * The method is frequent directions (Liberty 2013; Ghashami, Liberty, Phillips, Woodruff 2016): 2 ell rows of nAC doubles stand for
 * the N x nAC matrix A of the rows y_t, with a deterministic error bound that every read-out reports.
 *   hmcmt_chain_sketch_begin  2 <= ell <= HMCMT_SKETCH_ELL_MAX.  pivot[nAC] (host, finite) or NULL: the model of the first counted
 *                         commit, the convention of the accumulators above; sketches of several chains can be merged only under one
 *                         given pivot.  Allocates and zeroes B[2 ell + 1][nAC], x0, tot, q[nAC] and the staging of the Gram matrix
 *                         ([2 ell + 1]^2) and of the coefficients -- about 8 (2 ell + 4) nAC bytes.  On HMCMT_ENOMEM the chain goes on
 *                         without the sketch.  A second call replaces the first sketch
 *       Per counted commit t = 0, 1, ... one kernel, one thread per cell a:
 *           y = m[a] - x0[a] (one subtraction);  tot[a] += y;  q[a] = fma(y, y, q[a]);  B[fill][a] = y;   then ++fill.
 *       The shrink, when fill == 2 ell, in the same call:
 *         a. device: K = B B' over the rows 0 .. 2 ell - 1 in fp64, every entry ONE fma chain over the cells upwards from 0, no atomics;
 *         b. ONE wait and one download of K (at most 128 KB);
 *         c. host, double: cyclic Jacobi (the warm-up estimator's), the eigenvalues taken descending d_0 >= d_1 >= ...;
 *            delta = max(d_ell, 0);  c_i = d_i > delta ? sqrt((d_i - delta) / d_i) : 0 for i < ell;  T[i][j] = c_i V[j][i] ([ell][2 ell]);
 *            Delta += delta;  ++shrinks;
 *         d. device: T is uploaded; B'[i][a] = sum_j T[i][j] B[j][a], j upwards by fma from 0, IN PLACE: the thread that owns cell a
 *            has copied all of column a aside before it writes any of it; rows ell .. 2 ell - 1 are zeroed and fill = ell.
 *       So the sketch adds one wait per ell counted commits and none otherwise.  A HIP error in a shrink is handled as at a window end
 *       of the low-rank warm-up: the sample stands, its call returns HMCMT_EHIP, the sketch is ended.  An eigensolver that does not
 *       converge within its 64 sweeps (or a Gram matrix that is not finite) ends the sketch too, the call returns what it would have;
 *       the read-outs below then return HMCMT_EINVAL with a message that says so.
 *       The guarantee, in exact arithmetic: 0 <= A'A - B'B <= Delta I in the positive semidefinite order, and
 *       Delta <= |A - A_k|_F^2 / (ell - k) for every k < ell (A_k the best rank-k approximation of A).
 *   hmcmt_chain_sketch    info (may be NULL) = {count N, ell, fill, shrinks, Delta, pivot_given}; mean[nAC] = x0 + tot / N and
 *                         var[nAC] = (q - (tot tot) / N) / N in the formulas of hmcmt_chain_cov; rows[fill][nAC], the sketch as it
 *                         stands, unshrunk rows included (room for 2 ell rows).  Each may be NULL; on_device as for hmcmt_chain_cov;
 *                         complete on return; nothing is changed by reading.  HMCMT_EINVAL when N = 0 and an array is asked for
 *   hmcmt_chain_pca       the leading eigenpairs of the centred covariance estimate (B'B - N ybar ybar') / N, ybar = tot / N;
 *                         1 <= rank <= HMCMT_MASS_RANK_MAX.  Device: row 2 ell of B = sqrt(N) ybar; G = W W' over W = the filled rows
 *                         and that row (the shrink's Gram kernel).  One wait, then host: G = Q Lambda Q' keeping the m values
 *                         Lambda_i > 1e-10 Lambda_max; S = Lambda^1/2 Q' J Q Lambda^1/2 with J = diag(1, ..., 1, -1), symmetrised;
 *                         S = Z Theta Z'; the min(rank, #theta > 0) largest theta are kept, descending, the lower index first among
 *                         equals; coefficients Q Lambda^-1/2 Z_sel.  Device: U[k][a] = sum_i coef[i][k] W[i][a], i upwards by fma; a
 *                         direction's entry of largest magnitude (the lowest index among equals) is positive; the orthonormality
 *                         defect max |U U' - I| is computed as hmcmt_set_mass_lowrank computes it.  *kept = the directions returned,
 *                         lambda[kept] = theta_k / N, U[kept][nAC] (room for rank rows; lambda and U may be NULL, device pointers with
 *                         on_device), *err = Delta / N (may be NULL; kept and err are always host).  Every returned lambda[k] lies
 *                         within err of the k-th eigenvalue of the exact centred covariance of the counted commits, in exact
 *                         arithmetic: Weyl's inequality on the guarantee above, since both matrices subtract the same rank-one term.
 *                         It does not change the sketch (it writes the staging row 2 ell, which no commit reads), so two calls in a
 *                         row return the same bytes.  HMCMT_EINVAL for N < 2; HMCMT_EBREAKDOWN for a defect above 1e-8, a Gram matrix
 *                         that is not finite or an eigensolver that did not converge
 * hmcmt_chain_begin (also over a running chain), hmcmt_chain_end, hmcmt_set_prior and hmcmt_set_mass end the sketch and release its
 * buffers; a step that fails touches nothing.  HMCMT_EINVAL: NULL context, ell or rank outside the above, a non-finite pivot, no chain,
 * no sketch begun, a call between hmcmt_grad_device_async and hmcmt_wait.  Results repeat bitwise (every sum has one owner thread and
 * one order: no atomics). */
#define HMCMT_SKETCH_ELL_MAX 64
typedef struct hmcmt_sketch_info {
    int64_t count;         /* N: counted commits in the sketch */
    int32_t ell, fill;     /* fill: rows in use, 0 .. 2 ell - 1 */
    int64_t shrinks;
    double  Delta;         /* sum of the shrinks' delta: the bound on A'A - B'B */
    int32_t pivot_given, reserved_;
} hmcmt_sketch_info;
extern int hmcmt_chain_sketch_begin(hmcmt_ctx* ctx, int32_t ell, const double* pivot);
extern int hmcmt_chain_sketch(hmcmt_ctx* ctx, hmcmt_sketch_info* info, double* mean, double* var, double* rows, int32_t on_device);
extern int hmcmt_chain_pca(hmcmt_ctx* ctx, int32_t rank, int32_t* kept, double* lambda, double* U, double* err, int32_t on_device);

/* The chain's step size and diagonal mass between two steps, and their warm-up adaptation (optional: with no call below, every
 * record, moment and accumulator keeps its bits).
 *   hmcmt_chain_set_dt    replaces the chain's dt (finite, > 0) between two steps.  The chain, its accumulators, a momentum already
 *                         drawn and the gradient the last decision left on the device stay valid: none depends on dt.  HMCMT_EINVAL
 *                         while an adaptation is active
 *   hmcmt_chain_set_mass_diag   replaces the diagonal of M^-1 (invM[nAC], host; every entry finite and > 0, checked before anything is
 *                         enqueued) without ending the chain.  A momentum drawn before the call is dropped -- its K0 belongs to the old
 *                         mass -- so the next hmcmt_chain_step fails with "no momentum since the last step" until a new one is drawn;
 *                         the stored gradient and D, M stay valid.  HMCMT_EINVAL with HMCMT_MASS_WM and while an adaptation with
 *                         adapt_mass is active
 *   hmcmt_chain_mass_diag reads out the diagonal in force: invM[nAC], host or with on_device = 1 a device pointer; complete on return
 *   hmcmt_chain_adapt_begin   starts a warm-up of nwarmup steps, counted from this call; a step counts when hmcmt_chain_step succeeds.
 *                         With c the steps adapted so far and W = nwarmup, a counted step does, behind its decision and its commit
 *                         (both unchanged):
 *                           1. alpha = hdif > 0 ? 1 : exp(hdif) from the record's hdif
 *                           2. with adapt_mass and init_buffer <= c < W - term_buffer: the chain's current model -- after the decision,
 *                              so a rejection repeats it -- is added to the window's Welford accumulator (two nAC buffers of the
 *                              adaptation's own, not the chain's moments, which stay behind the burn-in)
 *                           3. dual averaging of x = ln dt in double, in this order, t = updates since the last restart + 1:
 *                                eta = 1 / (t + t0),  s_bar = (1 - eta) s_bar + eta (delta - alpha),  x = mu - s_bar sqrt(t) / gamma,
 *                                x_eta = pow(t, -kappa),  x_bar = (1 - x_eta) x_bar + x_eta x,  dt = exp(x)
 *                              dt clipped into [dt_min, dt_max] where set (x is held to +-700 before exp).  The begin call restarts:
 *                              mu = ln(10 dt), s_bar = x_bar = 0
 *                           4. if 2. ran and c is the window's last step, with n samples in the window: for n >= 2 one kernel writes
 *                                invM[a] = (m2[a] / (n - 1)) w + f,  w = n / (n + 5),  f = 1e-3 * 5 / (n + 5)
 *                              windows_done is incremented and the dual averaging restarts around the dt of 3.; a window of n < 2
 *                              leaves the mass and the dual averaging alone.  Either way the window's accumulator is zeroed and the
 *                              next window follows Stan's rule: the first ends at step init_buffer + base_window - 1; behind the
 *                              window that ends at W - term_buffer - 1 there is none (next_window_end = -1); otherwise the size
 *                              doubles, next = c + size, and if next != W - term_buffer - 1 and next + 2 size >= W - term_buffer the
 *                              window runs up to W - term_buffer - 1
 *                           5. ++c; at c == W: dt = exp(x_bar), clipped (dt stays if a restart fell on the last step), active = 0
 *                         All of it is enqueued on the context's stream or scalar host work: the step keeps its single wait, and the
 *                         next hmcmt_chain_momentum sees the new mass.  A step that fails touches nothing of the adaptation.  The
 *                         adapted diagonal is the context's diagonal mass from then on: hmcmt_leapfrog* and hmcmt_mass_apply see it
 *                         until the next hmcmt_set_prior.  On HMCMT_ENOMEM the chain goes on without adaptation.  A second call
 *                         replaces a running adaptation
 *   hmcmt_chain_adapt_info   during an adaptation and after one that ended in this chain.  step = c, window_count = samples in the open
 *                         window, dt = the step size the next step uses, dt_bar = exp(x_bar) clipped (dt before the first update
 *                         behind a restart), alpha_last / alpha_sum = the last alpha and the sum of all
 *   hmcmt_chain_adapt_end stops now: dt = exp(x_bar) as at the regular end; the mass stays as the last closed window left it
 * hmcmt_chain_begin (also over a running chain), hmcmt_chain_end, hmcmt_set_prior and hmcmt_set_mass end an adaptation and release its
 * buffers.  HMCMT_EINVAL: NULL context or argument, no chain, a call between hmcmt_grad_device_async and hmcmt_wait, a non-finite
 * value; for the begin call nwarmup < 1, delta outside (0, 1), gamma or t0 not positive, kappa outside (0.5, 1], dt_min > dt_max with
 * both set, a negative bound, and with adapt_mass: HMCMT_MASS_WM, a negative buffer, base_window < 1 or
 * init_buffer + base_window + term_buffer > nwarmup; for info and end: no adaptation begun in this chain.  For equal inputs the
 * adapted dt and mass repeat bitwise. */
typedef struct hmcmt_adapt_options {
    int64_t nwarmup;                               /* steps to adapt over, counted from the begin call; >= 1 */
    int32_t adapt_mass;                            /* 1: windowed estimate of diag(M^-1) (HMCMT_MASS_DIAGONAL only); 0: step size only */
    int32_t init_buffer, term_buffer, base_window; /* defaults 75, 50, 25 */
    double  delta, gamma, t0, kappa;               /* defaults 0.8, 0.05, 10, 0.75 */
    double  dt_min, dt_max;                        /* clip of dt; 0 = no bound on that side */
} hmcmt_adapt_options;
typedef struct hmcmt_adapt_info {
    int64_t step, nwarmup, window_count, next_window_end;
    int32_t active, windows_done;
    double  dt, dt_bar, mu, s_bar, alpha_last, alpha_sum;
} hmcmt_adapt_info;
extern int hmcmt_chain_set_dt(hmcmt_ctx* ctx, double dt);
extern int hmcmt_chain_set_mass_diag(hmcmt_ctx* ctx, const double* invM);
extern int hmcmt_chain_mass_diag(hmcmt_ctx* ctx, double* invM, int32_t on_device);
extern void hmcmt_default_adapt_options(hmcmt_adapt_options* o);   /* nwarmup = 0: the caller sets it; adapt_mass = 1 */
extern int hmcmt_chain_adapt_begin(hmcmt_ctx* ctx, const hmcmt_adapt_options* o);
extern int hmcmt_chain_adapt_info(hmcmt_ctx* ctx, hmcmt_adapt_info* info);
extern int hmcmt_chain_adapt_end(hmcmt_ctx* ctx);

/* Low-rank mass in the warm-up: the directions U and factors Lambda of HMCMT_MASS_LOWRANK (above: M^-1 = S (I + U (Lambda - I) U') S)
 * estimated inside the adaptation, from the window's draws AND the gradients the decisions leave on the device.  For a Gaussian the
 * gradients are A^-1 (x - mu), and the symmetric positive definite Sigma with Sigma cov(grad) Sigma = cov(draws) is the covariance
 * itself; the sampling noise of the two covariances, which at n << nAC swamps the eigenvalues of cov(draws) alone, cancels (the metric
 * nutpie adapts with).
 *   hmcmt_chain_adapt_lowrank   upgrades a running adaptation begun with adapt_mass = 1; called after hmcmt_chain_adapt_begin and before
 *                         that adaptation's first counted step.  It allocates two row stores [max_samples][nAC] (draws, gradients), the
 *                         Gram buffer [2 max_samples]^2, staging for s, U and the coefficients, and the mass's own low-rank buffers for
 *                         `rank` directions: (2 max_samples + 2 rank + 7) nAC doubles.  HMCMT_EINVAL, with nothing changed: no such adaptation,
 *                         one that has counted a step, a value out of range or not finite.  HMCMT_ENOMEM leaves the diagonal adaptation
 *                         running as it was.
 *                         Per counted step inside a window (2. above), behind the Welford kernel and with no wait: with L the window's
 *                         length, known when it opens, stride = ceil(L / max_samples) (1 for L <= max_samples), and the window's i-th
 *                         step stores a pair when i % stride == 0: the chain's current model and the full potential gradient there,
 *                         g = g_data + regParam Wm (m - m_ref), g_data the data gradient the decision left on the device (the one the
 *                         next step's start reuses; a NUTS sample's selected state's).  A rejection repeats a pair.  Were no valid
 *                         gradient held, the pair would be skipped and counted, nothing evaluated for its sake; a decision always
 *                         leaves one, also behind a foreign evaluation on the context (the step then evaluated its own start gradient).
 *                         At a window's end (4. above), behind the kernel that writes invM, with n stored pairs, s = sqrt(invM) of
 *                         that kernel, W = [Zd; Zg], Zd = (X - mean X) / s / sqrt(n - 1), Zg = (G - mean G) s / sqrt(n - 1), the means
 *                         over the stored rows in row order:
 *                           a. device: K = W W' ([2n][2n], fp64, every entry one fma chain over the cells upwards, no atomics)
 *                           b. ONE WAIT and one download of K (at most 512 KB) -- once per window end, never per step
 *                           c. host, double, cyclic Jacobi throughout: K = V D V', the m values D_i > 1e-10 D_max kept,
 *                              T = D^-1/2 V';  Pd = T K[:, :n], Pg = T K[:, n:];  Cd = Pd Pd' + gamma I, Cg = Pg Pg' + gamma I;
 *                              Sigma = Cg^-1/2 (Cg^1/2 Cd Cg^1/2)^1/2 Cg^-1/2, symmetrised, = Y Theta Y';  the directions with
 *                              theta > cutoff or theta < 1 / cutoff, by |ln theta| descending (the lower index first among equals), at
 *                              most `rank`;  B = T' Y_sel ([2n][r])
 *                           d. device: B up, U[k][a] = sum_i B[i][k] W[i][a] (i upwards by fma), then each direction's sign so that its
 *                              entry of largest magnitude is positive (the lowest index among equals); the orthonormality check of
 *                              hmcmt_set_mass_lowrank on the staged U (its read-back is a second, short wait of the window end)
 *                           e. r >= 1 and defect <= 1e-8: s, U, lambda = theta are copied into the mass's buffers and the kind becomes
 *                              HMCMT_MASS_LOWRANK; r = 0 or a fallback (fewer than 4 pairs, defect above 1e-8, a non-finite value, an eigensolver
 *                              that did not converge within 64 sweeps): the
 *                              kind is HMCMT_MASS_DIAGONAL with the new invM and the directions of an earlier window are dropped
 *                         Either way the dual averaging restarts and the stores rewind, as the diagonal adaptation does.  A HIP error at a
 *                         window end is no fallback: the window ends on the diagonal, the sample stands, and its call returns HMCMT_EHIP.  The diagonal
 *                         kernel keeps writing the context's invM, so hmcmt_chain_mass_diag stays truthful.  At the end of the warm-up
 *                         the mass stays as the last window left it, until the next hmcmt_set_prior or hmcmt_set_mass.
 *   hmcmt_chain_adapt_lowrank_info   the last closed window: windows closed so far, pairs stored, stride, skipped, dims (m), rank kept,
 *                         theta_min / theta_max over all m, defect = max |U U' - I| as measured (0 with no direction), fallback,
 *                         host_ms of step c.  HMCMT_EINVAL without an upgraded adaptation in this chain
 *   hmcmt_chain_set_mass_lowrank   the between-steps twin of hmcmt_chain_set_mass_diag: the arguments and checks of
 *                         hmcmt_set_mass_lowrank (orthonormality included, complete before anything changes), but the chain goes on:
 *                         a momentum already drawn is dropped; the stored gradient, D and M and every accumulator stay.  rank = 0 with
 *                         invM (U, lambda ignored) sets a plain diagonal and returns the kind to HMCMT_MASS_DIAGONAL.  invM NULL with rank >= 1:
 *                         the scales in force.  HMCMT_EINVAL
 *                         under HMCMT_MASS_WM and while an adaptation of the mass is active.  It exists so that an adapted run can be
 *                         replayed from its record
 *   hmcmt_chain_mass_lowrank   reads out the mass in force: *rank (0 under the diagonal mass, then only invM is written), invM [nAC],
 *                         U [*rank][nAC] (room for HMCMT_MASS_RANK_MAX rows), lambda [*rank]; host, or device pointers for invM, U and
 *                         lambda with on_device = 1 (rank is always a host pointer); any of invM, U, lambda may be NULL */
typedef struct hmcmt_adapt_lowrank_options {
    int32_t rank;          /* most directions kept, 1 .. HMCMT_MASS_RANK_MAX; default 8 */
    int32_t max_samples;   /* most (draw, gradient) pairs stored per window, 4 .. 128; default 64 */
    double  cutoff;        /* keep theta > cutoff or theta < 1/cutoff; > 1; default 2 */
    double  gamma;         /* added to both projected covariances; > 0; default 1e-5 */
} hmcmt_adapt_lowrank_options;
typedef struct hmcmt_adapt_lowrank_info {
    int32_t windows, stored, skipped, dims, rank, fallback;
    int64_t stride;
    double  theta_min, theta_max, defect, host_ms;
} hmcmt_adapt_lowrank_info;
extern void hmcmt_default_adapt_lowrank_options(hmcmt_adapt_lowrank_options* o);
extern int hmcmt_chain_adapt_lowrank(hmcmt_ctx* ctx, const hmcmt_adapt_lowrank_options* o);
extern int hmcmt_chain_adapt_lowrank_info(hmcmt_ctx* ctx, hmcmt_adapt_lowrank_info* info);
extern int hmcmt_chain_set_mass_lowrank(hmcmt_ctx* ctx, const double* invM, int32_t rank, const double* U, const double* lambda);
extern int hmcmt_chain_mass_lowrank(hmcmt_ctx* ctx, int32_t* rank, double* invM, double* U, double* lambda, int32_t on_device);

/* The chain's own random numbers: a seeded chain draws its momenta on the device and its L and u in the library, and waits once per
 * sample.  The generator is Philox4x32-10 (Salmon et al., SC'11: multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
 * 0xBB67AE85, ten rounds), used by counter: a draw is a pure function of four integers and no state is carried.
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (c0, stream, t & 0xffffffff, t >> 32); t = the draw's index, one per sample, from 0; stream = the chain's number in a
 *             multi-chain run; c0 = the active-cell index a (0-based) for the momentum's normal of cell a, 0xFFFFFFFF for the sample's
 *             scalars (nAC is an int32: the two never meet).  The block's four words are x0 .. x3.
 *   uniform   U(hi, lo) = (2 k + 1) 2^-53 with k = ((uint64)(hi >> 6) << 26) | (lo >> 6): exact in fp64, strictly inside (0, 1)
 *   normal    of cell a: z = sqrt(-2 ln U(x0, x1)) * cos(2 pi U(x2, x3)) in fp64 from the block at c0 = a (one block per cell; the
 *             sine is not used).  The chain clips it at +-2.5 like a host normal.  |z| <= 8.57
 *   scalars   from the block at c0 = 0xFFFFFFFF: u = U(x0, x1); L = Lmin + (int)((x2 * (Lmax - Lmin + 1)) >> 32) in 64-bit arithmetic,
 *             whose bias is at most (Lmax - Lmin + 1) / 2^32 per value
 * So a chain's generator state is (seed, stream, t): three integers are what a checkpoint carries.
 *   hmcmt_rng_draw        L and u of draw t on the host (each may be NULL): no context, no device.  HMCMT_EINVAL for Lmin < 1 or
 *                         Lmax < Lmin.  u is the chain's bit for bit, L exactly
 *   hmcmt_rng_normals     the UNCLIPPED normals of the cells a0 .. a0 + n - 1 of draw t on the host, z[n]: no context, no device.  The
 *                         uniforms under them are the device's bit for bit; log, sqrt and cos are the host's libm, so z agrees with
 *                         the device's to a few ulp of 8.57 (4e-14 absolute holds both against a long-double evaluation).
 *                         HMCMT_EINVAL for a0 < 0, n < 0, a0 + n > 2^31 or a NULL z with n > 0
 *   hmcmt_chain_seed      on a live chain, at any point between two steps: sets (seed, stream) and t = 0.  hmcmt_chain_begin forgets
 *                         the seed
 *   hmcmt_chain_rng_state / hmcmt_chain_rng_seek   read (seed, stream, t; each may be NULL) / set t, the index of the next draw
 *   hmcmt_chain_normals   the device's clipped normals of draw t of this chain's (seed, stream), z[nAC] (host, or a device pointer with
 *                         on_device = 1); complete on return.  Moves neither t nor anything else of the chain
 *   hmcmt_chain_sample    one sample with draw t: the momentum on the device (k_chain_draw_momentum; for HMCMT_MASS_WM and
 *                         HMCMT_MASS_LOWRANK the clipped normals through the mass's own route), L in Lmin .. Lmax and u as
 *                         hmcmt_rng_draw gives them, then exactly hmcmt_chain_step: trajectory, accept test, commit, record, outputs
 *                         (m_out[nAC], pred_out complex [nData], host, each may be NULL).  t advances by one whether the sample succeeds
 *                         or fails: a failed sample consumes its draw as a failed step consumes its momentum, and leaves the chain
 *                         where it was.  The host waits once (plus once for the outputs when asked for); K0 comes from the record, and a
 *                         non-finite K0 is HMCMT_EBREAKDOWN.  The sample equals, bit for bit, hmcmt_chain_momentum with the normals
 *                         hmcmt_chain_normals(t) returns followed by hmcmt_chain_step with hmcmt_rng_draw(t)'s L and u
 *   hmcmt_chain_run       nsamples times hmcmt_chain_sample in one call: recs[nsamples] (required), models[nsamples][nAC] and preds
 *                         complex [nsamples][nData] (host, each may be NULL; row i filled behind sample i's decision).  Stops at the
 *                         first failing sample and returns its code; *done (may be NULL) = the number of valid records
 * hmcmt_chain_momentum and hmcmt_chain_step keep working on a seeded chain with the host's numbers and do not move t.  Warm-up
 * adaptation and the accumulators work unchanged: they live in the step's commit.  HMCMT_EINVAL: NULL context, rec, recs or z, no chain,
 * no seed, Lmin < 1, Lmax < Lmin, nsamples < 0, a call between hmcmt_grad_device_async and hmcmt_wait. */
extern int hmcmt_rng_draw(uint64_t seed, uint32_t stream, uint64_t t, int32_t Lmin, int32_t Lmax, int32_t* L, double* u);
extern int hmcmt_rng_normals(uint64_t seed, uint32_t stream, uint64_t t, int64_t a0, int64_t n, double* z);
extern int hmcmt_chain_seed(hmcmt_ctx* ctx, uint64_t seed, uint32_t stream);
extern int hmcmt_chain_rng_state(hmcmt_ctx* ctx, uint64_t* seed, uint32_t* stream, uint64_t* t);
extern int hmcmt_chain_rng_seek(hmcmt_ctx* ctx, uint64_t t);
extern int hmcmt_chain_normals(hmcmt_ctx* ctx, uint64_t t, double* z, int32_t on_device);
extern int hmcmt_chain_sample(hmcmt_ctx* ctx, int32_t Lmin, int32_t Lmax, hmcmt_chain_record* rec, double* m_out, double* pred_out);
extern int hmcmt_chain_run(hmcmt_ctx* ctx, int64_t nsamples, int32_t Lmin, int32_t Lmax, hmcmt_chain_record* recs, double* models,
                           double* preds, int64_t* done);

/* The No-U-turn sampler on a seeded chain: the trajectory length is chosen per sample (multinomial NUTS, Betancourt 2017, grown leaf
 * by leaf without recursion).  A sample ends in hmcmt_chain_step's commit, so the moments, the accumulators and a warm-up ride on it
 * unchanged; nothing above changes its bits.
 * Draws of sample t beside the momentum's normals (draw t's, as in hmcmt_chain_sample), in the counter scheme above:
 *   kind 0, doubling j: the block at c0 = 0xC0000000 + j; forward = x2 >> 31, u = U(x0, x1)
 *   kind 1, the sample's l-th leaf (0-based over the whole tree): the block at c0 = 0x80000000 + l; u = U(x0, x1)
 * Algorithm.  H = D + M + K, x = M^-1 p, momenta in the forward-time sign, log-weights delta = H0 - H.  The tree starts with both ends
 * at the start state, rho = p0, logW = 0, the selection the start.  Doubling j builds 2^j leaves from the end `forward` names; a leaf
 * is one step of hmcmt_leapfrog_device's map (backward: the same map on -p).  Leaf i of the subtree:
 *   delta not finite or -delta > 1000: the sample stops (stop 3, a divergence)
 *   logWs = logaddexp(logWs, delta); the leaf becomes the subtree's selection iff u_leaf < exp(delta - logWs) (leaf 0 always); rhos += p
 *   even i: the checkpoint k = popcount(i >> 1) = (p, x, rhos) is stored
 *   odd i: for k = popcount(i >> 1) down to k - (trailing ones of i) + 1, span = rhos - rhos_ck[k] + p_ck[k]; the leaf turns iff
 *          x_ck[k].span <= 0 or x.span <= 0 (stop 1) -- these are the aligned spans [i + 1 - 2^s, i]
 * A stopped subtree is discarded whole.  A completed one is merged: its selection replaces the tree's iff u_j < exp(min(0, logWs -
 * logW)); logW = logaddexp(logW, logWs); rho += rhos; the end moves; stop 2 iff x_minus.rho <= 0 or x_plus.rho <= 0; stop 0 at
 * max_depth doublings.  exp and logaddexp are host double arithmetic.
 *   hmcmt_chain_nuts_sample  one sample with draw t.  Per leaf one evaluation (whose solver records the host waits for, as in every
 *                            trajectory), one copy of scalars and one host wait behind it; rec.rec.nfevals =
 *                            nleaves, plus 1 when the start gradient had to be evaluated.  The next sample finds its start gradient on
 *                            the device.  Diagonal mass (set or adapted) and HMCMT_MASS_LOWRANK; HMCMT_MASS_WM is HMCMT_EINVAL.  An
 *                            active warm-up is fed rec.alpha.  The first call allocates the tree's buffers (HMCMT_ENOMEM leaves the
 *                            chain usable).  t advances by one whether the sample succeeds or fails; a leaf whose evaluation fails
 *                            returns that code and leaves the chain where it was
 *   hmcmt_chain_nuts_run     nsamples times hmcmt_chain_nuts_sample, in hmcmt_chain_run's conventions
 *   hmcmt_rng_nuts           the draws above on the host (forward, u: each may be NULL): no context, no device.  HMCMT_EINVAL for a
 *                            kind other than 0 / 1, index >= 32 (kind 0) or >= 2^30 (kind 1)
 * hmcmt_chain_step and hmcmt_chain_sample may follow a NUTS sample and the reverse.  HMCMT_EINVAL: max_depth outside 1 ..
 * HMCMT_NUTS_DEPTH_MAX, no chain, no seed, NULL rec, a call between hmcmt_grad_device_async and hmcmt_wait. */
#define HMCMT_NUTS_DEPTH_MAX 10
typedef struct hmcmt_nuts_record {
    hmcmt_chain_record rec;   /* accepted = selected != 0; nfevals; K0; K1, D1, M1 at the SELECTED state; D, M after the commit;
                                 hdif = H0 - H(selected); nsamples, nmoments as ever */
    int32_t depth;            /* doublings merged into the tree */
    int32_t nleaves;          /* leapfrog steps taken (<= 2^max_depth - 1) */
    int32_t stop;             /* 0 max_depth, 1 U-turn inside the new subtree, 2 U-turn of the merged tree, 3 divergence */
    uint32_t dirs;            /* bit j set: doubling j went forward in time (attempted doublings, the discarded one included) */
    int64_t selected;         /* signed time index of the selected state, 0 = the start */
    double  alpha;            /* mean over the leaves of min(1, exp(H0 - H_leaf)); a divergent leaf counts 0 */
} hmcmt_nuts_record;
extern int hmcmt_chain_nuts_sample(hmcmt_ctx* ctx, int32_t max_depth, hmcmt_nuts_record* rec, double* m_out, double* pred_out);
extern int hmcmt_chain_nuts_run(hmcmt_ctx* ctx, int64_t nsamples, int32_t max_depth, hmcmt_nuts_record* recs, double* models,
                                double* preds, int64_t* done);
extern int hmcmt_rng_nuts(uint64_t seed, uint32_t stream, uint64_t t, int32_t kind, uint32_t index, int32_t* forward, double* u);

/* Checkpoint and resume of a chain: everything a chain holds on the device and in the library -- state, moments, generator, the mass
 * in force, every accumulator that is on, an adaptation that was begun -- as one blob in host memory, and a chain made from such a blob.
 *   hmcmt_chain_save_size   *bytes = what hmcmt_chain_save writes for the chain as it stands
 *   hmcmt_chain_save      on a live chain, at any point between two samples.  It waits for the stream and copies into buf; *written
 *                         (may be NULL) = the blob's length.  capacity too small: HMCMT_EINVAL, *written = the size needed, nothing
 *                         written.  It is a read-out that changes NOTHING, parked cross-moment commits included (they are saved as
 *                         they are parked): a chain saved behind every sample gives the bits of one never saved, and two saves in a
 *                         row give the same bytes
 *   hmcmt_chain_restore   takes the place of hmcmt_chain_begin and of every accumulator's and adaptation's begin call.  It needs
 *                         hmcmt_set_prior, a context of the blob's nAC and nData and, for a blob saved under HMCMT_MASS_WM, a context
 *                         already on that mass (hmcmt_set_mass).  It runs NO evaluation: D, M and the predicted data are the blob's.
 *                         The blob's mass is installed as hmcmt_chain_set_mass_diag / hmcmt_chain_set_mass_lowrank install theirs (the
 *                         stored directions are not checked for orthonormality again) and is the context's from then on.  A chain that
 *                         is running is replaced whole, with the accumulators it had and the blob has not.  The blob is validated
 *                         completely before anything changes -- container (below), sizes, the mass kind, every range the begin calls
 *                         check --: HMCMT_EINVAL leaves a running chain untouched.  HMCMT_ENOMEM / HMCMT_EHIP leave the context usable,
 *                         without a chain.  Which run a blob belongs to (data, weights, reference model) the library does not know: it
 *                         checks sizes and kinds only
 *   hmcmt_chain_blob_info validates a blob's container without a context or a device and reports the header's fields, the sections'
 *                         tags and lengths in table order
 * NOT in a blob, so not restored: a momentum already drawn (a seeded chain draws its own, a host-fed one is drawn again:
 * hmcmt_chain_step without hmcmt_chain_momentum is refused); the gradient on the device -- the first sample behind a restore evaluates
 * its start gradient, so its nfevals is one more than the uninterrupted run's, the ONLY difference in its record; the NUTS tree's
 * buffers (allocated again by the first NUTS sample); the solver's warm-start history, sweep choice and queue tables; timers, profiles
 * and debug counters.  On a context whose gradient is a function of the model alone (warm_start cold, a fixed sweep count) the chain
 * behind a restore continues the saved one bit for bit.
 * HMCMT_EINVAL: NULL argument; save / save_size: no chain, a call between hmcmt_grad_device_async and hmcmt_wait.
 *
 * The container.  Little-endian throughout; every offset and length is a multiple of 8.
 *     0   char[8]  "HMCMTCK\0"
 *     8   uint32   version = 1 (any other is refused)        12  uint32  nsections (<= 16)
 *     16  uint64   total bytes, the checksum included
 *     24  int64    nAC                                       32  int64   nData
 *     40  int32    mass kind (HMCMT_MASS_*)                  44  uint32  seeded (0 / 1)
 *     48  int64    nsamples                                  56  int64   nmoments
 *     64  nsections x { uint32 tag; uint32 0; uint64 offset; uint64 bytes }
 *         the payloads, in table order, contiguous: the first at 64 + 24 nsections, each at the end of the one before
 *     end uint64   checksum: h = 0xcbf29ce484222325; for every preceding 8-byte word w, in order: h = (h ^ w) * 0x100000001b3 (mod 2^64)
 * A tag is four characters read as a little-endian uint32 ("CHAN" = 0x4e414843).  CHAN and MASS are always there, in this order; then,
 * each iff its part is on or was begun, HIST, DMOM, ACOV, "COV ", ADPT, ADLR (ADLR only with ADPT), SKCH (the last of the table, so
 * that every blob without a sketch keeps its bytes and its order).  No tag repeats.
 * The payloads: scalars first, 8 bytes each (i = int64, f = double, u = uint64), then arrays of doubles (unless said otherwise) in the
 * device's layout.
 *   CHAN  f dt, regParam, lnSigMin, lnSigMax, D, M;  i burnin, nsamples, nmoments;  u seed, t;  uint32 stream, seeded;
 *         m[nAC], pred[2 nData], mean[nAC], m2[nAC]  (the current model, its predicted data, the Welford pair of the moments)
 *   MASS  i kind, rank (0 unless HMCMT_MASS_LOWRANK), cap (directions the low-rank buffers have room for; 0: none), given (1: the
 *         scales hmcmt_set_mass_lowrank was given follow);  under HMCMT_MASS_WM nothing more (Wm and its factor are the prior's);
 *         else invM[nAC] (the diagonal as it stands);  then under HMCMT_MASS_LOWRANK s[nAC], U[rank][nAC], lambda[rank] (the bits
 *         that were given or estimated);  then, given = 1, invM0[nAC]
 *   HIST  i ntarget, nbins, count;  f lo, hi;  int64 target[ntarget];  uint32 counts[nbins][ntarget] (bin-major), zero-padded to 8
 *   DMOM  i count;  mean[2 nData], m2[2 nData]
 *   ACOV  i ntarget, all (1: every cell, no list), K = maxlag, count;  all = 0: int64 target[ntarget];  x0[ntarget], tot[ntarget],
 *         S[K + 1][ntarget], H[K + 1][ntarget], ring[K + 1][ntarget]
 *   COV   i nrow, all, B = batch, count, npend (commits parked);  all = 0: int64 row[nrow];  x0[nAC], tot[nAC], q[nAC],
 *         pend[npend][nAC], S[nrow][nAC]
 *   ADPT  i nwarmup, adapt_mass, init_buffer, term_buffer, base_window;  f delta, gamma, t0, kappa, dt_min, dt_max  (the options);
 *         f mu, s_bar, x_bar, x;  i t  (the dual averaging);  i c (steps adapted), wcount, wnext, wsize, windows_done;
 *         f alpha_last, alpha_sum;  i begun (1), active;  adapt_mass = 1: mean[nAC], m2[nAC] (the open window's Welford pair)
 *   ADLR  i rank, max_samples;  f cutoff, gamma  (the options);  i win_start, stride, stored, skipped, closed_stored, rows;
 *         the last closed window's info: i windows, stored, skipped, dims, rank, fallback, stride;  f theta_min, theta_max, defect,
 *         host_ms;  X[rows][nAC], G[rows][nAC] (rows = stored, or closed_stored while the open window is empty: the rows a later
 *         call can still read)
 *   SKCH  i ell, fill, count, shrinks, pivot_given;  f Delta;  x0[nAC], tot[nAC], q[nAC], B[fill][nAC]  (the row sketch; refused
 *         unless 2 <= ell <= 64, 0 <= fill < 2 ell -- a commit that fills the buffer shrinks it in the same call --, the counters
 *         belong together, Delta is finite and >= 0 and every array is finite) */
#define HMCMT_BLOB_VERSION 1
#define HMCMT_BLOB_SECTIONS_MAX 16
typedef struct hmcmt_chain_blob_header {
    uint32_t version, nsections;
    uint64_t total_bytes;
    int64_t  nAC, nData;
    int32_t  mass_kind;
    uint32_t seeded;
    int64_t  nsamples, nmoments;
    uint32_t tags[HMCMT_BLOB_SECTIONS_MAX];            /* in table order; 0 behind the last */
    uint64_t section_bytes[HMCMT_BLOB_SECTIONS_MAX];
} hmcmt_chain_blob_header;
extern int hmcmt_chain_save_size(hmcmt_ctx* ctx, uint64_t* bytes);
extern int hmcmt_chain_save(hmcmt_ctx* ctx, void* buf, uint64_t capacity, uint64_t* written);
extern int hmcmt_chain_restore(hmcmt_ctx* ctx, const void* buf, uint64_t bytes);
extern int hmcmt_chain_blob_info(const void* buf, uint64_t bytes, hmcmt_chain_blob_header* out);

/* Solution fields of the last evaluation THAT RAN (a call answered from the stored results runs nothing) in the
 * reference's layout: complex[(ny+1)*(nz+1)*nFreq],
 * node index (iz*(ny+1)+iy) fastest, then frequency (MT2DFwdSolver.jl:111-112).  adjoint=1 returns
 * the adjoint fields instead (interior = eVal of compJacTMatVec.jl:221, boundary 0). */
int hmcmt_get_fields(hmcmt_ctx* ctx, int32_t adjoint, double* exTE, double* hxTM);

/* Explicit data Jacobian (compJacMat / compJacTMat, MTSensitivity/compJacMat.jl, compJacTMat.jl) by the adjoint route: one
 * adjoint solve per receiver and batch of systems (the gradient's solve with that receiver's functional row as its source),
 * after a cold forward solve at m.  A Jacobian call leaves the context's evaluation state as it found it: warm-start fields
 * and their extrapolation history, the memo, the sweep choice and queue tables, the evaluation count, hmcmt_get_stats.
 *   wrt        HMCMT_JAC_WRT_SIGMA: d data / d sigma of the active cells (compJacMat's J); HMCMT_JAC_WRT_LNSIGMA: d / dm,
 *              m = ln sigma (the sampler's parameter): columns times sigma
 *   row0, nrows  rows row0 .. row0+nrows-1 of J in data order; only the receivers of those rows are solved, and only the
 *              systems their data address
 *   J          row-major [nrows][nAC]: complex (interleaved) for DataType Impedance, real for Rho_Pha (apparent resistivity
 *              (2/(w mu0)) Re(conj(Z) dZ), phase in degrees (180/pi) Im(conj(Z) dZ)/|Z|^2).  Row-major J is column-major
 *              J^T: Julia's compJacTMat layout
 *   st         (may be NULL) the Jacobian's own solves: forward / adjoint iteration totals and maxima, max error estimate,
 *              status, fallback solves
 * HMCMT_EINVAL for a row range outside [0, nData], an unknown wrt, or a call between hmcmt_grad_device_async and hmcmt_wait;
 * HMCMT_ENOCONV / HMCMT_EBREAKDOWN when a solve fails (the rows of that receiver's batch are not written).
 * hmcmt_jacobian_device: d_m, d_J are device pointers on the context's GPU (complete on return).
 * hmcmt_sensitivity: sens[nAC] = sqrt(sum_k |dataW_k J_ka|^2) over all data, without materialising J. */
#define HMCMT_JAC_WRT_SIGMA   0
#define HMCMT_JAC_WRT_LNSIGMA 1
int hmcmt_jacobian(hmcmt_ctx* ctx, const double* m, int64_t row0, int64_t nrows, int32_t wrt, double* J, hmcmt_stats* st);
int hmcmt_jacobian_device(hmcmt_ctx* ctx, const double* d_m, int64_t row0, int64_t nrows, int32_t wrt, double* d_J, hmcmt_stats* st);
int hmcmt_sensitivity(hmcmt_ctx* ctx, const double* m, int32_t wrt, double* sens, hmcmt_stats* st);

/* Matrix-free products with the data Jacobian at a linearisation point: J v by the forward (tangent-linear) route, J^T u by the
 * adjoint route, and the Gauss-Newton Hessian product -- each ONE solve of the live systems per direction, no J anywhere.
 *   hmcmt_linearize(m)   an evaluation at m that always runs (never answered from the stored results), from a zero guess:
 *              conductivities, coefficients, forward fields, receiver functionals and the boundary sensitivities -- everything
 *              hmcmt_grad computes in front of its adjoint solve.  It is an ordinary forward evaluation as far as the context's
 *              state goes (statistics, evaluation count, hmcmt_get_fields), except that it starts cold: the forward warm-start
 *              history begins again at m, like after hmcmt_set_options.  The point lives in the context's evaluation arrays and
 *              stays valid until the next call that evaluates (hmcmt_grad*, hmcmt_forward*, hmcmt_leapfrog*, hmcmt_jacobian*,
 *              hmcmt_sensitivity, hmcmt_linearize) or hmcmt_set_options.
 *   wrt        HMCMT_JAC_WRT_SIGMA (d sigma = v; J^T u as it is) or HMCMT_JAC_WRT_LNSIGMA (d sigma = sigma .* v; J^T u times sigma)
 *   hmcmt_jvp  Jv = compJacMat(m) * v (MTSensitivity/compJacMat.jl:206-314), v[nAC] real, Jv in the layout of pred: interleaved
 *              complex [nData]; Rho_Pha and RealTZY / ImagTZY data real with zero imaginary parts
 *   hmcmt_jtvp JTu[nAC] = real(compJacTMatVec(.., datVec = u, ..)) = Re(J^T conj(u)) (MTSensitivity/compJacTMatVec.jl:8) for any
 *              u in the layout of pred (of real data the real part is read).  hmcmt_grad's gradient is
 *              exp(m) .* hmcmt_jtvp(dataW^2 (pred - obs), HMCMT_JAC_WRT_SIGMA)
 *   hmcmt_gn_hessvec   Hv[nAC] = Re(J^H W^2 J) v = jtvp(W^2 jvp(v)), W = dataW, the intermediate kept on the device; no prior term
 *   st         (may be NULL) the product's own solves, as hmcmt_jacobian reports them: hmcmt_jvp one solve's forward-type
 *              iterations, hmcmt_jtvp adjoint-type ones, hmcmt_gn_hessvec one of each.  Only the systems that carry data are solved
 * A product leaves the context's evaluation state as it found it (forward fields, warm-start fields and history, the memo, the
 * sweep choice and queue tables, the evaluation count, hmcmt_get_stats) and is bitwise repeatable.
 * HMCMT_EINVAL (hmcmt_last_error says which): no valid linearisation point, a call between hmcmt_grad_device_async and
 * hmcmt_wait, an unknown wrt, a NULL or non-finite argument; HMCMT_ENOCONV / HMCMT_EBREAKDOWN when the product's solve fails.
 * The _device twins take device pointers on the context's GPU and are complete on return. */
int hmcmt_linearize(hmcmt_ctx* ctx, const double* m);
int hmcmt_linearize_device(hmcmt_ctx* ctx, const double* d_m);
int hmcmt_jvp(hmcmt_ctx* ctx, const double* v, int32_t wrt, double* Jv, hmcmt_stats* st);
int hmcmt_jtvp(hmcmt_ctx* ctx, const double* u, int32_t wrt, double* JTu, hmcmt_stats* st);
int hmcmt_gn_hessvec(hmcmt_ctx* ctx, const double* v, int32_t wrt, double* Hv, hmcmt_stats* st);
int hmcmt_jvp_device(hmcmt_ctx* ctx, const double* d_v, int32_t wrt, double* d_Jv, hmcmt_stats* st);
int hmcmt_jtvp_device(hmcmt_ctx* ctx, const double* d_u, int32_t wrt, double* d_JTu, hmcmt_stats* st);
int hmcmt_gn_hessvec_device(hmcmt_ctx* ctx, const double* d_v, int32_t wrt, double* d_Hv, hmcmt_stats* st);

/* Block products: nvec directions at the linearisation point in ONE solve per route -- a persistent launch over the nvec x (live
 * systems) virtual systems instead of nvec launches that each leave most of a large device idle (randomized SVD of J or of the
 * Gauss-Newton Hessian, block / subspace Gauss-Newton steps, Hessian probes, a few columns of J).
 *   layout     direction j is contiguous: V[j*nAC ..), JV[j*2*nData ..) interleaved complex in the layout of pred, U likewise, JTU and
 *              HV [nvec][nAC] -- rows of a C-ordered numpy array, columns of a Julia matrix
 *   meaning    direction j of a result is what the single-direction call returns for direction j at the same point (wrt, real data,
 *              Re(J^T conj(u)), the per-direction power-of-two normalisation), to the accuracy of the solves
 *   hmcmt_jvp_block   one forward-type solve; hmcmt_jtvp_block one adjoint-type solve; hmcmt_gn_hessvec_block one of each, U = W^2 J V
 *              kept on the device
 *   zero       a direction that is identically zero has its systems switched off: exact zeros, no iterations
 *   st         (may be NULL) the block's own solves as hmcmt_jacobian reports them: iteration sums over all virtual systems,
 *              nsystems = the systems solved (directions that are not zero x systems that carry data; gn: of the forward-type solve)
 *   nvec = 1   runs the single product's own code (no block arrays): the same bits as the single call; a zero direction's systems
 *              leave that solve at iteration 0 and are counted in nsystems
 *   nvec       1 .. HMCMT_BLOCK_MAX.  The block's solver arrays (about 300 bytes per node, system and direction) are allocated by
 *              the first block call, grow to the largest nvec seen and are released by hmcmt_destroy; HMCMT_ENOMEM when they do not
 *              fit -- the context stays usable, without them
 * State rules, errors and repeatability are the single products': a block product needs the linearisation point, runs no evaluation,
 * leaves the context's evaluation and solve state as it found it and is bitwise repeatable; HMCMT_EINVAL also for nvec out of range.
 * HMCMT_ENOCONV / HMCMT_EBREAKDOWN when any virtual system fails: nothing is promised about the outputs then. */
#define HMCMT_BLOCK_MAX 32
int hmcmt_jvp_block(hmcmt_ctx* ctx, const double* V, int32_t nvec, int32_t wrt, double* JV, hmcmt_stats* st);
int hmcmt_jtvp_block(hmcmt_ctx* ctx, const double* U, int32_t nvec, int32_t wrt, double* JTU, hmcmt_stats* st);
int hmcmt_gn_hessvec_block(hmcmt_ctx* ctx, const double* V, int32_t nvec, int32_t wrt, double* HV, hmcmt_stats* st);
int hmcmt_jvp_block_device(hmcmt_ctx* ctx, const double* d_V, int32_t nvec, int32_t wrt, double* d_JV, hmcmt_stats* st);
int hmcmt_jtvp_block_device(hmcmt_ctx* ctx, const double* d_U, int32_t nvec, int32_t wrt, double* d_JTU, hmcmt_stats* st);
int hmcmt_gn_hessvec_block_device(hmcmt_ctx* ctx, const double* d_V, int32_t nvec, int32_t wrt, double* d_HV, hmcmt_stats* st);

/* The MAP model on the device: projected L-BFGS over the gradient the library computes (host_map.h, kernels_map.h).
 * Model, gradient and history never leave the GPU; the host waits once per trial evaluation and decides from a handful of scalars.
 * Objective (what the chain calls D + M): Phi(m) = D(m) + 0.5 regParam (m - m_ref)' Wm (m - m_ref), g = g_data + regParam Wm (m - m_ref),
 * lnSigMin <= m <= lnSigMax; m_ref and Wm are hmcmt_set_prior's.  State: m, g, Phi, D, M, the predicted data, a ring of at most
 * `history` pairs (s, y).  One iteration (hmcmt_map_step):
 *   1. B = {a : (m_a <= lo and g_a > 0) or (m_a >= hi and g_a < 0)}; pg = g off B, 0 on B.
 *   2. d = -H pg with the L-BFGS inverse Hessian of the stored pairs, oldest to newest, H0 = gamma I, gamma = s'y / y'y of the newest pair
 *      (compact form: R = upper triangle of S'Y, Dg its diagonal, p = R^-1 S'pg, a = R^-T ((Dg + gamma Y'Y) p - gamma Y'pg),
 *      H pg = gamma pg + S a - gamma Y p); without pairs d = -pg min(1, 1 / |pg|inf); then d = 0 on B.  If g'd >= 0 with pairs stored,
 *      the pairs are dropped and d is the direction without pairs (a reset).
 *   3. Line search from alpha = 1: the trial is m_t = clip(m + alpha d, lo, hi), ONE full gradient evaluation there; accepted iff Phi_t is
 *      finite and Phi_t <= Phi + c1 g'(m_t - m); else alpha <- shrink alpha, at most max_backtracks shrinkings (max_backtracks + 1 trials).
 *      All trials failed with pairs stored: the pairs are dropped (a reset) and step 2 runs once more.  All failed without pairs: status
 *      HMCMT_MAP_STALLED, and m, g, Phi, D, M and the predicted data are bit for bit what they were.  (The reference's gradient is not
 *      everywhere the derivative of its misfit -- DESIGN.md section 2 -- so a run may stall well above the minimum; it never accepts a rise.)
 *   4. s = m_t - m, y = g_t - g are stored iff s'y > curv_eps |s|2 |y|2; a full ring overwrites its oldest pair.
 *   5. m, g, Phi, D, M and the predicted data become the trial's; status HMCMT_MAP_CONVERGED when |pg|inf <= gtol max(1, |pg0|inf) at
 *      the new state (pg0: at hmcmt_map_begin's, where the same test runs).
 * A trial whose evaluation fails (HMCMT_ENOCONV, HMCMT_EBREAKDOWN) makes the step return that code; the state and the pairs stay
 * untouched and the next step starts afresh (hmcmt_chain_step's rule).
 * hmcmt_map_begin needs hmcmt_set_prior (else HMCMT_EINVAL), clips m_start into the bounds, evaluates once and owns its buffers;
 * HMCMT_ENOMEM leaves the context usable; a begin over a live run reuses its buffers when `history` fits them.  hmcmt_set_prior,
 * hmcmt_set_mass* and hmcmt_destroy end the run.  A run and a chain may live on one context: both evaluate, so the chain's next step
 * re-evaluates its start gradient; a MAP step after foreign evaluations needs nothing, it keeps its own g.  Every MAP call that
 * evaluates ends a linearisation point.  Between hmcmt_grad_device_async and hmcmt_wait every MAP call is HMCMT_EINVAL, as are a step
 * of a run whose status is not HMCMT_MAP_RUNNING, NULL or non-finite arguments and options out of range (1 <= history <=
 * HMCMT_MAP_HISTORY_MAX, 0 <= max_backtracks <= 15, 0 < c1 < 1, 0 < shrink < 1, curv_eps >= 0, gtol >= 0).
 * The record describes the state the call returns: iter (0 from begin), status, nfevals (evaluations of this call), backtracks
 * (shrinkings of the last round), resets, npairs (stored after the call), pair_stored, nbound (|B|), alpha (accepted; 0 when stalled),
 * gamma and gTd of the last round's direction, phi = D + M, |pg|inf, |pg|2, sTy of the accepted step, and phi_trial: Phi of the last
 * round's trials in order, NaN beyond.  hmcmt_map_run iterates until a status other than HMCMT_MAP_RUNNING or maxiter steps, recs
 * [maxiter] (may be NULL), *ndone the steps made; a failed step ends it with that step's code.  hmcmt_map_state: the current model,
 * full gradient [nAC] and predicted data [2 nData] (each may be NULL; device pointers with on_device); it answers in every status. */
#define HMCMT_MAP_HISTORY_MAX 32
#define HMCMT_MAP_RUNNING 0
#define HMCMT_MAP_CONVERGED 1
#define HMCMT_MAP_STALLED 2
typedef struct hmcmt_map_options {
    int32_t history, max_backtracks;
    double c1, shrink, curv_eps, gtol;
} hmcmt_map_options;
typedef struct hmcmt_map_record {
    int32_t iter, status, nfevals, backtracks, resets, npairs, pair_stored, nbound;
    double alpha, gamma, phi, D, M, pg_inf, pg_2, gTd, sTy;
    double phi_trial[16];
} hmcmt_map_record;
void hmcmt_map_default_options(hmcmt_map_options* o);   /* history 8, max_backtracks 10, c1 1e-4, shrink 0.5, curv_eps 1e-10, gtol 1e-5 */
int hmcmt_map_begin(hmcmt_ctx* ctx, const double* m_start, double regParam, double lnSigMin, double lnSigMax,
                    const hmcmt_map_options* options /* NULL: the defaults */, hmcmt_map_record* rec0 /* may be NULL */);
int hmcmt_map_step(hmcmt_ctx* ctx, hmcmt_map_record* rec);
int hmcmt_map_run(hmcmt_ctx* ctx, int32_t maxiter, hmcmt_map_record* recs, int32_t* ndone);
int hmcmt_map_state(hmcmt_ctx* ctx, double* m, double* grad, double* pred, int32_t on_device);
int hmcmt_map_end(hmcmt_ctx* ctx);

/* All-gather of the chains' sample blocks over RCCL (xGMI inside a node): one process per GPU, one communicator per
 * process.  Replaces parallelHMCSampler's collection of the workers' results (HMCSampler/parallelHMC.jl:23-45:
 * remotecall_fetch of hmcmodel / hmcstats / hmcdata per worker) for hosts that hold their chains in this library:
 *   hmcmt_comm_id        rank 0 obtains the 128-byte RCCL id and hands it to the other ranks by its own means (the Julia
 *                        host: a remotecall; Python: torch.distributed's store; a file) -- ncclGetUniqueId
 *   hmcmt_comm_create    every rank, with the same id: ncclCommInitRank on `device_id` (collective)
 *   hmcmt_allgather_samples   `count` doubles per rank: recv[r*count .. (r+1)*count) = rank r's send -- ncclAllGather on
 *                        the communicator's stream, complete on return.  on_device = 1: send / recv are device pointers
 *                        on the communicator's GPU; 0: host buffers, staged through device memory
 * librccl.so is loaded on first use; without it these calls fail with HMCMT_ENODEV and nothing else is affected. */
#define HMCMT_COMM_ID_BYTES 128
typedef struct hmcmt_comm hmcmt_comm;
int hmcmt_comm_id(void* id /*[HMCMT_COMM_ID_BYTES]*/);
int hmcmt_comm_create(hmcmt_comm** comm, int32_t device_id, int32_t nranks, int32_t rank, const void* id);
int hmcmt_allgather_samples(hmcmt_comm* comm, const double* send, double* recv, int64_t count, int32_t on_device);
int hmcmt_comm_destroy(hmcmt_comm* comm);
const char* hmcmt_comm_last_error(const hmcmt_comm* comm);   /* comm may be NULL: hmcmt_comm_id / hmcmt_comm_create errors */

/* Production guard of the stopping rule, and chains that share a device. */
int hmcmt_guard(const hmcmt_ctx* ctx, double* out4);   /* {checks, worst true residual seen, last, trips (checks above HMCMT_GUARD_LIMIT, default 1e-6)}: the production guard of the stopping rule (every HMCMT_GUARD_EVERY-th evaluation, default 100) */
int hmcmt_next_cu_share(int32_t index, int32_t count);   /* the calling thread's NEXT hmcmt_create builds a context confined to share `index` of `count`
                                                             (1, 2, 4) equal shares of the CUs of every XCD (CU-masked streams): the persistent solve kernels of
                                                             `count` such contexts -- independent chains on one device, parallelHMC.jl:23-45 -- run side by side,
                                                             each with its share of the system slots (cfg3: two chains 1.15x one chain's steps/s).  Such a context's
                                                             streams are blocking HIP streams: they synchronise with the legacy default stream.
                                                             Consumed by that create; default: the whole device */

/* Instrumentation, introspection of the persistent solve kernel and the test hooks are declared in hmcmt_debug.h (same library):
 * hmcmt_profile*, hmcmt_dims, hmcmt_persist_*, hmcmt_debug_*.  Nothing in INTEGRATION.md section 1 needs them. */

#ifdef __cplusplus
}
#endif
#endif /* HMCMT_H */
