// libhmcmt_hip.so -- gfx950 (MI355X) implementation of the HMCMT2D hot path behind include/hmcmt.h.
//
// One translation unit in several files:
//   hmcmt_hip.hip     this file: the context, the host orchestration of an evaluation (evaluate / solve), the C ABI
//   hmcmt_knobs.h     the one reader of the environment variables (Knobs, read_knobs); Config below is what creation makes of them
//   host_jacobian.h   host code of the calls that borrow the context: explicit Jacobian, Jacobian products, block products
//   kernels_cocg.h    Solver state, deterministic reductions (DPP wave sums), classic COCG kernels (Jacobi / plain FDM
//                     preconditioners; the fp64 restart of a stagnating mixed-precision solve)
//   kernels_fdm.h     fast-diagonalisation stage: y-eigenbasis transforms on the matrix cores (split-bf16
//                     v_mfma_f32_16x16x32_bf16 by default, v_mfma_f64_16x16x4_f64 for fdm_precision = 1) around batched
//                     tridiagonal solves in z; k_fdm_fwd / k_back_post are the two fused kernels of the default path
//   kernels_fused.h   the fused COCG iteration (k_spmv_fused, k_update_fused), solve start / end, initial guesses
//   kernels_persist.h the whole COCG solve as ONE persistent kernel (round 4: a system = 8 workgroups of one XCD, r in
//                     registers, per-system barriers in the XCD's L2) -- the default where it applies
//   kernels_chain.h   the vector kernels of the device-resident HMC chain (hmcmt_chain_*); host_chain.h is its host code
//   kernels_path.h    "item" kernels, one thread per node / cell / receiver / boundary column with bodies in
//                     hmcmt_items.h (assembly from sigma, 1-D boundary fields and sensitivities, receiver functionals,
//                     adjoint sources, J^T v accumulation), and the leapfrog vector kernels
// The systems are never stored as CSR: real 5-point stencil coefficients shared by all frequencies of a polarisation,
// i*omega*D formed on the fly; every reduction is a fixed-order two-stage sum (bitwise repeatable).
// There is no host compute path: every entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <vector>
#include <mutex>
#include <functional>
#include <fcntl.h>
#include <unistd.h>
#include <sys/file.h>
#include "../../include/hmcmt.h"
#include "../../include/hmcmt_debug.h"
#include "hmcmt_host.h"
#include "hmcmt_items.h"
#include "hmcmt_knobs.h"

using namespace hmcmt;

#ifndef HMCMT_LP_NRG
#define HMCMT_LP_NRG 2
#endif
#ifndef HMCMT_LP_KC
#define HMCMT_LP_KC 4
#endif

namespace {

constexpr int MAXNB = 64;          // max partial-sum blocks per system (<= 64: one wave sums them, total_part)
#ifndef HMCMT_VBLOCK
#define HMCMT_VBLOCK 256
#endif
constexpr int VBLOCK = HMCMT_VBLOCK;        // threads of the vector kernels (build-time knob for A/B runs: 512 measured in round 3)

#include "kernels_cocg.h"
#include "kernels_fdm.h"
#include "kernels_fused.h"
#include "kernels_persist.h"
#include "kernels_persist4.h"
#include "kernels_path.h"
#include "kernels_mass.h"
#include "kernels_chain.h"
#include "kernels_nuts.h"
#include "kernels_map.h"
#include "kernels_jac.h"
#include "kernels_jvp.h"

// an instantiation of the persistent solve kernel (g_psKernels, launch_persist): k_cocg_persist<cw, sw, mw, cs, nyk, st> (two
// halves) or k_cocg_persist4<cw, sw, 32, nyk, 4, st> (four strips), strips x cw threads per workgroup
struct PsKernel {
    int strips, cw, sw, mw, cs, nyk;
    bool st;
    const void* fn;
};

}  // namespace

// measurement only (hmcmt_debug_chain_*_time): HIP-event pairs round the launches of one accumulator of the chain's commit, summed
// in two classes (host_chain.h)
struct ChainTimer {
    bool timing = false;
    std::vector<hipEvent_t> ev;           // pool, two per pending launch
    std::vector<int> pending;             // class of each pending launch
    double ms[2] = {0, 0};
    long long launches[2] = {0, 0};
    bool start(hipStream_t st);
    void stop(hipStream_t st, int cls);
    void collect(hipStream_t st);
    void free(int device, hipStream_t st);
    void report(hipStream_t st, int enable, double* msOut, int64_t* launchesOut);
};

// ----------------------------------------------------------------------------------------------
// context
// ----------------------------------------------------------------------------------------------
// What hmcmt_create decides once -- the knobs as read (Knobs: hmcmt_knobs.h) and everything derived from them, the mesh and the
// device (make_config) -- and nothing changes afterwards: the context holds it as a const member, so an assignment to one of these
// outside make_config does not compile.  The fields the kernels take by value (RT, RT2, RTS, splitT, xInFwd, twist, and stallIt /
// w2 of Knobs) are copied into Solver / View by create_impl.
struct Config : Knobs {
    int device = 0;
    int shareIdx = 0, shareCnt = 1;       // this context's share of every XCD's CUs (hmcmt_next_cu_share): index, 1 / 2 / 4 parts
    unsigned shareMask = 0xF;             // ... as quarters
    size_t maxLds = 64 * 1024;            // dynamic LDS the fused kernels may request
    size_t maxLdsBack = 64 * 1024;
    int bcCW = 0, bcSlots = 1;            // k_bc_fused: boundary columns per workgroup (0: k_bc_layers + k_bc_forward), edge slots
    size_t bcLds = 0;
    int bcbCW = 0, bcbSlots = 1;          // k_bc_blocked (meshes k_bc_fused's slabs do not fit): columns per workgroup (0: the two-kernel form)
    int bcbNT = 512, bcbLBu = 14, bcbLBd = 8;   // its threads, layers per block of the two recurrences
    size_t bcbLds = 0;
    bool sensFusedAlways = false;         // HMCMT_SENS_FUSED=1: also where the persistent kernel leaves CUs free (launch_adjoint_side)
    size_t sensFusedLds = 0;              // k_sens_fused: its LDS bytes (0: k_sens_layers + k_sens_profile + k_bcsens_pre; HMCMT_SENS_FUSED=0)
    int RT = 0, RT2 = 0, RTS = 0;         // rows per tile of the stencil kernels, of k_update_fused<2>, of k_spmv_fused<2> (Solver)
    int residThreads = 256;               // k_resid_pre
    int upd2Threads = 256, upd2Batch = 6; // launch shape of k_update_fused<2> (launch_update2; HMCMT_UPD2)
    int spmvThreads = 256;                // launch shape of k_spmv_fused (launch_spmv; HMCMT_SPMV)
    int upd1Threads = 256;                // ... of k_update_fused<1> (HMCMT_UPD1)
    // forward half of the FDM stage: slab width (in 16-mode tiles) of the fused kernel, 0 = the separate kernels -- where the fused
    // one is asked for (fwdNtwFused: HMCMT_FUSED_FWD != 0 assumed, hmcmt_debug_fdm_fwd) and as configured
    int fwdNtwFused = 0, fwdNtw = 0;
    int splitT = 0, xInFwd = 0, twist = 0;   // Solver::splitT / xInFwd, Solver / View::twist
    bool fusedBackFits = false;           // the fused back transform + post-smoother exists for this problem (pre-split operands, 16-row tile in LDS): fused_back_ok
    // persistent solve kernel (kernels_persist.h)
    int persistG = 0, persistCW = 0;      // workgroups per system, threads / 2 (0: the problem does not fit the kernel)
    int persistCS = 1, persistGZ = 0;     // column parts of a row block (2: wide meshes, kernels_persist.h), row blocks per system
    int persistMW = 32;                   // modes per slab of the persistent kernel's tridiagonal solves (32; 16 on tall meshes)
    int persistSlots = 0;                 // system slots per XCD of the context's own problem (Inst::persistSlots)
    size_t persistLds = 0;                // LDS bytes of psKern's kernels
    const PsKernel* psKern[2] = {};       // the instantiations launch_persist runs for one / two sweeps (g_psKernels)
    bool persistFillsShare = false;       // no CU of this context's share left over beside a solve (launch_adjoint_side)
};

struct hmcmt_ctx {
    const Config cfg;
    hmcmt_ctx(HostProblem&& problem, const hmcmt_options& o, const Config& c) : cfg(c), hp(std::move(problem)), opt(o) {}
    HostProblem hp;
    View v{};
    Solver sv{};
    hmcmt_options opt{};
    hmcmt_stats stats{};
    // What a solve or an evaluation moves.  The explicit Jacobian, the Jacobian products and the block products borrow the context,
    // solve, and give it back (Borrowed, host_jacobian.h): they copy this struct in front and assign it back behind, together with
    // v, sv, opt and stats, so that the context's next evaluation computes bit for bit what it would have.  A member whose value a
    // solve or an evaluation changes, and a later one reads, belongs HERE: as a plain member of hmcmt_ctx it leaves those calls
    // changed, and nothing says so -- a chain that differs in the 12th digit after a Jacobian call.  What creation decided cannot
    // be such a member any more: it is `cfg`, const.  The plain members that remain are resources (streams, events, buffers and
    // their sizes), counters and statistics, the memo, and the per-evaluation protocol flags -- solveBegun, preDone, psStart,
    // side*, *WaitPending, specValid, lpFallback, solveFail --, which the bracket resets rather than saves.
    struct SolveState {
        long long evalCount = 0;
        unsigned profMask = 0;            // bit c: time category c with HIP events
        int guardEvery = 100;                 // HMCMT_GUARD_EVERY (0: off)
        int dbgFlags = 0;                     // hmcmt_debug_flags
        int nSysOn = 0;                       // systems switched on (View::sysOn)
        bool haveFwd = false, haveAdj = false;   // previous fields usable as initial guesses
        bool haveModel = false;
        bool guardDropWarm = false;           // a trip: the next evaluation starts both solves cold
        bool solveDone[2] = {true, true};
        int lastItFwd = 0, lastItAdj = 0;
        int sweepsKind[2] = {1, 1};              // sweepsMode ... what the forward / adjoint solve uses next (auto: from its last iteration count)
        int sweepsUsed[2] = {1, 1};              // ... what the last evaluation's solves used
        int sweepsCount2[2] = {0, 0}, sweepsSince[2] = {0, 0};   // ... iterations of the last two-sweep solve, solves since the last probe
        bool sweepsProbe[2] = {false, false};    // ... the solve at hand is a one-sweep probe out of the two-sweep mode
        std::vector<int> itersLast;           // [2*S]
        std::vector<int> psOrder[2];          // what d_psOrder holds per solve kind (empty: the kernel's own order, no table passed)
        std::vector<float> psCost[2];         // the costs the tables are made from (smoothed iteration counts)
        long psRebalanced = 0;
        LfStep lfStep{};                      // a position update of hmcmt_leapfrog* still to be performed (by k_sigma_rows, or k_lf_step in front of k_sigma)
        LfMom lfMom{};                           // a momentum update of hmcmt_leapfrog* that the evaluation's last kernel performs (k_gradfinal)
        bool persistOn = true;                // HMCMT_PERSIST=0: the launch-per-phase loop only
        int persistWhyOff = 0;                // why persistOn is false: 1 = a placement fallback (for good), 2 = a timed-out wait (backoff)
        long persistBackoff = 0;              // after a timed-out wait: solves on the launch-per-phase loop before the kernel is tried again (doubles per timeout)
    } ss;
    // The resources of one solver instance that are not in Solver: partial sums, records, spare vectors, the persistent kernel's
    // words.  The context holds one set for its own problem, Blk one for the block products' virtual problem; a block call exchanges
    // the two for its duration (prod_run), so solve(), the kernel table and the fallbacks see an ordinary problem.
    struct Inst {
        double* d_partZZ = nullptr;
        double *d_partRes = nullptr, *d_partBn = nullptr;
        double* h_rec = nullptr;              // packed per-solve records: [2][S] iters, [2][S] status (int), [2][S] err (double)
        double* d_recHost = nullptr;          // device address of h_rec (pinned, mapped): k_solve_end writes it directly
        cplx* d_b = nullptr;                  // copy of the right-hand side (verify)
        cplx* d_sw = nullptr;                    // fp64 path with two sweeps per side: spare vector
        float2* d_invp32 = nullptr;
        float2* d_yhat2 = nullptr;            // column parts: the second part's partial product of the forward transform
        unsigned* d_psync = nullptr;          // [8 * slots][32] barrier words | exit counter | fail word
        size_t psyncBytes = 0;
        int persistSlots = 0;                 // system slots per XCD
        u4v* d_prec = nullptr;                // [S][MAXNB][2][8] records of the kernel's reductions (tagged, never cleared)
        PsConst* d_psConst = nullptr;         // the kernel's launch-invariant state, read through a constant-address-space pointer
        PsConst psShadow{};                   // what d_psConst holds (launch_persist refreshes the device copy when a field differs)
        bool psConstValid = false;
        bool dinvValid = true;                // Solver::dinv / dinv32 belong to the current model (ensure_dinv)
    } inst;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;       // sigma-only sensitivity tables run beside the forward solve
    hipEvent_t evModel = nullptr, evSens = nullptr, evExtF = nullptr, evExtA = nullptr, evPiv = nullptr, evRec = nullptr;
    bool solveBegun = false;                 // k_resid0 / k_resid_pre has done k_solve_begin's work for the next solve
    bool preDone = false;                    // k_resid_pre has done the first pre-smoothing pass of the next solve
    bool statsPending = false, pendingAdj = false;   // records of an asynchronous evaluation not read yet
    std::vector<void*> allocs;
    std::string err;
    // device scalars / buffers not in View
    u4v *d_Vb = nullptr, *d_Vtb = nullptr;        // bf16 fragment-order copies of V, V' (hi parts)
    u4v *d_Vbl = nullptr, *d_Vtbl = nullptr;      // ... lo parts: V = hi + lo to ~16 mantissa bits
    double *d_m = nullptr, *d_V = nullptr, *d_Vt = nullptr, *d_misfit = nullptr;
    double hostUs[4] = {0, 0, 0, 0}; long hostN = 0;      // HMCMT_TICKS: host time of the launch sequences around the solves
    bool sensWaitPending = false, extAWaitPending = false;
    cplx* d_fieldsOut = nullptr;
    // pinned host staging
    int* h_nactive = nullptr;
    int* h_stall = nullptr;               // pinned, mapped: Solver::stallHost (HW_WORDS words, host_word)
    int* h_prog = nullptr;                // pinned, mapped: Solver::progHost
    double* h_stage = nullptr;            // m / grad / pred / misfit staging
    size_t stageDoubles = 0;
    cplx* d_prevField[2] = {nullptr, nullptr};   // the EXT_NP-1 previous solutions (warm_start == 2), per solve kind: a ring [EXT_NP-1][S*vstride]
    double* d_mHist[2] = {nullptr, nullptr};     // [EXT_NP+1][nAC] model history per solve kind (a ring: kernels_fused.h)
    double* d_ext[2] = {nullptr, nullptr};       // {w_0..w_{EXT_NP-1}, keep, count, ring heads, partial sums, ticket} (kernels_fused.h)
    cplx* d_guessCap[2] = {nullptr, nullptr};    // test hook hmcmt_debug_guess_capture: the initial guesses of the last evaluation [S*vstride] (allocated when first enabled)
    bool guessCapture = false;
    View sideView; const double* sideM = nullptr;   // deferred side-stream launches of the adjoint half (launch_adjoint_side)
    bool sidePending = false, sideExtrap = false, sideSens = false;
    bool lpFallback = false;                 // this solve has switched its stragglers to the fp64 preconditioner
    // profiling
    int profEvery = 1;                // ... in every profEvery-th evaluation only (the brackets cost ~20 % if always on)
    std::vector<hipEvent_t> evPool;
    struct Interval { uint32_t a, b; int cat; bool chained; };   // events in front of / behind a sampled launch (ProfScope)
    std::vector<Interval> ivs;
    size_t evUsed = 0;
    size_t chainEnd = (size_t)-1;         // event behind the last chained launch, if nothing has been launched on the stream since
    double profOverheadChainMs = 0.0;     // overhead of an interval whose first event is the previous launch's last (one marker, not two)
    double profOverheadMs = 0.0;      // event-bracket overhead of one launch (spin-kernel calibration, hmcmt_profile)
    double profMs[HMCMT_NCAT] = {0};
    long long profN[HMCMT_NCAT] = {0};
    unsigned long long* d_cnt = nullptr;   // device counter behind Solver::cntActive
    long long profStartSys = 0, profEvals = 0, profSolves = 0, profSolves2 = 0;
    long long profSerialIts = 0, profPersistSolves = 0;    // sampled: sum over solves of (iterations of the slowest system + 1), solves run by the persistent kernel
    bool evalSampled = false;              // the evaluation whose records are parsed next was a sampled one   // sampled: systems active at the start of a solve (summed), evaluations, solves, solves with two sweeps
    // leapfrog / prior
    double *d_mref = nullptr, *d_invM = nullptr, *d_wmVal = nullptr, *d_p = nullptr, *d_mcur = nullptr, *d_g = nullptr;
    long long *d_wmRow = nullptr, *d_wmCol = nullptr;
    double *d_lfPart = nullptr, *d_lfScal = nullptr;
    int* d_lfFlag = nullptr;
    int* d_lfDone = nullptr;                 // [nAC] LfMom::done
    int lfGen = 0;                           // LfMom::gen of the last evaluation that carried a momentum update
    int* h_lfFlag = nullptr;                 // pinned copy of d_lfFlag (read after a synchronisation)
    double* d_gStart = nullptr;              // data gradient at the start model of the last trajectory (a rejection restarts there)
    bool havePrior = false, lfHaveGrad = false, lfFlagPending = false;
    std::vector<long long> wmRowH, wmColH;   // host copy of the CSR of Wm (hmcmt_set_mass factors it)
    std::vector<double> wmValH;
    // mass matrix (hmcmt_set_mass, kernels_mass.h): the factor and the transforms belong to the Wm in key*; kept across
    // hmcmt_set_prior calls with the same Wm (a host that re-registers the prior every trajectory does not refactor)
    struct Mass {
        int kind = HMCMT_MASS_DIAGONAL;
        bool ready = false;
        std::vector<long long> keyRow, keyCol;
        std::vector<double> keyVal;
        int bw = 0, separable = 0, nzb = 0, nyb = 0, pcgIters = 0;
        double factorSec = 0.0;
        double *d_L = nullptr, *d_Qz = nullptr, *d_QzT = nullptr, *d_Qy = nullptr, *d_QyT = nullptr, *d_lz = nullptr, *d_ly = nullptr;
        double *d_T1 = nullptr, *d_T2 = nullptr;          // [nzb*nyb] box images
        double *d_x = nullptr;                            // [nAC] Wm^-1 p of the leapfrog
        double *d_in = nullptr, *d_out = nullptr;         // [nAC] staging of hmcmt_mass_apply / PCG solution
        double *d_r = nullptr, *d_z = nullptr, *d_pp = nullptr, *d_q = nullptr, *d_s = nullptr;   // PCG vectors, scalars [8]
        int* d_map = nullptr;                             // [nzb*nyb] active index of each box cell, -1 frozen
        // HMCMT_MASS_LOWRANK (hmcmt_set_mass_lowrank): buffers of their own, released by mass_lr_release; d_x, d_in, d_out are shared
        int lrRank = 0, lrCap = 0;                        // directions in force; rows d_lrU, d_lrC and d_lrPart have room for
        double *d_lrS = nullptr, *d_lrU = nullptr;        // [nAC] s = sqrt(invM), [rank][nAC]
        double *d_lrC = nullptr;                          // [2][rank] lambda - 1, lambda^-1/2 - 1
        double *d_lrPart = nullptr;                       // [rank][LFNB] partial sums of the projection
        std::vector<double> lrLambda;                     // [rank] lambda as given or estimated (hmcmt_chain_mass_lowrank returns these bits)
        std::vector<double> lrInvM;                       // [nAC] the invM hmcmt_set_mass_lowrank was given; empty: d_invM holds the scales' squares
    } mass;
    // the device-resident HMC chain (hmcmt_chain_*, host_chain.h, kernels_chain.h)
    long long stateGen = 0;               // counts the evaluations and option changes of the context: a chain compares it with the value it left
                                          // (a plain member ON PURPOSE: the calls that borrow the context count too)
    struct Chain {
        bool active = false, haveMomentum = false;
        int cur = 0;                      // d_m[cur] / d_pred[cur]: the current state, [cur ^ 1]: the proposal
        double *d_m[2] = {nullptr, nullptr}, *d_pred[2] = {nullptr, nullptr};
        double *d_p = nullptr, *d_z = nullptr, *d_mean = nullptr, *d_m2 = nullptr;
        double *d_part = nullptr;         // [2][LFNB] partial sums of the kinetic energy at the start / at the proposal
        double *d_scal = nullptr;         // [CHAIN_SCAL]
        double *h_rec = nullptr;          // pinned: [CHAIN_REC] the sample's scalars, then [LFNB] partial sums (hmcmt_chain_momentum)
        double dt = 0, regParam = 0, lo = 0, hi = 0;
        double D = 0, M = 0, K0 = 0;
        long long burnin = 0, nsamples = 0, nmoments = 0;
        int nextStart = 0;                // start_grad of the next step: 0 evaluate, 1 accepted, 2 rejected
        long long gen = 0;                // stateGen when the chain last left the context
        // the chain's own generator (hmcmt_chain_seed; hmcmt_items.h: item_rng_*): the state is these three integers, t the next draw
        bool seeded = false;
        uint64_t seed = 0, t = 0;
        uint32_t stream = 0;
        std::vector<void*> allocs;
        // the optional accumulators of the commit (hmcmt_chain_hist_*, hmcmt_chain_data_moments*, hmcmt_chain_acov_*, hmcmt_chain_cov_*):
        // each owns its buffers through `allocs` (chain_acc_alloc / chain_acc_free; the d_ pointers only name them), released with the
        // chain and by every hmcmt_chain_begin
        struct Hist {
            bool on = false;
            long long ntarget = 0, count = 0;
            int nbins = 0;
            double lo = 0, hi = 0, scale = 0, w = 0;
            long long* d_target = nullptr;            // [ntarget] active-cell indices
            unsigned int* d_counts = nullptr;         // [nbins][ntarget], bin-major (hmcmt_items.h)
            std::vector<void*> allocs;
        } hist;
        struct DataMoments {
            bool on = false;
            long long count = 0;
            double *d_mean = nullptr, *d_m2 = nullptr;   // [2 nData] each
            std::vector<void*> allocs;
        } dmom;
        struct Acov {                                 // hmcmt_chain_acov_*: lagged autocovariances, every array lag-major (hmcmt_items.h)
            bool on = false;
            long long ntarget = 0, count = 0;
            int K = 0;
            long long* d_target = nullptr;            // [ntarget] active-cell indices; nullptr: every cell, row j = cell j
            double *d_x0 = nullptr, *d_tot = nullptr; // [ntarget] pivot and sum of y
            double *d_S = nullptr, *d_H = nullptr, *d_ring = nullptr;   // [K + 1][ntarget] each
            std::vector<void*> allocs;
            ChainTimer timer;                         // every k_chain_acov launch: class 0 some lag still fills H_k (t < K), 1 steady
        } acov;
        struct Cov {                                  // hmcmt_chain_cov_*: cross moments of the cells, cell index fastest (hmcmt_items.h)
            bool on = false;
            long long nrow = 0, count = 0;
            int B = 0, npend = 0;                     // batch length; commits in d_pend not yet folded into d_S
            long long* d_row = nullptr;               // [nrow] active-cell indices; nullptr: every cell, row r = cell r
            double *d_x0 = nullptr, *d_tot = nullptr, *d_q = nullptr;   // [nAC] pivot, sum of y, sum of y^2
            double *d_pend = nullptr;                 // [B][nAC]
            double *d_S = nullptr;                    // [nrow][nAC]
            std::vector<void*> allocs;
            ChainTimer timer;                         // every launch of the commit: class 0 k_chain_cov_commit, 1 k_chain_cov_flush
        } cov;
        struct Sketch {                               // hmcmt_chain_sketch_*: frequent-directions row sketch, cell index fastest (hmcmt_items.h)
            bool on = false, pivotGiven = false;
            int ell = 0, fill = 0;                    // rows 0 .. fill - 1 of d_B are in use; row 2 ell is the read-out's mean row
            long long count = 0, shrinks = 0;
            double Delta = 0;                         // sum of the shrinks' delta
            double *d_B = nullptr;                    // [2 ell + 1][nAC]
            double *d_x0 = nullptr, *d_tot = nullptr, *d_q = nullptr;   // [nAC] pivot, sum of y, sum of y^2
            double *d_K = nullptr, *d_T = nullptr;    // [2 ell + 1]^2 Gram staging; [2 ell + 1][HMCMT_MASS_RANK_MAX] doubles: T [ell][2 ell] or the PCA's coefficients
            std::vector<double> hK, hT;               // the host's copy of the Gram matrix; T or the PCA's coefficients while their upload is in flight
            std::string ended;                        // why a shrink ended the sketch (the read-outs' message); empty: it did not
            double hostMs = 0;                        // measurement: host ms of the shrinks' eigenproblems while the timer is on
            std::vector<void*> allocs;
            ChainTimer timer;                         // class 0 k_chain_sketch_commit, 1 k_chain_sketch_gram and k_chain_sketch_shrink (two launches per shrink)
        } sketch;
        struct Adapt {                                // hmcmt_chain_adapt_*: warm-up of dt and of the diagonal of M^-1 (hmcmt_items.h: item_adapt_*)
            bool begun = false, active = false;       // begun: in this chain, running or ended (hmcmt_chain_adapt_info)
            hmcmt_adapt_options opt{};
            AdaptDA da{};
            long long c = 0;                          // steps adapted so far
            long long wcount = 0, wnext = -1, wsize = 0;   // samples in the open window, its last step (-1: none follows), its length
            int windowsDone = 0;
            double alphaLast = 0, alphaSum = 0;
            double *d_mean = nullptr, *d_m2 = nullptr;   // [nAC] each: the window's Welford accumulator (adapt_mass)
            // hmcmt_chain_adapt_lowrank: the window's stored pairs and the window end's staging (hmcmt_items.h: item_adapt_lr_*)
            struct Lr {
                bool on = false;
                hmcmt_adapt_lowrank_options opt{};
                long long winStart = 0, stride = 1;   // the open window's first step and thinning
                int stored = 0, skipped = 0;          // pairs in the open window, pairs it skipped
                int closedStored = 0;                 // pairs of the window that closed last (its rows stay in the stores until the next pair)
                double *d_X = nullptr, *d_G = nullptr;          // [max_samples][nAC] draws, full gradients
                double *d_K = nullptr, *d_B = nullptr;          // [2 max_samples]^2, [2 max_samples][rank]
                double *d_meanX = nullptr, *d_meanG = nullptr;  // [nAC]
                double *d_s = nullptr, *d_U = nullptr, *d_c = nullptr, *d_part = nullptr;   // staging: [nAC], [rank][nAC], [2 rank], [rank][LFNB]
                std::vector<double> hK, hTheta;
                double times[4] = {0, 0, 0, 0};       // the last window end: ms of the two pairs, host ms up to K on the host, host ms of the check
                hmcmt_adapt_lowrank_info last{};
            } lr;
            std::vector<void*> allocs;
        } adapt;
        struct Nuts {                                 // hmcmt_chain_nuts_*: the tree's buffers, allocated at the first NUTS sample, released with the chain
            bool ready = false;
            double *d_m[2] = {nullptr, nullptr}, *d_p[2] = {nullptr, nullptr};   // [nAC] the ends, [0] backward (momentum stored negated), [1] forward
            double *d_x[2] = {nullptr, nullptr}, *d_g[2] = {nullptr, nullptr};   // [nAC] M^-1 p of an end (non-diagonal mass), its data gradient
            double *d_g0 = nullptr;                   // [nAC] the start state's gradient
            double *d_rho[2] = {nullptr, nullptr}, *d_rhoS = nullptr;            // [nAC] the tree's momentum sum and its successor, the subtree's
            double *d_ck[NUTS_CK_MAX][3] = {};        // [nAC] each: the checkpoints' p, x, rhoS
            double *d_selM[2] = {nullptr, nullptr}, *d_selG[2] = {nullptr, nullptr}, *d_selPred[2] = {nullptr, nullptr};   // captures: tree / subtree
            double *d_pred = nullptr;                 // [2 nData] the leaf's predicted data
            double *d_part = nullptr, *d_scal = nullptr;   // [NUTS_NQ][LFNB], [NUTS_SCAL]
            double *h_scal = nullptr;                 // pinned [NUTS_SCAL]
            long long its[2] = {0, 0}, solves[2] = {0, 0};   // measurement (hmcmt_debug_nuts_iters): solver iterations and solves of the leaves
                                                      //   [1] that follow a change of direction, [0] of the others
            std::vector<void*> allocs;
        } nuts;
    } chain;
    // the MAP optimiser (hmcmt_map_*, host_map.h, kernels_map.h): state, trial and history on the device, the scalars of the decisions here
    struct Map {
        bool active = false;
        int status = 0, cap = 0;              // cap: the history the ring and the small matrices have room for
        hmcmt_map_options opt{};
        int cur = 0;                          // d_m[cur], d_g[cur], d_pred[cur]: the state, [cur ^ 1]: the trial
        double *d_m[2] = {nullptr, nullptr}, *d_g[2] = {nullptr, nullptr}, *d_pred[2] = {nullptr, nullptr};
        double *d_gd = nullptr, *d_pg = nullptr, *d_d = nullptr;   // [nAC] the trial's data gradient, the projected gradient, the direction
        double *d_ring = nullptr;             // [2 cap][nAC]
        double *d_part = nullptr;             // [MAP_PART_ROWS][LFNB]
        double *d_SY = nullptr, *d_YY = nullptr;   // [cap][cap] by slot
        double *d_cs = nullptr;               // [MAP_COEF + MAP_SCAL] the coefficient block, then the trial's scalars
        double *h_rec = nullptr;              // pinned copy of d_cs
        int head = 0, count = 0;
        long long iter = 0;
        double regParam = 0, lo = 0, hi = 0;
        double phi = 0, D = 0, M = 0, pginf0 = 0, pginf = 0, pg2 = 0;
        int nbound = 0;
        std::vector<void*> allocs;
    } map;
    int solveFail = 0;                   // status a system of the last solve gave up with (mapped failure word), 0 = none
    // persistent solve kernel (kernels_persist.h)
    unsigned long long persistTag = 0;    // ... the tag base of the next launch
    long long* d_pstamps = nullptr;       // HMCMT_STAMPS=persist
    long long persistSolves = 0, persistFallbacks = 0, persistTimeouts = 0;
    // the order in which the queues of the persistent kernel take the systems (PsLaunch::order; persist_balance): per solve kind
    int* d_psOrder = nullptr;             // [2][S]
    int* h_psOrder = nullptr;             // pinned staging of the same
    struct PsStart { int resid = 0, begin = 0; };      // the solve's start inside the persistent kernel (PsLaunch::resid / begin): set by evaluate_once for the NEXT solve
    PsStart psStart{};
    bool persistTimedOut = false;         // a wait of the last persistent launch timed out: evaluate() redoes the evaluation with the launch-per-phase loop
    int dbgPlace = 0;                     // test hook (hmcmt_debug_flags bit 2): 1 + index of the group of the next persistent launch that fails its placement check
    bool dbgPlaceAdj = false;             // ... (bit 4) not the next launch but the next ADJOINT one: forward launches pass it by
    int fbKind = -1;                      // the last placement fallback: kind of its launch (0 forward, 1 adjoint; -1 none yet) and the systems that
    int fbStalled = -1;                   //   launch had started and left active -- stalled, continued from their own x and r -- (-1: not known there)
    bool counted = false;                 // this context is counted in g_quarterUse / holds a reference on the device lock
    // production guard on the error-estimate stopping rule: every guardEvery-th evaluation the TRUE residual of both
    // solves is formed (two vector passes and a read-back: ~0.1 ms once in guardEvery evaluations) -- hmcmt_guard
    long long guardChecks = 0;
    double guardWorst = 0.0, guardLast = 0.0;
    long long guardTrips = 0;
    // kernels queued behind a persistent solve before the host knows its outcome (View::gate; evaluate(), solve())
    int* d_gate = nullptr;                // [2] device words written by the persistent kernel's last workgroup, per solve kind
    int gateGen = 0;                      // serial number of the persistent launches
    bool specValid = false;               // the last solve's speculative followers ran (the solve ended clean)
    bool guardNow = false;                // the evaluation at hand is a guarded one
    // results of the last two host-API evaluations, keyed by the model: a sampler re-evaluates the model it has
    // just evaluated (getHamiltonian at the proposal, HMCSampler.jl:364; the first gradient of the next trajectory,
    // :217) or, after a rejection, the start model of the trajectory before -- those calls cost a memcmp
    struct Memo { std::vector<double> m, pred, grad; double misfit = 0; bool valid = false, hasGrad = false; hmcmt_stats stats{}; };
    Memo memo[2];
    int memoNext = 0;
    long long memoHits = 0;
    // the adjoint side of the Jacobian family: solution, boundary sources, boundary weights and their contraction with dBC
    struct AdjArrays { cplx *lam = nullptr, *srcB = nullptr, *wL = nullptr, *wR = nullptr, *colw = nullptr, *gL = nullptr, *gR = nullptr; };
    // the products' work arrays, [directions] times one direction's (kernels_jvp.h); scale: [4] per direction, the power-of-two
    // normalisation of the tangent's / the adjoint's input (k_dir_norm)
    struct ProdArrays {
        double *vin = nullptr, *out = nullptr, *dSig = nullptr, *gPartG = nullptr, *qPart = nullptr, *scale = nullptr;
        cplx *dbcL = nullptr, *dbcR = nullptr, *dbcB = nullptr, *jv = nullptr, *u = nullptr, *vbar = nullptr, *rxCoef = nullptr;
    };
    // explicit Jacobian (hmcmt_jacobian / hmcmt_sensitivity, kernels_jac.h): its own solution and boundary arrays, the saved forward
    // fields and extrapolation state of the context's evaluations, the batches' data lists and system flags (allocated on first use)
    struct Jac : AdjArrays {
        bool ready = false;
        cplx *xSave = nullptr, *qJ = nullptr, *pred = nullptr;
        double *extSave = nullptr, *misfit = nullptr, *m = nullptr, *rows = nullptr, *sens = nullptr;
        double* h_rows = nullptr;          // pinned staging of one batch's rows (host entry point)
        JacEntry* list = nullptr;          // [nData]
        JacGroup* groups = nullptr;        // [nData] runs of the list with one system
        int* sysOn = nullptr;              // [nRx][S]
        int maxRows = 0;                   // most data of one receiver
    } jac;
    // matrix-free Jacobian products (hmcmt_linearize, hmcmt_jvp / hmcmt_jtvp / hmcmt_gn_hessvec and their _block forms,
    // kernels_jvp.h): the linearisation point's model and the work arrays of ONE direction -- a product of one direction runs on
    // these, with the Jacobian's adjoint arrays (`jac`) and the context's own solver
    struct Jvp : ProdArrays {
        bool ready = false;
        bool valid = false;                // a linearisation point is set and no evaluation has run since
        double *m = nullptr, *misfit = nullptr;
        long long gen = 0;                 // serial number of the linearisation points (the block's replicated pivots belong to one)
    } jvp;
    // products of nvec > 1 directions: a second solver instance over nvec * S virtual systems -- its own per-system arrays, sync
    // words, records and constant block -- and work and adjoint arrays per direction.  Allocated by the first such call, grown to
    // the largest nvec seen, released at hmcmt_destroy (its own list: growing frees the smaller set)
    struct Blk : ProdArrays, AdjArrays {
        int cap = 0;                       // directions the arrays hold (0: none yet)
        long long gen = -1; int genVec = 0;   // the linearisation point and nvec the replicated pivots were made for
        std::vector<void*> allocs, hostAllocs;
        Solver sv{};
        Inst inst{};                       // (while a block call runs: the context's own, exchanged)
        int slots = 0;                     // system slots per XCD the sync words were made for (inst.persistSlots: those of the call at hand)
        cplx* invp = nullptr;
        double* omega = nullptr;
        int *h_onV = nullptr, *d_onVHost = nullptr;   // mapped: [cap S] the virtual systems solved, as k_blk_flags wrote them
        int *dirOn = nullptr, *sysOnDir = nullptr, *sysOnV = nullptr;
    } blk;
};

static thread_local std::string g_createError;      // (per thread: contexts of different chains are created from different threads)

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
            return (e_ == hipErrorOutOfMemory) ? HMCMT_ENOMEM : HMCMT_EHIP;                            \
        }                                                                                              \
    } while (0)

namespace {

// scope guard: f runs on every way out
template <class F>
struct AtExit {
    F f;
    explicit AtExit(F g) : f(g) {}
    AtExit(const AtExit&) = delete;
    ~AtExit() { f(); }
};

template <class T>
int dalloc(hmcmt_ctx* ctx, T** p, size_t n, bool zero = true) {
    void* q = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIPCHK(hipMalloc(&q, bytes));
    ctx->allocs.push_back(q);
    if (zero) HIPCHK(hipMemsetAsync(q, 0, bytes, ctx->stream));
    *p = (T*)q;
    return 0;
}
template <class T>
int dupload(hmcmt_ctx* ctx, T** p, const std::vector<T>& h) {
    int rc = dalloc(ctx, p, h.size(), false);
    if (rc) return rc;
    if (!h.empty()) HIPCHK(hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// One sampled launch = one interval between two events on the context's stream.  The four launches of an iteration
// follow each other with nothing in between, so the event behind one is the event in front of the next (`chain`): one
// hipEventRecord per launch instead of two -- half the marker packets in the queue, half the cost of sampling (round 3;
// the two forms have their own calibrated overheads, hmcmt_profile).
struct ProfScope {
    hmcmt_ctx* c; int cat; size_t a; bool chain, reused;
    static size_t new_event(hmcmt_ctx* c) {
        if (c->evUsed + 1 > c->evPool.size())
            for (int i = 0; i < 512; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return (size_t)-1; c->evPool.push_back(e); }
        const size_t i = c->evUsed++;
        hipEventRecord(c->evPool[i], c->stream);
        return i;
    }
    ProfScope(hmcmt_ctx* ctx, int cat_, bool chain_ = false) : c(ctx), cat(cat_), a((size_t)-1), chain(chain_), reused(false) {
        const bool on = ((c->ss.profMask >> cat) & 1u) && (c->ss.evalCount % c->profEvery) == 0 && !c->lpFallback;   // (the fp64 restart of a
        // straggling solve runs other kernels: not part of the sampled population)
        if (!on) { c->chainEnd = (size_t)-1; return; }
        if (chain && c->chainEnd != (size_t)-1) { a = c->chainEnd; reused = true; }
        else a = new_event(c);
        c->chainEnd = (size_t)-1;
    }
    ~ProfScope() {
        if (a == (size_t)-1) return;
        const size_t b = new_event(c);
        if (b == (size_t)-1) return;
        c->ivs.push_back(hmcmt_ctx::Interval{(uint32_t)a, (uint32_t)b, cat, reused});
        if (chain) c->chainEnd = b;
    }
};

void prof_collect(hmcmt_ctx* c) {
    if (c->evUsed == 0) return;
    hipStreamSynchronize(c->stream);
    for (const hmcmt_ctx::Interval& iv : c->ivs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->evPool[iv.a], c->evPool[iv.b]) == hipSuccess) {
            c->profMs[iv.cat] += std::max(0.0, (double)ms - (iv.chained ? c->profOverheadChainMs : c->profOverheadMs));
            c->profN[iv.cat] += 1;
        }
    }
    c->ivs.clear();
    c->evUsed = 0;
    c->chainEnd = (size_t)-1;
}

inline dim3 grid1(int n, int b) { return dim3((n + b - 1) / b); }

int launch_transform(hmcmt_ctx* ctx, const cplx* A, const double* Bsw, cplx* C, const int* active) {
    const View& v = ctx->v;
    const int M = v.S * v.NZP, NT = v.NYP / 16;
    const int groups = (M + 7) / 8;
    const int NW = std::min(4, (NT + 6) / 7);
    if ((NT + NW - 1) / NW > 7) { ctx->err = "mesh too wide for the transform kernel (ny+1 > 448)"; return HMCMT_EINVAL; }
    const int RG = std::max(1, 4 / NW);
    ProfScope ps(ctx, 0, true);
    hipLaunchKernelGGL(k_transform, dim3((groups + RG - 1) / RG), dim3(64 * NW * RG), 0, ctx->stream, A, Bsw, C, M,
                       v.NYP, v.NZP, active, NW, RG);
    return 0;
}

template <int OUT>
int launch_transform_lp(hmcmt_ctx* ctx, const float2* A, bool transposed, void* C, const int* active) {
    const View& v = ctx->v;
    const int M = v.S * v.NZP, NT = v.NYP / 16;
    const int groups = (M + 8 * LP_NRG - 1) / (8 * LP_NRG);
    // waves of LP_NTW column tiles; a workgroup holds all NW waves of RG row-group sets (<= 8 waves)
    const int NW = std::min(8, (NT + LP_NTW - 1) / LP_NTW);      // wider meshes: a wave loops over its tiles
    ProfScope ps(ctx, 0, true);
    const dim3 grid(groups), block(64 * NW);
    const size_t lds = (size_t)LP_NRG * ((v.NYP + 31) / 32) * 2 * 64 * sizeof(u4v);       // staged A fragments
    const u4v *bh = transposed ? ctx->d_Vtb : ctx->d_Vb, *bl = transposed ? ctx->d_Vtbl : ctx->d_Vbl;
    if (ctx->sv.splitT)        // the input was written pre-split (store_t32 / k_fdm_fwd)
        hipLaunchKernelGGL((k_transform_lp<OUT, 1>), grid, block, lds, ctx->stream, A, bh, bl, C, ctx->sv.dinv, ctx->sv.r, M, v.NYP,
                           v.NZP, active, NW);
    else
        hipLaunchKernelGGL((k_transform_lp<OUT, 0>), grid, block, lds, ctx->stream, A, bh, bl, C, ctx->sv.dinv, ctx->sv.r, M, v.NYP,
                           v.NZP, active, NW);
    return 0;
}

// Which of the two forms of a half of the FDM stage a launch takes: the hot path passes nothing (as configured); the debug entry
// points, which compare the two, ask for one
enum class FdmPath { Configured, Fused, Separate };
// LDS of k_back_post: z tile + staged A fragments
size_t back_post_lds(int NYP) { return (size_t)16 * NYP * sizeof(cplx) + (size_t)2 * ((NYP + 31) / 32) * 2 * 64 * 16; }
// the fused back transform + post-smoother runs (it exists for this problem: Config::fusedBackFits; HMCMT_FUSED_BACK, or the caller's path)
bool fused_back_ok(const hmcmt_ctx* ctx, FdmPath path = FdmPath::Configured) {
    return ctx->cfg.fusedBackFits && (path == FdmPath::Configured ? ctx->cfg.fusedBack : path == FdmPath::Fused);
}
// grid of the fused stencil kernels for `ntiles` row tiles per system (tile_map, kernels_fused.h)
dim3 tile_grid(const Solver& k, int ntiles) {
    return dim3(ntiles, k.S);
}
size_t update2_lds(const Solver& k) { return (size_t)(3 * k.RT2 + 8) * k.NYP * sizeof(float2); }
int update2_tiles(const Solver& k) { return (k.nz - 1 + k.RT2 - 1) / k.RT2; }
// The two stencil kernels of the iteration are launched with a thread count / batch size / tile height chosen per
// problem (round 3): at the headline size their first phase runs at the bandwidth of the fabric (Infinity Cache) -- 88 MB
// in 10 us with all systems active, in-kernel stamps HMCMT_STAMPS=upd -- so what counts is the bytes a tile loads, i.e.
// the share of halo rows: taller tiles with proportionally more threads (same work per thread, same phase structure).
// HMCMT_UPD2="threads,batch,rows" / HMCMT_SPMV="threads" override the choice.
void launch_update2(hmcmt_ctx* ctx, const float2* pcur, const cplx* rin, cplx* rout, int it, int startOnly) {
    const Solver& k = ctx->sv;
    const dim3 grid = tile_grid(k, update2_tiles(k));
    const size_t lds = update2_lds(k);
#define UPD2(NT, UB) hipLaunchKernelGGL((k_update_fused<2, NT, UB>), grid, dim3(NT), lds, ctx->stream, k, pcur, rin, rout, it, startOnly)
    const int nt = ctx->cfg.upd2Threads, ub = ctx->cfg.upd2Batch;
    if (nt == 1024) UPD2(1024, 4);
    else if (nt == 512 && ub <= 4) UPD2(512, 4);
    else if (nt == 512 && ub <= 6) UPD2(512, 6);
    else if (nt == 512) UPD2(512, 8);
    else UPD2(256, 6);
#undef UPD2
}
template <int SW>
void launch_spmv(hmcmt_ctx* ctx, size_t lds, const float2* pin, float2* pout, int it) {
    const Solver& k = ctx->sv;
    const dim3 grid = tile_grid(k, SW == 2 ? (k.nz - 1 + k.RTS - 1) / k.RTS : k.NTR);
    if (ctx->cfg.spmvThreads == 512) hipLaunchKernelGGL((k_spmv_fused<SW, 512>), grid, dim3(512), lds, ctx->stream, k, ctx->inst.d_partZZ, pin, pout, it, ctx->opt.maxit);
    else if (ctx->cfg.spmvThreads == 1024) hipLaunchKernelGGL((k_spmv_fused<SW, 1024>), grid, dim3(1024), lds, ctx->stream, k, ctx->inst.d_partZZ, pin, pout, it, ctx->opt.maxit);
    else hipLaunchKernelGGL((k_spmv_fused<SW, 256>), grid, dim3(256), lds, ctx->stream, k, ctx->inst.d_partZZ, pin, pout, it, ctx->opt.maxit);
}
// two sweeps per side exist on the fused mixed-precision path (and on the fp64 path of the restarts)
bool sweeps2_ok(const hmcmt_ctx* ctx) {
    const Solver& k = ctx->sv;
    const size_t spmv2 = (size_t)(k.RTS + 2) * k.NYP * sizeof(cplx) + (size_t)(k.RTS + 4) * k.NYP * sizeof(float2);
    return ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI &&
           (ctx->opt.fdm_precision != 0 || (update2_lds(k) <= (size_t)150 * 1024 && spmv2 <= (size_t)150 * 1024 &&
                                            (k.merged2 || (fused_back_ok(ctx) && k.NTR <= k.NB))));
}

// forward half of the mixed-precision FDM stage: y32 = tridiag^-1 (t32 V); fused kernel when its LDS slabs fit
// back half of the FDM stage + post-smoother: fused kernel on the pre-split path when its 16-row tile fits LDS
// stamps: per-block s_memtime stamps of k_back_post (HMCMT_BACK_STAMPS, debug entry only)
int launch_back_post(hmcmt_ctx* ctx, FdmPath path = FdmPath::Configured, long long* stamps = nullptr) {
    Solver& k = ctx->sv;
    const int NT = k.NYP / 16, NW = std::min(8, (NT + LP_NTW - 1) / LP_NTW);
    const size_t lds = back_post_lds(k.NYP);
    dim3 vg(k.NB, k.S), vb(VBLOCK);
    if (fused_back_ok(ctx, path)) {      // the kernel holds all of a wave's V fragments: 8 k-groups, 2 tiles
        const int nwg = (k.nz - 1 + BP_OWN - 1) / BP_OWN;
        if (k.sweeps == 2) {
            { ProfScope ps(ctx, 0, true);
              hipLaunchKernelGGL((k_back_post<1, 2>), dim3(nwg, k.S), dim3(64 * NW), lds, ctx->stream, k, k.y32, ctx->d_Vtb, ctx->d_Vtbl,
                                 ctx->inst.d_partZZ, NW, stamps); }
            if (k.merged2) return 0;                  // (the second post-sweep runs inside k_spmv_fused<2>)
            ProfScope ps(ctx, 7, true);
            hipLaunchKernelGGL(k_post2, dim3(k.NTR, k.S), vb, (size_t)(k.RT + 2) * k.NYP * sizeof(float2), ctx->stream, k, ctx->inst.d_partZZ);
            return 0;
        }
        ProfScope ps(ctx, 0, true);
        hipLaunchKernelGGL((k_back_post<1, 1>), dim3(nwg, k.S), dim3(64 * NW), lds, ctx->stream, k, k.y32, ctx->d_Vtb, ctx->d_Vtbl,
                           ctx->inst.d_partZZ, NW, stamps);
        return 0;
    }
    int rc;
    if (k.sweeps == 2) {                     // wide meshes, two sweeps: F t as fp64, then z4 and the sums of the rho identity
        if ((rc = launch_transform_lp<1>(ctx, k.y32, true, k.z, k.active))) return rc;
        { ProfScope ps(ctx, 7, true); hipLaunchKernelGGL(k_post_w2, vg, vb, 0, ctx->stream, k, ctx->inst.d_partZZ); }
        if (!k.merged2) { ProfScope ps2(ctx, 7, true); hipLaunchKernelGGL(k_post2, dim3(k.NTR, k.S), vb, (size_t)(k.RT + 2) * k.NYP * sizeof(float2), ctx->stream, k, ctx->inst.d_partZZ); }
        return 0;
    }
    if ((rc = launch_transform_lp<2>(ctx, k.y32, true, k.z, k.active))) return rc;   // z = F t + dinv r
    { ProfScope ps(ctx, 7, true); hipLaunchKernelGGL(k_post, vg, vb, 0, ctx->stream, k, ctx->inst.d_partZZ, k.z32); }
    return 0;
}

// slab width (in 16-mode tiles) of the fused forward kernel for this problem, 0 = use the separate kernels
size_t fdm_fwd_lds(const Solver& k, int ntw, int twist) {
    const int n = k.nz - 1, mid = twist_mid(n, twist);
    const size_t rl = (size_t)(twist ? mid + 1 : k.NZP) + 4 * FW_TB, nreg = twist ? 2 : 1, sw = 16 * (size_t)ntw;
    return (((size_t)k.NZP * sizeof(float) + 127) & ~(size_t)127) + (sw + 2 * FW_TB * sw + 3 * nreg * rl * sw + 2 * FW_TB * sw) * sizeof(c32) + 64;   // (+ 8 per-wave sums of the x update)
}
// fusedFwd: the fused kernel is wanted (HMCMT_FUSED_FWD != 0), force: also where the heuristic prefers the separate kernels (= 2)
int fdm_fwd_ntw(const Solver& k, bool fusedFwd, bool force, bool twistOn, size_t maxLds) {
    // The fused kernel pays off while every slab workgroup of a launch is resident at once and re-reading a
    // system's rows per slab is cheap: 32-mode slabs that fit LDS on meshes up to 256 nodes wide (measured:
    // 21 vs 29 us at 200x100 cells; at 400x200 the separate kernels win, 146 vs 219 us).  HMCMT_FUSED_FWD=2
    // forces it (16-mode slabs if need be), =0 disables it.
    if (!fusedFwd) return 0;
    const int tw = twistOn ? 1 : 0;
    if (fdm_fwd_lds(k, FW_NTW, tw) <= maxLds && (k.NYP <= 256 || force)) return FW_NTW;
    if (force && fdm_fwd_lds(k, 1, tw) <= maxLds) return 1;
    return 0;
}

int launch_fdm_fwd(hmcmt_ctx* ctx, const float2* pX = nullptr, FdmPath path = FdmPath::Configured) {        // pX: this iteration's direction -> the kernel's idle waves do x += alpha p
    Solver& k = ctx->sv;
    auto ldsFor = [&](int ntw) { return fdm_fwd_lds(k, ntw, k.twist); };
    // (k.splitT is set from the same width: the operand format goes with the path)
    const int ntw = !k.splitT ? 0 : path == FdmPath::Configured ? ctx->cfg.fwdNtw : path == FdmPath::Fused ? ctx->cfg.fwdNtwFused : 0;
    if (ntw) {
        const int G = (k.NZP + 7) / 8, per = (G + 7) / 8, nw = (G + per - 1) / per;
        const dim3 grid(((k.NYP / 16 + ntw - 1) / ntw) * k.S), block(64 * nw);
        ProfScope ps(ctx, 1, true);
        if (ntw == 1)
            hipLaunchKernelGGL(k_fdm_fwd<1>, grid, block, ldsFor(1), ctx->stream, k, k.t32, ctx->d_Vb, ctx->d_Vbl, ctx->inst.d_invp32, k.y32, (long long*)nullptr, k.xInFwd ? pX : (const float2*)nullptr);
        else
            hipLaunchKernelGGL(k_fdm_fwd<FW_NTW>, grid, block, ldsFor(FW_NTW), ctx->stream, k, k.t32, ctx->d_Vb, ctx->d_Vbl, ctx->inst.d_invp32, k.y32, (long long*)nullptr, k.xInFwd ? pX : (const float2*)nullptr);
        return 0;
    }
    int rc;
    if ((rc = launch_transform_lp<0>(ctx, k.t32, false, k.y32, k.active))) return rc;
    const dim3 tg((k.ny - 1 + 63) / 64, k.S);
    { ProfScope ps(ctx, 1, true); hipLaunchKernelGGL(k_thomas32, tg, dim3(64), 0, ctx->stream, k); }
    return 0;
}

// z = P^-1 r for the active systems and the partial sums of r'z, |z|^2 (partA / d_partZZ)
int apply_precond(hmcmt_ctx* ctx) {
    Solver& k = ctx->sv;
    dim3 vg(k.NB, k.S), vb(VBLOCK);
    if (ctx->opt.precond == HMCMT_PRECOND_JACOBI) {
        { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_jacobi, vg, vb, 0, ctx->stream, k); }
        { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_dots, vg, vb, 0, ctx->stream, k, ctx->inst.d_partZZ); }
        return 0;
    }
    const bool smooth = ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI;
    const dim3 tg((k.ny - 1 + 63) / 64, k.S);
    int rc;
    if (ctx->opt.fdm_precision == 0 && !ctx->lpFallback) {
        // mixed precision: split-bf16 operands / fp32 accumulation in the transforms, complex64 tridiagonal
        if (smooth && ctx->preDone) ctx->preDone = false;                        // (k_resid_pre has written t)
        else if (smooth && k.sweeps == 2) {                                       // both pre-sweeps of the residual at hand
            ProfScope ps(ctx, 3);
            launch_update2(ctx, k.p32a, k.r, k.r, 0, 1);
        }
        else if (smooth) { ProfScope ps(ctx, 2); hipLaunchKernelGGL(k_pre_c64, vg, vb, 0, ctx->stream, k); }
        else { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_to_c64, vg, vb, 0, ctx->stream, k, k.r); }
        if ((rc = launch_fdm_fwd(ctx))) return rc;
        if (smooth) {
            if ((rc = launch_back_post(ctx))) return rc;                                     // z = F t + dinv r, then the second Jacobi half
            std::swap(k.z, k.t);
        } else {
            if ((rc = launch_transform_lp<1>(ctx, k.y32, true, k.z, k.active))) return rc;
            ProfScope ps(ctx, 3);
            hipLaunchKernelGGL(k_dots, vg, vb, 0, ctx->stream, k, ctx->inst.d_partZZ);
        }
        return 0;
    }
    if (smooth && k.sweeps == 2) {                  // two sweeps per side, fp64 (fdm_precision = 1, and the restart of a stagnating solve)
        if (!ctx->inst.d_sw) { int rc2 = dalloc(ctx, &ctx->inst.d_sw, (size_t)k.S * k.vstride); if (rc2) return rc2; }
        hipLaunchKernelGGL(k_pre, vg, vb, 0, ctx->stream, k);                                        // t1 = r - A D r
        hipLaunchKernelGGL(k_sweep_exp, vg, vb, 0, ctx->stream, k, k.t, ctx->inst.d_sw, 0);               // z2 = D (r + t1)
        hipLaunchKernelGGL(k_sweep_exp, vg, vb, 0, ctx->stream, k, ctx->inst.d_sw, k.t, 1);               // t2 = r - A z2
        if ((rc = launch_transform(ctx, k.t, ctx->d_V, k.y, k.active))) return rc;
        hipLaunchKernelGGL(k_thomas, tg, dim3(64), 0, ctx->stream, k);
        if ((rc = launch_transform(ctx, k.y, ctx->d_Vt, k.z, k.active))) return rc;
        hipLaunchKernelGGL(k_sweep_exp, vg, vb, 0, ctx->stream, k, ctx->inst.d_sw, k.z, 3);               // z3 = F t2 + z2
        hipLaunchKernelGGL(k_sweep_exp, vg, vb, 0, ctx->stream, k, k.z, ctx->inst.d_sw, 2);               // z4 = z3 + D (r - A z3)
        Solver k2 = k; k2.z = ctx->inst.d_sw;
        hipLaunchKernelGGL(k_post, vg, vb, 0, ctx->stream, k2, ctx->inst.d_partZZ, (float2*)nullptr);     // t = z4 + D (r - A z4), dots
        std::swap(k.z, k.t);
        return 0;
    }
    if (smooth) { ProfScope ps(ctx, 2); hipLaunchKernelGGL(k_pre, vg, vb, 0, ctx->stream, k); }
    if ((rc = launch_transform(ctx, smooth ? k.t : k.r, ctx->d_V, k.y, k.active))) return rc;
    { ProfScope ps(ctx, 1); hipLaunchKernelGGL(k_thomas, tg, dim3(64), 0, ctx->stream, k); }
    if ((rc = launch_transform(ctx, k.y, ctx->d_Vt, k.z, k.active))) return rc;
    if (smooth) {
        { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_mid, vg, vb, 0, ctx->stream, k); }
        { ProfScope ps(ctx, 7); hipLaunchKernelGGL(k_post, vg, vb, 0, ctx->stream, k, ctx->inst.d_partZZ, (float2*)nullptr); }
        std::swap(k.z, k.t);                            // the smoothed result is the preconditioned residual
    } else {
        ProfScope ps(ctx, 3);
        hipLaunchKernelGGL(k_dots, vg, vb, 0, ctx->stream, k, ctx->inst.d_partZZ);
    }
    return 0;
}

void launch_adjoint_side(hmcmt_ctx* ctx);
int collect_pending(hmcmt_ctx* ctx);
int collect_stats(hmcmt_ctx* ctx, bool withAdjoint);
int finish_status(hmcmt_ctx* ctx);

constexpr double SPIN_LIMIT_S = 60.0;       // a convergence poll that sees no progress for this long gives up (HMCMT_EHIP)

// Two persistent kernels on one device could each hold CUs the other's missing workgroups need (they spin at their barriers
// until the bounded waits give up).  Inside a process: the contexts alive on each device are counted (per quarter of every XCD's CUs:
// g_quarterUse below), and the kernel runs only for a context that is alone on its share of the device.  Across processes: an advisory lock per device -- flock on
// $HMCMT_LOCK_DIR (/tmp) /hmcmt_persist_<PCI bus id>.lock, taken by the first context of a process on that device and held
// while it has one there; a process that does not get it runs the launch-per-phase loop and asks again every 256 solves.
// (Protects hmcmt processes from each other where they share the lock directory; HMCMT_PERSIST_LOCK=0 skips it.)
constexpr int MAXDEV = 64;
// CU shares (hmcmt_next_cu_share): a context may be confined to 1/2 or 1/4 of the CUs of EVERY XCD -- its streams carry a CU
// mask -- so that the persistent kernels of 2 or 4 contexts (chains) are co-resident on one device, each with a share of the
// system slots.  Use of the four quarters per device; a context runs the persistent kernel when it is alone in ALL its quarters.
std::atomic<int> g_quarterUse[MAXDEV][4];
thread_local int g_nextShareIdx = 0, g_nextShareCnt = 1;
static unsigned quarter_mask(int idx, int cnt) { return cnt == 1 ? 0xFu : cnt == 2 ? (idx ? 0xCu : 0x3u) : 1u << idx; }
struct DevLock { int fd = -1; int refs = 0; bool held = false; long asked = 0; };
std::mutex g_lockMu;
DevLock g_devLock[MAXDEV];

static bool devlock_try(DevLock& L) {
    if (L.fd < 0) return false;
    L.held = flock(L.fd, LOCK_EX | LOCK_NB) == 0;
    return L.held;
}
static void devlock_ref(const Config& cfg) {      // (HMCMT_PERSIST_LOCK, HMCMT_LOCK_DIR: those of the first context that takes the device's lock)
    const int dev = cfg.device;
    if (dev < 0 || dev >= MAXDEV) return;
    std::lock_guard<std::mutex> g(g_lockMu);
    DevLock& L = g_devLock[dev];
    if (L.refs++ > 0) return;
    if (!cfg.persistLock) { L.held = true; return; }
    char bus[64] = "unknown";
    if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) { (void)hipGetLastError(); snprintf(bus, sizeof bus, "dev%d", dev); }
    for (char* c = bus; *c; ++c) if (*c == ':' || *c == '/') *c = '_';
    // $HMCMT_LOCK_DIR, else /tmp: the one directory every user's processes on a machine share (a per-user runtime directory would
    // not coordinate two users' processes on one GPU).  The name is predictable, so the open follows no symlink (a planted link
    // could make it create or open a file elsewhere with this process's rights) and the file carries no data.
    const std::string path = cfg.lockDir + "/hmcmt_persist_" + bus + ".lock";
    L.fd = open(path.c_str(), O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
    if (L.fd < 0) L.fd = open(path.c_str(), O_RDONLY | O_CLOEXEC | O_NOFOLLOW);      // (another user's file: a shared lock needs no write access)
    if (L.fd < 0) { L.held = true; return; }           // (no lock directory: nothing to coordinate through)
    if (!devlock_try(L))
        fprintf(stderr, "libhmcmt_hip: %s is held by another process: this one runs the launch-per-phase solver on device %d until it is free "
                        "(hmcmt_persist_info: usable_now)\n", path.c_str(), dev);
}
static void devlock_unref(int dev) {
    if (dev < 0 || dev >= MAXDEV) return;
    std::lock_guard<std::mutex> g(g_lockMu);
    DevLock& L = g_devLock[dev];
    if (--L.refs > 0) return;
    if (L.fd >= 0) close(L.fd);                         // (drops the lock)
    L = DevLock{};
}
static bool devlock_held(int dev) {
    if (dev < 0 || dev >= MAXDEV) return true;
    std::lock_guard<std::mutex> g(g_lockMu);
    DevLock& L = g_devLock[dev];
    if (!L.held && (++L.asked & 255) == 0) devlock_try(L);
    return L.held;
}

// the persistent solve kernel applies to the solve at hand (default path, a mesh its tiles fit, alone on the device)
// (this context is alone on its device in the process, and the process holds the device's lock)
bool persist_alone(const hmcmt_ctx* ctx) {
    if (ctx->cfg.device < 0 || ctx->cfg.device >= MAXDEV) return false;
    for (int q = 0; q < 4; ++q)
        if (((ctx->cfg.shareMask >> q) & 1u) && g_quarterUse[ctx->cfg.device][q].load() != 1) return false;
    return devlock_held(ctx->cfg.device);
}
// the problem fits the kernel and the solver instance at hand has its words (a block call's instance may not: blk_enter)
bool persist_fits(const hmcmt_ctx* ctx) { return ctx->cfg.persistCW > 0 && ctx->inst.d_psync; }
bool persist_ok(const hmcmt_ctx* ctx) {
    return ctx->ss.persistOn && persist_fits(ctx) && ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI && ctx->opt.fdm_precision == 0 && persist_alone(ctx);
}
// a word of the mapped host block (HostWord)
volatile int& host_word(const hmcmt_ctx* ctx, HostWord w) { return reinterpret_cast<volatile int*>(ctx->h_stall)[w]; }

// Every instantiation of the persistent solve kernel: persist_config raises their LDS limit and picks the pair (one / two sweeps)
// of this context (ps_pick), launch_persist launches it.  HMCMT_STAMPS=persist: the phase stamps compiled in, on the 512-thread
// shapes the phase tables are made on; nyk: width-specialised (PS_WIDTHS: the row width is a compile-time constant).
template <int CW, int SW, int MW, int CS, int NYK = 0, bool ST = false>
PsKernel ps2() { return {2, CW, SW, MW, CS, NYK, ST, reinterpret_cast<const void*>(k_cocg_persist<CW, SW, MW, CS, NYK, ST>)}; }
template <int CW, int SW, int NYK = 0, bool ST = false>
PsKernel ps4() { return {4, CW, SW, 32, 1, NYK, ST, reinterpret_cast<const void*>(k_cocg_persist4<CW, SW, 32, NYK, 4, ST>)}; }
const PsKernel g_psKernels[] = {
    ps2<256, 1, 32, 1, 208, true>(), ps2<256, 2, 32, 1, 208, true>(), ps2<256, 1, 16, 2, 416, true>(), ps2<256, 2, 16, 2, 416, true>(),
    ps2<256, 1, 32, 1, 0, true>(),   ps2<256, 2, 32, 1, 0, true>(),   ps2<256, 1, 16, 2, 0, true>(),   ps2<256, 2, 16, 2, 0, true>(),
    ps2<256, 1, 32, 1, 208>(), ps2<256, 2, 32, 1, 208>(),
    ps2<128, 1, 32, 1, 112>(), ps2<128, 2, 32, 1, 112>(),      // (the reference's example meshes: 96 cells)
    ps2<256, 1, 16, 2, 416>(), ps2<256, 2, 16, 2, 416>(),
    ps2<256, 1, 32, 1>(), ps2<256, 2, 32, 1>(), ps2<128, 1, 32, 1>(), ps2<128, 2, 32, 1>(), ps2<64, 1, 32, 1>(), ps2<64, 2, 32, 1>(),
    ps2<256, 1, 16, 1>(), ps2<256, 2, 16, 1>(), ps2<128, 1, 16, 1>(), ps2<128, 2, 16, 1>(), ps2<64, 1, 16, 1>(), ps2<64, 2, 16, 1>(),
    ps2<256, 1, 16, 2>(), ps2<256, 2, 16, 2>(), ps2<128, 1, 16, 2>(), ps2<128, 2, 16, 2>(), ps2<64, 1, 16, 2>(), ps2<64, 2, 16, 2>(),
    ps4<256, 1, 208>(), ps4<256, 2, 208>(), ps4<256, 1, 208, true>(), ps4<256, 2, 208, true>(),
    ps4<256, 1>(), ps4<256, 2>(), ps4<128, 1>(), ps4<128, 2>(), ps4<64, 1>(), ps4<64, 2>()};
// The entry for a shape (strips, cw, mw, cs) of the kernel, the mesh's padded row width wk (0: generic only) and sw sweeps: the
// most specialised entry the table has -- with stamps where asked for, then width-specialised, then generic.  That is: stamps on
// cw = 256 with (cs, mw) = (1, 32) or (2, 16), and at four strips with width 208; width-specialised for (wk, cw, cs, mw) = (208,
// 256, 1, 32), (112, 128, 1, 32), (416, 256, 2, 16), at four strips for (208, 256); null if the table has no entry at all.
const PsKernel* ps_pick(int strips, int cw, int mw, int cs, int wk, bool stamps, int sw) {
    for (const bool st : {stamps, false})
        for (const int nyk : {wk, 0})
            for (const PsKernel& e : g_psKernels)
                if (e.strips == strips && e.cw == cw && e.sw == sw && e.mw == mw && e.cs == cs && e.nyk == nyk && e.st == st) return &e;
    return nullptr;
}
// one launch = the whole solve (or, precondOnly, one application of the preconditioner to k.r -> zout)
int launch_persist(hmcmt_ctx* ctx, int sweeps, int precondOnly, float2* zout, int kind = 0, hmcmt_ctx::PsStart start = hmcmt_ctx::PsStart{}) {
    Solver& k = ctx->sv;
    const int groups = 8 * ctx->inst.persistSlots;
    // the launch-invariant state: rebuilt from the solver's structures on every launch (a few hundred bytes of host work) and
    // compared with what the device copy holds -- any field that changes (an option, a buffer) refreshes it, nothing has to
    // remember to
    PsConst c{};
    c.S = k.S; c.nFreq = k.nFreq; c.NYP = k.NYP; c.NZP = k.NZP; c.ny = k.ny; c.nz = k.nz; c.twist = k.twist; c.stallIt = k.stallIt;
    c.vstride = k.vstride;
    c.G = ctx->cfg.persistG; c.GZ = ctx->cfg.persistGZ; c.slots = ctx->inst.persistSlots;
    c.C0 = ctx->cfg.persistCS > 1 ? ps_split_col(k.NYP) : k.NYP; c.TW = ps_tile_width(k.NYP, ctx->cfg.persistCS); c.PLW = ctx->cfg.persistCS > 1 ? ps_plane_width(k.NYP) : k.NYP;
    c.syncWords = (int)(ctx->inst.psyncBytes / sizeof(unsigned));      // (zero at create; every launch's last workgroup leaves them zero)
    c.spinLimit = ctx->cfg.persistSpin;
    c.wJ = (float)ctx->cfg.jacobiW;
    c.omega = k.omega; c.ofz = k.ofz; c.dM = k.dM; c.cY = k.cY; c.cZ = k.cZ; c.cf32 = k.cf32;
    c.active = k.active; c.iters = k.iters; c.status = k.status; c.nactive = k.nactive; c.nactHost = k.nactHost;
    c.failHost = k.failHost; c.stallHost = k.stallHost; c.progHost = k.progHost; c.errEst = k.errEst; c.ticks = k.ticks;
    c.sync = ctx->inst.d_psync; c.exitCnt = ctx->inst.d_psync + 32 * groups; c.fail = reinterpret_cast<int*>(ctx->inst.d_psync + 32 * groups + 8);
    c.placeHost = k.stallHost + HW_PLACE;
    c.Vb = ctx->d_Vb; c.Vtb = ctx->d_Vtb;
    c.pubR = k.t2_32; c.pubZ = k.zs32; c.pubP = k.p32a;
    c.yhat = k.y32; c.yhat2 = ctx->inst.d_yhat2; c.ysol = k.t32; c.tbuf = k.z4_32;
    c.ip32 = ctx->inst.d_invp32; c.rec = ctx->inst.d_prec;
    if (!ctx->inst.psConstValid || std::memcmp(&c, &ctx->inst.psShadow, sizeof c) != 0) {
        HIPCHK(hipStreamSynchronize(ctx->stream));             // (rare: an earlier launch may still read the old copy)
        HIPCHK(hipMemcpy(ctx->inst.d_psConst, &c, sizeof c, hipMemcpyHostToDevice));
        ctx->inst.psShadow = c; ctx->inst.psConstValid = true;
    }
    PsLaunch a{};
    a.kc = ctx->inst.d_psConst;
    a.x = k.x; a.r = k.r; a.tol2 = k.tol2; a.w2 = k.w2;
    a.maxit = ctx->opt.maxit; a.precondOnly = precondOnly;
    ctx->persistTag += std::max(1ull << 20, 2ull * ((unsigned long long)std::max(ctx->opt.maxit, 0) + 8));   // (an iteration takes two tags: a launch's range never reaches the next one's)
    a.tagBase = ctx->persistTag;
    a.zout = zout;
    a.stamps = ctx->d_pstamps;
    a.cntActive = k.cntActive;
    a.tickId = kind == 1 ? TK_PERSIST_A : TK_PERSIST_F;
    a.gateOut = precondOnly ? nullptr : ctx->d_gate + (kind == 1 ? 1 : 0);
    if (ctx->gateGen >= 0x3fffffff) ctx->gateGen = 0;           // (wrap BEFORE the increment: the followers are handed ctx->gateGen, the value this launch writes)
    a.gateGen = ++ctx->gateGen;
    if (ctx->dbgPlaceAdj && kind != 1) a.dbgPlace = 0;
    else { a.dbgPlace = ctx->dbgPlace; ctx->dbgPlace = 0; ctx->dbgPlaceAdj = false; }
    a.order = ctx->ss.psOrder[kind == 1].empty() ? nullptr : ctx->d_psOrder + (kind == 1 ? k.S : 0);
    a.resid = start.resid; a.begin = start.begin; a.nOn = ctx->ss.nSysOn; a.sysOn = ctx->v.sysOn;
    a.doneCnt = ctx->inst.d_psync + 32 * groups + 4;       // (in the block the kernel's last workgroup clears: exitCnt at +0, fail at +8)
    a.placedCnt = precondOnly ? nullptr : ctx->inst.d_psync + 32 * groups + 5; a.nGroups = groups;
    if (start.begin) *(volatile int*)ctx->h_nactive = ctx->ss.nSysOn;      // (mapped: "not all done yet" until the kernel's last converged system says otherwise)
    if (ctx->d_pstamps) HIPCHK(hipMemsetAsync(ctx->d_pstamps, 0, sizeof(long long) * 16 * 256, ctx->stream));
    const PsKernel& e = *ctx->cfg.psKern[sweeps == 2 ? 1 : 0];
    void* args[] = {&a};
    (void)hipLaunchKernel(e.fn, dim3(groups * ctx->cfg.persistG), dim3(e.strips * e.cw), args, ctx->cfg.persistLds, ctx->stream);
    HIPCHK(hipGetLastError());
    return 0;
}
// spin until `reached()` (the polls of solve(): a spin on host memory wakes within a microsecond; `pause` leaves the core's other
// hyper-thread its cycles, and the stream is looked at every 2^16 spins: a device error, or everything done, ends the wait; a
// device that makes no progress for SPIN_LIMIT_S seconds is reported instead of spinning forever)
template <class Reached>
int spin_until(hmcmt_ctx* ctx, Reached reached) {
    long spins = 0;
    std::chrono::steady_clock::time_point t0;
    while (!reached()) {
        __builtin_ia32_pause();
        if ((++spins & 0xffff) == 0) {
            if (hipStreamQuery(ctx->stream) != hipErrorNotReady) break;
            const auto now = std::chrono::steady_clock::now();
            if (spins == 0x10000) t0 = now;
            else if (std::chrono::duration<double>(now - t0).count() > SPIN_LIMIT_S) { ctx->err = "the device made no progress on a solve for 60 s"; return HMCMT_EHIP; }
        }
    }
    if (!reached()) HIPCHK(hipStreamSynchronize(ctx->stream));   // reports the error, if any
    return 0;
}
constexpr double SWEEPS2_COST = 1.20;       // time of a two-sweep iteration / time of a one-sweep iteration on the launch-per-phase loop (59-60 us / 50 us at the headline size)
constexpr double SWEEPS2_COST_PERSIST = 1.12, SWEEPS2_COST_PERSIST_CS2 = 1.08;   // ... in the persistent kernel (round 6 stamps: 33.1 / 29.6 us at cfg3, 40.0 / 37.1 at cfg5; round 5: 1.15 / 1.10)
constexpr int SWEEPS_PROBE_EVERY = 40;      // in two-sweep mode: every so many solves of a kind one solve runs one sweep, to compare
// damped Jacobi sweeps on each side of the FDM stage for the next solve of this kind.  Two sweeps cut the iterations by
// 20 % (smooth models) to 35 % (high-contrast ones) and cost ~20 % more time per iteration: by
// default a solve kind switches to two when its last solve needed more than sweepsUp iterations, back to one below
// sweepsDown, and -- since the gain depends on the model, not on the count -- tries one sweep once every
// SWEEPS_PROBE_EVERY solves and keeps whichever is cheaper (parse_stats).
int pick_sweeps(const hmcmt_ctx* ctx, int kind) {
    if (ctx->cfg.sweepsMode == 1 || !sweeps2_ok(ctx)) return 1;
    return ctx->cfg.sweepsMode == 2 ? 2 : ctx->ss.sweepsKind[kind];
}

// Solves A x = r for all systems (x zero on interior on entry; r destroyed).  kind 0 forward, 1 adjoint.
void launch_solve_end(hmcmt_ctx* ctx, int kind) {
    const int S = ctx->sv.S;
    hipLaunchKernelGGL(k_solve_end, dim3((S + 63) / 64), dim3(64), 0, ctx->stream, ctx->sv, kind, (int*)ctx->inst.d_recHost, ctx->inst.d_recHost + 2 * S);
}
SolveRec solve_rec(hmcmt_ctx* ctx, int kind) {
    const Solver& k = ctx->sv;
    return SolveRec{k.iters, k.status, k.errEst, (int*)ctx->inst.d_recHost, ctx->inst.d_recHost + 2 * k.S, kind, k.S};
}

// deferEnd: the caller's next kernel writes the per-solve records (k_rxall / k_wb with solve_rec) instead of k_solve_end
// spec: launches the caller wants queued right behind the solve -- with the persistent kernel they go out BEFORE the host has seen
// the solve end, gated on the device word the kernel's last workgroup writes (View::gate): the host's wake-up and launch latency
// (18 us behind the forward solve, 11 behind the adjoint one) run under kernels that are already in the queue.  ctx->specValid
// says whether they ran; if not (a stalled, failed or displaced solve: they returned at once) the caller queues them again.
using SpecFn = std::function<void(const int* gate, int gen)>;
// The Jacobi diagonals of every system for the kernels of the launch-per-phase loop, where k_coef_all left them out (an evaluation that
// was to run in the persistent kernel: a placement fallback, a stagnated system's fp64 restart, a second context on the device).
void ensure_dinv(hmcmt_ctx* ctx) {
    if (ctx->inst.dinvValid) return;
    hipLaunchKernelGGL(k_dinv, dim3(ctx->sv.NB, ctx->sv.S), dim3(VBLOCK), 0, ctx->stream, ctx->sv, ctx->cfg.jacobiW);
    ctx->inst.dinvValid = true;
}
// What the persistent attempt of a solve came to (solve_persist)
enum class PsOutcome {
    NotRun,         // the persistent kernel does not apply to this solve
    Misplaced,      // a group's workgroups were not on one XCD: the context has left the kernel, the launch-per-phase loop solves
    Done,           // the kernel ran, every system converged
    Stalled,        // ... a system stagnated: the fp64 restart loop continues the active systems
    Unfinished      // ... neither: a system gave up or a wait timed out (the failure word says which), else the fp64 restart loop
};
// The persistent attempt: ONE launch solves every system (kernels_persist.h).  The kernel tells the host through mapped words: the
// progress word when its last workgroup leaves, the active-system counter, the stagnation / failure / placement / timeout words.
int solve_persist(hmcmt_ctx* ctx, int kind, hmcmt_ctx::PsStart start, const SpecFn* spec, PsOutcome& out) {
    Solver& k = ctx->sv;
    const int S = k.S;
    ctx->preDone = false;                          // (it does its own first pre-smoothing pass)
    host_word(ctx, HW_STALL) = 0;
    host_word(ctx, HW_PLACE) = 0;
    host_word(ctx, HW_TIMEOUT) = 0;
    *(volatile int*)ctx->h_prog = 0;
    { ProfScope ps(ctx, 2); int prc = launch_persist(ctx, k.sweeps, 0, nullptr, kind, start); if (prc) return prc; }
    ++ctx->persistSolves;
    if (k.cntActive) ++ctx->profPersistSolves;
    if (kind == 0 && ctx->sidePending) {
        // (the host is free while the device solves.)  Not before the persistent kernel's whole grid is resident (progress word 1, behind
        // the last group's placement check): the side streams do not wait for the kernels in front of the solve, and k_sens_fused's
        // workgroups (LDS, 256 threads), dispatched first, sit on CUs this kernel's workgroups need -- at the stress size the solve
        // started 0.1 ms late.  (A misplaced group never reports: the kernel then ends early, PS_DONE ends this wait as well.)
        long spins = 0;
        while (*(volatile int*)ctx->h_prog == 0 && ++spins < (1l << 26)) {
            __builtin_ia32_pause();
            if ((spins & 0xffff) == 0 && hipStreamQuery(ctx->stream) != hipErrorNotReady) break;
        }
        launch_adjoint_side(ctx);
    }
    if (spec && ctx->cfg.specOn) (*spec)(ctx->d_gate + kind, ctx->gateGen);
    { int prc = spin_until(ctx, [ctx] { return *(volatile int*)ctx->h_prog == PS_DONE; }); if (prc) return prc; }
    if (host_word(ctx, HW_TIMEOUT)) {
        // a wait inside the kernel timed out (a word of its own: a healthy group's system that ends with a status afterwards
        // overwrites the shared status word, and the redo below would be skipped) (its grid was not co-resident: a foreign kernel holds CUs, a lock directory that
        // does not coordinate): the systems are in no defined state.  This context leaves the persistent kernel -- for 256 solves
        // after the first timeout, twice as long after every further one --, and evaluate() runs the evaluation again, cold,
        // with the launch-per-phase loop, which works under any sharing
        ctx->persistTimedOut = true;
        ctx->ss.persistOn = false; ctx->ss.persistWhyOff = 2; ++ctx->persistTimeouts;
        ctx->ss.persistBackoff = 256l << std::min<long long>(ctx->persistTimeouts - 1, 6);     // (the tenant may leave: 256, 512, .. 16 384 solves, then another try)
    }
    if (host_word(ctx, HW_PLACE)) {
        // the group's workgroups were not on one XCD (or the kernel could not be placed): nothing was touched by those
        // groups -- this context goes back to the launch-per-phase loop for good
        ctx->ss.persistOn = false; ctx->ss.persistWhyOff = 1; ctx->ss.persistBackoff = 0; ++ctx->persistFallbacks;
        ctx->fbKind = kind; ctx->fbStalled = -1;
        if (start.begin && start.resid) {
            // (rare, and behind a finished kernel: what it left is read back -- active 1: started and stalled, 2: never started)
            std::vector<int> act(S);
            HIPCHK(hipMemcpyAsync(act.data(), k.active, sizeof(int) * S, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            ctx->fbStalled = (int)std::count(act.begin(), act.end(), 1);
        }
        ensure_dinv(ctx);
        if (start.begin) {
            // (the kernel was to form the residual itself: the systems the misplaced groups did not touch -- active = 2 -- have none
            //  yet; those a healthy group started and left stalled -- active = 1 -- keep their x and r: r is no longer the right-hand
            //  side the adjoint start forms would read from it.  The launch-per-phase loop's partial sums start from zero)
            HIPCHK(hipMemsetAsync(k.partB, 0, (size_t)S * MAXNB * sizeof(double), ctx->stream));
            if (start.resid) hipLaunchKernelGGL(k_resid0, dim3(k.NB, S), dim3(VBLOCK), 0, ctx->stream, k, k.x, start.resid == PS_RESID_FULL ? 0 : start.resid, (const int*)nullptr, 2);
        }
        if (ctx->persistFallbacks == 1)
            fprintf(stderr, "libhmcmt_hip: the workgroups of a system of the persistent solve kernel were not dispatched to one XCD (a partitioned device, "
                            "another dispatch order?); this context runs the launch-per-phase loop from here on -- same results, several times slower "
                            "(hmcmt_persist_info: placement_fallbacks, why_off)\n");
        out = PsOutcome::Misplaced;
        return 0;
    }
    out = *(volatile int*)ctx->h_nactive == 0 ? PsOutcome::Done : host_word(ctx, HW_STALL) ? PsOutcome::Stalled : PsOutcome::Unfinished;
    return 0;
}
// The launch-per-phase loop of the mixed-precision path (the fused kernels): from it = 0 until every system is done, a system
// stagnates or the iteration cap; `it` ends as the iterations launched (done: needed)
int solve_fused(hmcmt_ctx* ctx, int kind, int nextCheck, bool& done, int& it) {
    Solver& k = ctx->sv;
    { int prc = apply_precond(ctx); if (prc) return prc; }          // z = P^-1 r and the partial sums of r'z, |z|^2
    float2* pb[2] = {k.p32a, k.p32b};
    cplx* rb[2] = {k.r, k.r2};
    int rcur = 0;
    // Convergence polls without events.  The device keeps three words in mapped pinned memory: the number of active
    // systems and the stagnation flag (k_spmv_fused of iteration `it` updates them with its decision on the state
    // after iteration it-1) and a progress word (the first thread of k_spmv_fused(it) stores `it` when it STARTS,
    // i.e. when everything of iteration it-1 has completed).  From the iteration count of the previous call on, the
    // host queues all of iteration `it`, then spins until the progress word says k_spmv_fused(it) has started --
    // three launches (~40 us) are still queued behind it at that moment and a spin on host memory wakes within a
    // microsecond, so the queue never drains -- and reads the counter.  (An event per polled iteration put a 6 us
    // bubble behind every polled k_spmv_fused and its hipEventSynchronize took 50-100 us to wake; round 1 lost
    // ~90 us per evaluation there.)  The launches queued behind a finished solve find every system inactive and
    // exit at once.
    host_word(ctx, HW_STALL) = 0;
    *(volatile int*)ctx->h_prog = 0;
    bool stalled = false;
    // (HMCMT_SIDE_IT = n > 0: at iteration n; default: half-way through the expected solve, between 2 and 12)
    const int sideIt = ctx->cfg.sideIt > 0 ? ctx->cfg.sideIt : std::max(2, std::min(12, nextCheck / 2));
    while (!done && !stalled && it < ctx->opt.maxit + 1) {
        ++it;
        // decide convergence of the state after iteration it-1, p = z + beta p, q = A p
        if (k.sweeps == 2 && k.merged2) {
            ProfScope ps(ctx, 2, true);
            launch_spmv<2>(ctx, (size_t)(k.RTS + 2) * k.NYP * sizeof(cplx) + (size_t)(k.RTS + 4) * k.NYP * sizeof(float2), pb[(it - 1) & 1], pb[it & 1], it);
        } else { ProfScope ps(ctx, 2, true); launch_spmv<1>(ctx, (size_t)(k.RT + 2) * k.NYP * sizeof(cplx), pb[(it - 1) & 1], pb[it & 1], it); }
        if (k.sweeps == 2) { ProfScope ps(ctx, 3, true); launch_update2(ctx, pb[it & 1], rb[rcur], rb[rcur ^ 1], it, 0); }
        else { ProfScope ps(ctx, 3, true); if (ctx->cfg.upd1Threads == 512) hipLaunchKernelGGL((k_update_fused<1, 512, 6>), tile_grid(k, k.NTR), dim3(512), (size_t)(2 * k.RT + 2) * k.NYP * sizeof(cplx), ctx->stream, k, pb[it & 1], rb[rcur], rb[rcur ^ 1], it, 0);
               else hipLaunchKernelGGL((k_update_fused<1, 256, 6>), tile_grid(k, k.NTR), dim3(256), (size_t)(2 * k.RT + 2) * k.NYP * sizeof(cplx), ctx->stream, k, pb[it & 1], rb[rcur], rb[rcur ^ 1], it, 0); }
        rcur ^= 1;
        k.r = rb[rcur];
        int prc;
        if ((prc = launch_fdm_fwd(ctx, pb[it & 1]))) return prc;
        if ((prc = launch_back_post(ctx))) return prc;
        std::swap(k.z, k.t);
        if (it >= nextCheck || it - 1 == ctx->opt.maxit) {
            { int prc = spin_until(ctx, [ctx, it] { return *(volatile int*)ctx->h_prog >= it; }); if (prc) return prc; }
            if (it - 1 == ctx->opt.maxit) HIPCHK(hipStreamSynchronize(ctx->stream));          // (k_spmv_fused(it) itself decides the cap)
            if (*(volatile int*)ctx->h_nactive == 0) { done = true; break; }
            if (host_word(ctx, HW_STALL)) stalled = true;
        }
        // (a dozen API calls, ~150 us of host time: issued half-way through the expected solve, at most a dozen
        // iterations deep -- short solves, 5-6 iterations on smooth paths, would otherwise get them behind the solve and
        // wait for the adjoint guess.  Without a tracer attached 2..12 measure the same within 1 %; under
        // rocprofv3, whose launches cost twice as much, the early settings drain the main queue.)
        if (kind == 0 && it == sideIt) launch_adjoint_side(ctx);
        // (likewise the wait for the adjoint guess of the side stream, four iterations behind its launch)
        if (kind == 0 && it == sideIt + 4 && ctx->extAWaitPending) { ctx->extAWaitPending = false; ctx->chainEnd = (size_t)-1; HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->evExtA, 0)); }
        // the gradient tail needs the sensitivity tables of the side stream (205 + 53 us of serial kernels beside the forward
        // solve, long complete by the adjoint solve's 8th iteration): the wait goes into the queue HERE, where the host runs
        // ahead of the device, not behind the solve, where the device waits for every call
        if (kind == 1 && it == 8 && ctx->sensWaitPending) { ctx->sensWaitPending = false; ctx->chainEnd = (size_t)-1; HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->evSens, 0)); }
    }
    if (!done) {
        // stragglers (or the iteration cap): read the counter once more, then hand over to the classic loop
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (*(volatile int*)ctx->h_nactive == 0) done = true;
    }
    if (done) it = std::max(0, it - 1);
    return 0;
}
// The classic loop with the fp64 preconditioner: the whole solve on the other preconditioners, and the restart of COCG from the
// systems' x and r where the mixed-precision solve (fused) stagnated or reached the cap
int solve_fp64(hmcmt_ctx* ctx, bool fused, int nextCheck, bool& done, int& it) {
    Solver& k = ctx->sv;
    const dim3 vg(k.NB, k.S), vb(VBLOCK);
    const int every = ctx->opt.check_every > 0 ? ctx->opt.check_every : 2;
    const int lpCap = 60;               // (classic loop only) mixed-precision safety net: stragglers continue with the fp64 preconditioner
    // (a mesh wider than 447 cells has no fp64 eigen-transform to restart with: a NUMERICAL event -- a stagnating solve -- ends the
    //  evaluation as "not converged", not as an invalid argument from launch_transform)
    if (fused && ctx->hp.NYP / 16 > 28) {
        ctx->err = "a mixed-precision solve stagnated on a mesh wider than 447 cells, where the fp64 restart does not exist (include/hmcmt.h, hmcmt_create): not converged";
        return HMCMT_ENOCONV;
    }
    const bool restart = fused;      // coming from the fused loop: restart COCG with the fp64 preconditioner
    if (restart) { ctx->lpFallback = true; ++ctx->stats.fallback_solves; }
    // z = P^-1 r ; rho = r'z ; p = z
    { int prc = apply_precond(ctx); if (prc) return prc; }
    { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_check, dim3(1), dim3(128), 0, ctx->stream, k, ctx->inst.d_partZZ, restart ? 2 : 1, ctx->opt.maxit); }
    { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_pupdate, vg, vb, 0, ctx->stream, k, 1); }
    while (!done && it < ctx->opt.maxit) {
        ++it;
        if (it == lpCap + 1 && ctx->opt.fdm_precision == 0 && ctx->opt.precond != HMCMT_PRECOND_JACOBI && !ctx->lpFallback) {
            ctx->lpFallback = true;     // restart COCG for the still-active systems: z = P64^-1 r, p = z
            ++ctx->stats.fallback_solves;
            { int prc = apply_precond(ctx); if (prc) return prc; }
            { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_check, dim3(1), dim3(128), 0, ctx->stream, k, ctx->inst.d_partZZ, 2, ctx->opt.maxit); }
            { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_pupdate, vg, vb, 0, ctx->stream, k, 1); }
        }
        { ProfScope ps(ctx, 2); hipLaunchKernelGGL(k_spmv, vg, vb, 0, ctx->stream, k); }
        { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_update, vg, vb, 0, ctx->stream, k); }
        { int prc = apply_precond(ctx); if (prc) return prc; }
        { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_check, dim3(1), dim3(128), 0, ctx->stream, k, ctx->inst.d_partZZ, 0, ctx->opt.maxit); }
        { ProfScope ps(ctx, 3); hipLaunchKernelGGL(k_pupdate, vg, vb, 0, ctx->stream, k, 0); }
        if (it >= nextCheck || it == ctx->opt.maxit) {
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (*(volatile int*)ctx->h_nactive == 0) done = true;
            nextCheck = it + every;
        }
    }
    return 0;
}
// The solve's records (k_solve_end, unless deferEnd) and, with options.verify or the production guard, the true residual
int solve_epilogue(hmcmt_ctx* ctx, int kind, const cplx* x, bool done, bool deferEnd, bool guard) {
    const Solver& k = ctx->sv;
    const int S = k.S;
    const dim3 vg(k.NB, S), vb(VBLOCK);
    if (!deferEnd) launch_solve_end(ctx, kind);
    if (ctx->opt.verify || (guard && done)) {
        hipLaunchKernelGGL(k_trueres, vg, vb, 0, ctx->stream, k, (guard && kind == 0) ? (const cplx*)nullptr : ctx->inst.d_b, x, ctx->inst.d_partRes, ctx->inst.d_partBn);
        std::vector<double> pr((size_t)S * MAXNB), pb((size_t)S * MAXNB);
        HIPCHK(hipMemcpyAsync(pr.data(), ctx->inst.d_partRes, pr.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(pb.data(), ctx->inst.d_partBn, pb.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (int s = 0; s < S; ++s) {
            double rr = 0, bb = 0;
            for (int b = 0; b < k.NB; ++b) { rr += pr[(size_t)s * MAXNB + b]; bb += pb[(size_t)s * MAXNB + b]; }
            if (bb > 0) ctx->stats.true_res_max = std::max(ctx->stats.true_res_max, std::sqrt(rr / bb));
        }
        if (guard) {
            ++ctx->guardChecks; ctx->guardLast = ctx->stats.true_res_max; ctx->guardWorst = std::max(ctx->guardWorst, ctx->guardLast);
            if (!(ctx->guardLast <= ctx->cfg.guardLimit)) {
                // the estimate ||z|| <= tol ||x|| stopped a solve whose residual is not small: say so, and do not warm-start from it
                ++ctx->guardTrips;
                ctx->ss.guardDropWarm = true;
                fprintf(stderr, "hmcmt: stopping-rule guard: evaluation %lld, %s solve: true residual %.3e > %.1e (tol %.1e)\n",
                        ctx->ss.evalCount, kind == 0 ? "forward" : "adjoint", ctx->guardLast, ctx->cfg.guardLimit, ctx->opt.tol);
            }
        }
    }
    return 0;
}
int solve(hmcmt_ctx* ctx, cplx* x, int kind, bool deferEnd = false, const SpecFn* spec = nullptr) {
    Solver& k = ctx->sv;
    k.x = x;
    k.tol2 = ctx->opt.tol * ctx->opt.tol;
    const int S = k.S;
    const size_t vecBytes = (size_t)S * k.vstride * sizeof(cplx);
    if (ctx->opt.verify) HIPCHK(hipMemcpyAsync(ctx->inst.d_b, k.r, vecBytes, hipMemcpyDeviceToDevice, ctx->stream));
    // production guard (every guardEvery-th evaluation): the true residual of this solve without options.verify -- the forward
    // problem's right-hand side lives in x's boundary nodes (k_trueres forms it), the adjoint one was copied to d_b by evaluate()
    const bool guard = !ctx->opt.verify && ctx->guardNow;
    // all systems of the requested modes start active (device copy: no host round trip)
    const hmcmt_ctx::PsStart start = ctx->psStart;          // (evaluate_once: residual and bookkeeping inside the persistent kernel)
    ctx->psStart = hmcmt_ctx::PsStart{};
    if (!ctx->solveBegun)           // (otherwise done by the residual kernel in front of this solve -- or about to be done by the persistent kernel)
        hipLaunchKernelGGL(k_solve_begin, dim3((S * MAXNB + 255) / 256), dim3(256), 0, ctx->stream, k, ctx->v.sysOn);
    ctx->solveBegun = false;
    if (k.cntActive) { ++ctx->profSolves; ctx->profStartSys += ctx->ss.nSysOn; if (k.sweeps == 2) ++ctx->profSolves2; }
    int& guess = kind == 0 ? ctx->ss.lastItFwd : ctx->ss.lastItAdj;
    const int nextCheck = guess > 2 ? guess : 4;
    ctx->lpFallback = false;
    ctx->solveFail = 0;
    host_word(ctx, HW_FAIL) = 0;             // (ordered before this solve's kernels: the previous solve has been waited for)
    const bool fused = ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI && ctx->opt.fdm_precision == 0;
    cplx* const r_entry = k.r;
    ctx->specValid = false;
    // (after a timed-out wait: another try when the backoff has run out -- a context that left the kernel because of its PLACEMENT
    //  stays off for good: persistWhyOff)
    if (!ctx->ss.persistOn && ctx->ss.persistWhyOff == 2 && ctx->ss.persistBackoff > 0 && --ctx->ss.persistBackoff == 0) { ctx->ss.persistOn = true; ctx->ss.persistWhyOff = 0; }
    PsOutcome outcome = PsOutcome::NotRun;
    if (fused && persist_ok(ctx)) { int prc = solve_persist(ctx, kind, start, spec, outcome); if (prc) return prc; }
    const bool viaPersist = outcome == PsOutcome::Done || outcome == PsOutcome::Stalled || outcome == PsOutcome::Unfinished;
    bool done = outcome == PsOutcome::Done;
    int it = 0;
    if (!done) ensure_dinv(ctx);          // (everything below that touches the systems again reads the diagonals)
    if (start.begin && outcome == PsOutcome::NotRun) {
        // (the persistent kernel was to start this solve but did not run after all -- a second context has appeared on the device since
        //  evaluate_once looked --: the start as launches of their own)
        if (start.resid) hipLaunchKernelGGL(k_resid0, dim3(k.NB, S), dim3(VBLOCK), 0, ctx->stream, k, x, start.resid == PS_RESID_FULL ? 0 : start.resid, ctx->v.sysOn, 0);
        else hipLaunchKernelGGL(k_solve_begin, dim3((S * MAXNB + 255) / 256), dim3(256), 0, ctx->stream, k, ctx->v.sysOn);
    }
    if (start.begin && outcome == PsOutcome::Stalled) HIPCHK(hipMemsetAsync(k.partB, 0, (size_t)S * MAXNB * sizeof(double), ctx->stream));   // (the fp64 restart's loop: its partial sums start from zero)
    if (fused && !viaPersist) { int prc = solve_fused(ctx, kind, nextCheck, done, it); if (prc) return prc; }
    if (viaPersist) it = guess;          // (what the kernel needed is in its records: parse_stats)
    if (!done && !(viaPersist && host_word(ctx, HW_FAIL))) {
        if (viaPersist) it = 0;
        int prc = solve_fp64(ctx, fused, nextCheck, done, it);
        if (prc) return prc;
    }
    // the fused loop ping-pongs r between the caller's buffer and r2: leave the struct as it was found
    if (k.r != r_entry) { k.r2 = k.r; k.r = r_entry; }
    // a system that hit the iteration cap or broke down has been deactivated like a converged one: "no active systems"
    // is then not "solved" (the host learns it from the mapped failure word at the poll that ended the loop)
    ctx->solveFail = host_word(ctx, HW_FAIL);
    if (ctx->solveFail) done = false;
    guess = it;        // (launched iterations; collect_stats replaces it with the iterations actually needed)

    ctx->ss.solveDone[kind] = done;
    ctx->specValid = spec && ctx->cfg.specOn && outcome == PsOutcome::Done && done;       // (the device decided the same from the same words: k_cocg_persist's exit)
    return solve_epilogue(ctx, kind, x, done, deferEnd, guard);
}

// residual + first pre-smoothing pass of a solve (k_resid_pre); threads by tile size like the stencil kernels of the iteration
// (HMCMT_RESID = 256 / 512 / 1024)
void launch_resid_pre(hmcmt_ctx* ctx, size_t lds, const cplx* x, int zero_r) {
    const Solver& k = ctx->sv;
    const dim3 grid(k.NTR, k.S);
    if (ctx->cfg.residThreads == 1024) hipLaunchKernelGGL(k_resid_pre<1024>, grid, dim3(1024), lds, ctx->stream, k, x, k.r, k.r2, zero_r, ctx->v.sysOn);
    else if (ctx->cfg.residThreads == 512) hipLaunchKernelGGL(k_resid_pre<512>, grid, dim3(512), lds, ctx->stream, k, x, k.r, k.r2, zero_r, ctx->v.sysOn);
    else hipLaunchKernelGGL(k_resid_pre<256>, grid, dim3(256), lds, ctx->stream, k, x, k.r, k.r2, zero_r, ctx->v.sysOn);
}

// weights of the initial-guess extrapolation for solve kind kd (side stream): partial sums, weights, history shift
void launch_extrap_weights(hmcmt_ctx* ctx, const double* d_m, int kd, hipStream_t sp) {
    hipLaunchKernelGGL(k_extrap_prepare, dim3(EXT_NBLK), dim3(256), 0, sp, d_m, ctx->d_mHist[kd], ctx->v.nAC, ctx->d_ext[kd],
                       ctx->cfg.extrapNp, kd == 1 ? 1 : 0, ctx->v.ticks);
}

// side stream, beside the forward solve: the adjoint initial guess and the sigma-only sensitivity tables (joined
// before the adjoint residual / before k_bcsens).  Called when the main queue is well filled, so that the host's
// dozen API calls do not leave the device idle.
void launch_adjoint_side(hmcmt_ctx* ctx) {
    if (!ctx->sidePending) return;
    ctx->sidePending = false;
    const View& v = ctx->sideView;
    const int S = v.S;
    if (ctx->sideExtrap) {
        launch_extrap_weights(ctx, ctx->sideM, 1, ctx->side);
        hipLaunchKernelGGL(k_extrap, dim3(ctx->sv.NB, S), dim3(VBLOCK), 0, ctx->side, ctx->sv, v.Lam, ctx->d_prevField[1], ctx->d_ext[1]);
        if (ctx->guessCapture) hipMemcpyAsync(ctx->d_guessCap[1], v.Lam, (size_t)S * v.vstride * sizeof(cplx), hipMemcpyDeviceToDevice, ctx->side);
        hipEventRecord(ctx->evExtA, ctx->side);
        ctx->extAWaitPending = true;
    }
    if (ctx->sideSens) {
        hipStreamWaitEvent(ctx->side, ctx->evPiv, 0);          // (the lateral means come from the second side stream)
        // One launch (k_sens_fused) where the persistent kernel fills the chip: the side stream's kernels then run as the first systems
        // converge, 0.2 ms instead of 0.37 at the headline size.  Where a solve leaves CUs free (the stress size: 240 of 256) the three
        // small kernels trickle along on them for milliseconds, harmlessly -- the side stream gets next to nothing of the machine
        // beside a solve there: the adjoint guess in front takes the whole forward solve, ANY kernel behind it starts at the adjoint
        // solve's own start, and the fused one's workgroups (LDS, 256 threads) then sit on CUs that solve's workgroups need (measured:
        // 84.2 against 85.0 steps/s; the tables in front of the guess: 83.5, the guess then delays the adjoint solve).
        if (ctx->cfg.sensFusedLds > 0 && (ctx->cfg.sensFusedAlways || !persist_ok(ctx) || ctx->cfg.persistFillsShare)) {
            hipLaunchKernelGGL(k_sens_fused, dim3(3, S), dim3(std::min(256, (v.nz + 1 + 63) / 64 * 64)), ctx->cfg.sensFusedLds, ctx->side, v);
        } else {
            hipLaunchKernelGGL(k_sens_layers, dim3((v.nz + 1 + 63) / 64, 3, S), dim3(64), 0, ctx->side, v);
            hipLaunchKernelGGL(k_sens_profile, dim3((3 * S + 63) / 64), dim3(64), 0, ctx->side, v);
            // the serial half of dBC^T w (78 us on a handful of CUs) depends on sigma only: here, not after the adjoint solve
            hipLaunchKernelGGL(k_bcsens_pre, dim3((v.nz + 63) / 64, 3, S), dim3(64), 0, ctx->side, v);
        }
        hipEventRecord(ctx->evSens, ctx->side);
    }
}

// the whole hot path on device buffers
int evaluate_once(hmcmt_ctx* ctx, const double* d_m, bool wantGrad, double* d_pred, double* d_misfit, double* d_grad);
int evaluate(hmcmt_ctx* ctx, const double* d_m, bool wantGrad, double* d_pred, double* d_misfit, double* d_grad) {
    ctx->persistTimedOut = false;
    int rc = evaluate_once(ctx, d_m, wantGrad, d_pred, d_misfit, d_grad);
    if (ctx->persistTimedOut) {
        // (solve(): a wait of the persistent kernel timed out.)  Everything in flight is drained, the leapfrog position update --
        // done by the first attempt's first kernel -- is not repeated, no warm start from fields in an undefined state
        ctx->persistTimedOut = false;
        fprintf(stderr, "libhmcmt_hip: a wait of the persistent solve kernel timed out (the device is shared?); this context continues with the "
                        "launch-per-phase loop for the next %ld solves, the evaluation is redone\n", ctx->ss.persistBackoff);
        (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->side);
        (void)hipGetLastError();
        ctx->statsPending = false; ctx->sidePending = false; ctx->sensWaitPending = ctx->extAWaitPending = false;
        ctx->ss.haveFwd = ctx->ss.haveAdj = false; ctx->ss.lastItFwd = ctx->ss.lastItAdj = 0;
        ctx->ss.lfStep.on = 0;
        ctx->solveFail = 0;
        host_word(ctx, HW_FAIL) = 0;
        rc = evaluate_once(ctx, d_m, wantGrad, d_pred, d_misfit, d_grad);
    }
    return rc;
}
int evaluate_once(hmcmt_ctx* ctx, const double* d_m, bool wantGrad, double* d_pred, double* d_misfit, double* d_grad) {
    View v = ctx->v;
    v.m = d_m;
    v.dbg = ctx->ss.dbgFlags;
    if (d_pred) v.pred = reinterpret_cast<cplx*>(d_pred);
    if (d_grad) v.grad = d_grad;
    hipStream_t st = ctx->stream;
    const int S = v.S;
    { int prc = collect_pending(ctx); if (prc) return prc; }      // (an earlier asynchronous evaluation's records / status)
    ctx->jvp.valid = false;             // (the evaluation arrays leave the linearisation point of hmcmt_linearize)
    ctx->stats = hmcmt_stats{};
    ctx->stats.nsystems = S;
    ++ctx->ss.evalCount;
    ++ctx->stateGen;
    ctx->sv.cntActive = (ctx->ss.profMask && ctx->ss.evalCount % ctx->profEvery == 0) ? ctx->d_cnt : nullptr;
    if (ctx->sv.cntActive) ++ctx->profEvals;
    ctx->evalSampled = ctx->sv.cntActive != nullptr;
    ctx->guardNow = !ctx->opt.verify && ctx->ss.guardEvery > 0 && ctx->ss.evalCount % ctx->ss.guardEvery == 0;
    if (ctx->ss.guardDropWarm) { ctx->ss.guardDropWarm = false; ctx->ss.haveFwd = ctx->ss.haveAdj = false; }
    const int nodes = v.NZP * (v.ny + 1);
    const size_t vecBytes = (size_t)S * v.vstride * sizeof(cplx);
    // initial guesses (options.warm_start): verify checks against the cold right-hand side
    // (test hook hmcmt_debug_flags bit 0: the Dirichlet values stay those of the previous evaluation -- they live in the
    //  boundary nodes of X, so the forward solve must start from the previous fields)
    const bool freezeBC = (ctx->ss.dbgFlags & 1) && ctx->ss.haveFwd;
    if (freezeBC && ctx->opt.verify) { ctx->err = "hmcmt_debug_flags: frozen boundary values and options.verify exclude each other"; return HMCMT_EINVAL; }
    const bool warmF = (ctx->opt.warm_start && ctx->ss.haveFwd && !ctx->opt.verify) || freezeBC;
    const bool warmA = ctx->opt.warm_start && ctx->ss.haveAdj && !ctx->opt.verify;
    const bool extrap = ctx->opt.warm_start == 2 && !ctx->opt.verify;
    // start of a solve on the default path: residual and first pre-smoothing pass in one launch (k_resid_pre)
    const size_t startLds = (size_t)(2 * ctx->sv.RT + 6) * v.NYP * sizeof(cplx);
    const bool fusedStartOk = ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI && ctx->opt.fdm_precision == 0 && !ctx->opt.verify &&
                              startLds <= (size_t)150 * 1024 && !ctx->cfg.noFusedStart;
    const int sweepsF = pick_sweeps(ctx, 0), sweepsA = pick_sweeps(ctx, 1);
    bool fusedStart = fusedStartOk && sweepsF == 1;      // (k_resid_pre does ONE pre-sweep; two go through k_resid0 + the solve's own start)
    // the solves' start -- initial residual, bookkeeping -- inside the persistent kernel (kernels_persist.h, PsLaunch::resid / begin)
    const bool inKernelStart = ctx->cfg.psInKernelStart && ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI && ctx->opt.fdm_precision == 0 && !ctx->opt.verify && persist_ok(ctx);
    ctx->sv.sweeps = sweepsF;
    ctx->stats.smoother_sweeps = 10 * sweepsF + (wantGrad ? sweepsA : 0);
    ctx->ss.sweepsUsed[0] = sweepsF; if (wantGrad) ctx->ss.sweepsUsed[1] = sweepsA;
    {
        ProfScope ps(ctx, 4);
        // conductivities and their lateral means, one wave per cell row (meshes of whole rows: always; k_sigma + k_rowmean otherwise)
        const bool rows = v.nCell == v.ny * v.nz && !ctx->cfg.noSigmaRows;
        const auto hostT0 = std::chrono::steady_clock::now();
        if (v.ticks) {                                   // HMCMT_TICKS: earliest starts <- max, latest ends <- 0
            HIPCHK(hipMemsetAsync(v.ticks, 0xff, 32 * sizeof(long long), st));
            HIPCHK(hipMemsetAsync(v.ticks + 32, 0, 64 * TK_N * sizeof(long long), st));
        }
        // initial guesses: zero on a cold start, otherwise the previous fields, optionally extrapolated
        if (!warmF) {
            HIPCHK(hipMemsetAsync(v.X, 0, vecBytes, st));
            HIPCHK(hipMemsetAsync(ctx->d_ext[0], 0, EXT_PART * sizeof(double), st));
        }
        if (wantGrad && !warmA) {
            HIPCHK(hipMemsetAsync(v.Lam, 0, vecBytes, st));
            HIPCHK(hipMemsetAsync(ctx->d_ext[1], 0, EXT_PART * sizeof(double), st));
        }
        // The coefficients run on the MAIN stream behind the boundary fields (until round 3 on a second side stream: alone they take
        // 10 us instead of 20 beside k_bc_fused, and three API calls -- wait, record, wait -- leave the host's sequence in front of the
        // residual: 860 -> 870 steps/s on the straight-line trajectories, +0.5 % elsewhere; the other placement was removed in round 4).
        hipStream_t sA = ctx->side, sB = st;
        // (a position update of the device-resident leapfrog that is still due rides along: leapfrog_core)
        if (ctx->ss.lfStep.on && !(rows && ctx->ss.lfStep.L.m == v.m)) {
            hipLaunchKernelGGL(k_lf_step, dim3((ctx->ss.lfStep.L.n + 127) / 128), dim3(128), 0, st, ctx->ss.lfStep.L, ctx->ss.lfStep.dt, ctx->ss.lfStep.lo, ctx->ss.lfStep.hi);
            ctx->ss.lfStep.on = 0;
        }
        if (rows) hipLaunchKernelGGL(k_sigma_rows, dim3(v.nz), dim3(64), 0, st, v, ctx->ss.lfStep);
        else hipLaunchKernelGGL(k_sigma, grid1(v.nCell, 256), dim3(256), 0, st, v);
        ctx->ss.lfStep.on = 0;
        HIPCHK(hipEventRecord(ctx->evModel, st));
        // Two chains start from sigma and meet at the forward residual (in-kernel timeline HMCMT_TICKS=1; near the true model
        // the first preconditioner application starts 92 us after k_sigma_rows, 131 us at the start of round 3):
        //   main    the 1-D boundary fields: per-layer terms and serial recurrences in one launch (k_bc_fused, 35 us), then the
        //           stencil coefficients + Jacobi diagonal + packed float copy (k_coef_all, 10 us), then the residual
        //   side    the extrapolated forward guess (weights from the model history, one pass over the fields: 15 + 15 us; the
        //           residual waits for it), then the FDM background -> inverse pivots of its tridiagonals (serial, 19-60 us;
        //           the first preconditioner application waits for them)
        // This stretch is bound by the host's 4-7 us per API call and by waits on events that are not yet complete when the
        // queue reaches them, not by the kernels: the order of the calls is the schedule, and every call
        // that could be dropped or moved to where the host runs ahead of the device has been.
        if (!freezeBC) {
            if (ctx->cfg.bcCW > 0) {
                hipLaunchKernelGGL(k_bc_fused, dim3((v.ny + ctx->cfg.bcCW) / ctx->cfg.bcCW, v.nFreq), dim3(256), ctx->cfg.bcLds, st, v, ctx->cfg.bcCW, ctx->cfg.bcSlots);
            } else if (ctx->cfg.bcbCW > 0) {
                hipLaunchKernelGGL(k_bc_blocked, dim3((v.ny + ctx->cfg.bcbCW) / ctx->cfg.bcbCW, v.nFreq), dim3(ctx->cfg.bcbNT), ctx->cfg.bcbLds, st, v, ctx->cfg.bcbCW, ctx->cfg.bcbSlots, ctx->cfg.bcbLBu, ctx->cfg.bcbLBd);
            } else {
                hipLaunchKernelGGL(k_bc_layers, dim3((v.ny + 1 + 63) / 64, v.nz, v.nFreq), dim3(64), 0, st, v);
                hipLaunchKernelGGL(k_bc_forward, dim3((v.ny + 1 + 63) / 64, v.nFreq), dim3(64), 4 * (size_t)v.nz * sizeof(cplx), st, v);
            }
        }
        const bool pivots = ctx->opt.precond != HMCMT_PRECOND_JACOBI;
        // the FDM background -> inverse pivots (serial, 17-60 us; the first preconditioner application waits for them)
        auto issue_pivot = [&](hipStream_t sp) {
            if (!rows) hipLaunchKernelGGL(k_rowmean, dim3(v.nz), dim3(64), 0, sp, v);
            if (pivots)
                hipLaunchKernelGGL(k_pivot, dim3((v.ny - 1 + 63) / 64, S), dim3(64), 4 * (size_t)v.NZP * sizeof(double), sp, v,
                                   ctx->opt.fdm_precision == 0 ? ctx->inst.d_invp32 : (float2*)nullptr);
            else
                hipLaunchKernelGGL(k_fdm_z, grid1(2 * v.NZP, 64), dim3(64), 0, sp, v);
            return hipEventRecord(ctx->evPiv, sp);
        };
        HIPCHK(hipStreamWaitEvent(sA, ctx->evModel, 0));
        if (extrap) {
            // (interior nodes only -- the boundary-value kernel owns the boundary nodes of X)
            launch_extrap_weights(ctx, d_m, 0, sA);
            hipLaunchKernelGGL(k_extrap, dim3(ctx->sv.NB, S), dim3(VBLOCK), 0, sA, ctx->sv, v.X, ctx->d_prevField[0], ctx->d_ext[0]);
            // (test hook: the boundary nodes of this copy race with the boundary-value kernel on the main stream -- interior nodes only)
            if (ctx->guessCapture) HIPCHK(hipMemcpyAsync(ctx->d_guessCap[0], v.X, vecBytes, hipMemcpyDeviceToDevice, sA));
            HIPCHK(hipEventRecord(ctx->evExtF, sA));
        }
        HIPCHK(issue_pivot(sA));
        if (ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI && !ctx->cfg.noCoefAll) {
            // (the per-system Jacobi diagonals only where something will read them: not the persistent kernel -- ensure_dinv)
            const bool lazy = ctx->cfg.lazyDinv && inKernelStart;
            hipLaunchKernelGGL(k_coef_all, dim3(lazy ? std::max(ctx->sv.NB, (int)std::min<long>(512, (v.vstride + VBLOCK - 1) / VBLOCK)) : ctx->sv.NB, lazy ? 2 : S), dim3(VBLOCK), 0, sB, v, ctx->sv, ctx->cfg.jacobiW, const_cast<float4*>(ctx->sv.cf32),
                               lazy ? v.nFreq : 1);
            ctx->inst.dinvValid = !lazy;
        } else {
            hipLaunchKernelGGL(k_coef, grid1(nodes, 256), dim3(256), 0, sB, v, 0, 1, 1, 0);
            if (ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI) {
                hipLaunchKernelGGL(k_dinv, dim3(ctx->sv.NB, S), dim3(VBLOCK), 0, sB, ctx->sv, ctx->cfg.jacobiW);
                hipLaunchKernelGGL(k_coef32, dim3(ctx->sv.NB, 2), dim3(VBLOCK), 0, sB, ctx->sv, const_cast<float4*>(ctx->sv.cf32));
            }
        }
        if (extrap) HIPCHK(hipStreamWaitEvent(st, ctx->evExtF, 0));
        // r = -Aio*bc - Aii*x0 with x0 = previous solution (or 0): one stencil pass over X -- inside the persistent kernel's per-system
        // set-up where that kernel runs the solve (round 6: k_resid0 + its launch boundary were 25 us in front of the forward solve)
        if (inKernelStart) {
            ctx->psStart.resid = 1; ctx->psStart.begin = 1;
            ctx->solveBegun = true;
            fusedStart = false;
        } else
        if (fusedStart) {
            launch_resid_pre(ctx, startLds, v.X, 1);
            std::swap(ctx->sv.r, ctx->sv.r2);             // (the residual went to the second buffer; swapped back after the solve)
            ctx->solveBegun = ctx->preDone = true;
        } else {
            hipLaunchKernelGGL(k_resid0, dim3(ctx->sv.NB, S), dim3(VBLOCK), 0, st, ctx->sv, v.X, 1, ctx->opt.verify ? nullptr : ctx->v.sysOn, 0);
            ctx->solveBegun = !ctx->opt.verify;
        }
        if (ctx->cfg.wantTicks) { ctx->hostUs[0] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hostT0).count(); ++ctx->hostN; }
        HIPCHK(hipStreamWaitEvent(st, ctx->evPiv, 0));
        // (the adjoint half's side-stream work -- its initial guess, the sigma-only sensitivity tables -- is launched
        // from inside the forward solve, once the main queue holds two iterations: launch_adjoint_side)
        ctx->sideView = v; ctx->sideM = d_m; ctx->sideExtrap = extrap && wantGrad; ctx->sideSens = wantGrad;
        ctx->sidePending = wantGrad;
    }
    // Followers of the two solves that need nothing but the View (receiver functionals and adjoint sources behind the forward solve;
    // the gradient's tail behind the adjoint one) are handed to solve() to be queued behind the persistent launch at once (SpecFn).
    // Only where that is the plain case: a gradient evaluation with a warm adjoint start (no clearing of the right-hand side), no
    // true-residual check, no guard copy, no HIP-event sampling.
    // (round 6: with the solve's start inside the persistent kernel a COLD adjoint start is the sparse case too -- r = b - A 0 with b read on the
    //  receiver layer's two node rows: no 11 MB fill of the right-hand side in front of k_src, and the followers are queued speculatively as well)
    const bool sparseSrcPlan = (warmA || inKernelStart) && !ctx->opt.verify && !ctx->guardNow;
    const bool specPlain = wantGrad && sparseSrcPlan && !ctx->evalSampled;
    const int nsrcBlocks = (2 * (v.ny + 1) + 127) / 128;
    double* const misfitPtr = d_misfit ? d_misfit : ctx->d_misfit;
    const SpecFn specF = [&](const int* gate, int gen) {
        View vg = v; vg.gate = gate; vg.gateGen = gen;
        hipLaunchKernelGGL(k_rxall, grid1(S * v.nRx, 64), dim3(64), 0, st, vg, 1, solve_rec(ctx, 0));
        hipLaunchKernelGGL(k_src, dim3(nsrcBlocks + (v.ny + 127) / 128, S), dim3(128), 0, st, vg, misfitPtr, nsrcBlocks);
    };
    int rc = solve(ctx, v.X, 0, true, specPlain ? &specF : nullptr);
    const bool specFwd = ctx->specValid;
    if (fusedStart) std::swap(ctx->sv.r, ctx->sv.r2);
    fusedStart = fusedStartOk && sweepsA == 1 && !inKernelStart;
    ctx->sv.sweeps = sweepsA;
    if (rc == 0 && ctx->solveFail) {
        launch_solve_end(ctx, 0);
        // the forward solve gave up (iteration cap / breakdown): no adjoint solve on its fields, no further leapfrog step on
        // its gradient -- the records of k_solve_end carry the status, the caller gets it now
        ctx->sidePending = false;
        // (side-stream work of the adjoint half that is already in flight -- its initial guess writes Lam, the sensitivity tables --
        //  must not run into the next evaluation: joined here, the pending waits dropped)
        if (ctx->extAWaitPending) { ctx->extAWaitPending = false; HIPCHK(hipStreamWaitEvent(st, ctx->evExtA, 0)); }
        if (ctx->sideSens && !ctx->sidePending) HIPCHK(hipStreamSynchronize(ctx->side));
        ctx->sensWaitPending = false;
        HIPCHK(hipEventRecord(ctx->evRec, st));
        ctx->ss.haveFwd = false;
        rc = collect_stats(ctx, false);
        return rc ? rc : finish_status(ctx);
    }
    const auto hostT1 = std::chrono::steady_clock::now();
    launch_adjoint_side(ctx);            // (no-op when the solve has already done it)
    ctx->ss.haveFwd = (rc == 0 && ctx->ss.solveDone[0]);
    if (rc) return rc;
    if (!specFwd) {
        ProfScope ps(ctx, 5);
        hipLaunchKernelGGL(k_rxall, grid1(S * v.nRx, 64), dim3(64), 0, st, v, wantGrad ? 1 : 0, solve_rec(ctx, 0));     // (+ the forward solve's records)
        if (!wantGrad) {
            HIPCHK(hipEventRecord(ctx->evRec, st));      // behind the records of the last solve
            hipLaunchKernelGGL(k_misfit, dim3(1), dim3(256), 0, st, v, d_misfit ? d_misfit : ctx->d_misfit);
        }
    }
    if (wantGrad) {
        {
            ProfScope ps(ctx, 5);
            // k_src assigns the two node rows of the receiver layer and all of srcB.  A warm adjoint start reads the right-hand
            // side on those rows only (k_resid0 / k_resid_pre, zero_r = 2 + row); a cold one takes the buffer as its residual
            const bool sparseSrc = sparseSrcPlan;                                     // (a guarded evaluation keeps a copy of the whole right-hand side)
            if (!specFwd) {
                if (!sparseSrc) HIPCHK(hipMemsetAsync(v.R, 0, vecBytes, st));
                hipLaunchKernelGGL(k_src, dim3(nsrcBlocks + (v.ny + 127) / 128, S), dim3(128), 0, st, v, misfitPtr, nsrcBlocks);
            }
            if (ctx->guardNow) HIPCHK(hipMemcpyAsync(ctx->inst.d_b, v.R, vecBytes, hipMemcpyDeviceToDevice, st));
            if (ctx->extAWaitPending) { ctx->extAWaitPending = false; HIPCHK(hipStreamWaitEvent(st, ctx->evExtA, 0)); }   // (a forward solve too short to have issued it)
            if (inKernelStart && persist_ok(ctx)) {
                // (warm start: r = b - A lambda0 with b on the receiver layer's two node rows; cold: the buffer k_src has filled IS the residual)
                ctx->psStart.resid = (warmA || sparseSrc) ? (sparseSrc ? 2 + v.zid : PS_RESID_FULL) : 0; ctx->psStart.begin = 1;
                ctx->solveBegun = true;
            } else
            if (warmA && fusedStart) {
                ensure_dinv(ctx);
                launch_resid_pre(ctx, startLds, v.Lam, sparseSrc ? 2 + v.zid : 0);
                std::swap(ctx->sv.r, ctx->sv.r2);
                ctx->solveBegun = ctx->preDone = true;
            } else if (warmA || sparseSrc) {      // (cold and sparse: the persistent kernel was to start this solve and is off since the forward one -- lambda0 = 0, r = b)
                ensure_dinv(ctx);
                hipLaunchKernelGGL(k_resid0, dim3(ctx->sv.NB, S), dim3(VBLOCK), 0, st, ctx->sv, v.Lam, sparseSrc ? 2 + v.zid : 0, ctx->v.sysOn, 0);
                ctx->solveBegun = true;
            }
        }
        ctx->sensWaitPending = true;     // (the wait for the side stream's sensitivity tables is issued from inside the adjoint solve)
        if (ctx->cfg.wantTicks) ctx->hostUs[1] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hostT1).count();
        const SpecFn specA = [&](const int* gate, int gen) {
            View vg = v; vg.gate = gate; vg.gateGen = gen;
            if (ctx->sensWaitPending) { ctx->sensWaitPending = false; hipStreamWaitEvent(st, ctx->evSens, 0); }
            { const int nwbx = (v.nz + v.ny + 127) / 128, ngcx = (v.nCell + 127) / 128;       // (k_wb + k_gradcell: one launch)
              hipLaunchKernelGGL(k_wb_gradcell, dim3(nwbx * S + ngcx * 2 * GRAD_NG), dim3(128), 0, st, vg, solve_rec(ctx, 1), nwbx, ngcx); }
            hipEventRecord(ctx->evRec, st);
            hipLaunchKernelGGL(k_bcsens_contract, dim3((BCC_L * v.nz + 127) / 128, 2, S), dim3(128), 0, st, vg, ctx->ss.lfMom.on ? ctx->ss.lfMom.L.part : (double*)nullptr);
            hipLaunchKernelGGL(k_gradfinal, grid1(GF_L * v.nAC, 128), dim3(128), 0, st, vg, ctx->ss.lfMom);
        };
        rc = solve(ctx, v.Lam, 1, true, specPlain ? &specA : nullptr);
        const bool specAdj = ctx->specValid;
        const auto hostT2 = std::chrono::steady_clock::now();
        if (warmA && fusedStart) std::swap(ctx->sv.r, ctx->sv.r2);
        ctx->ss.haveAdj = (rc == 0 && ctx->ss.solveDone[1]);
        if (rc) return rc;
        if (ctx->solveFail) {             // (as after the forward solve: no gradient from a failed adjoint, and the caller knows NOW)
            if (ctx->sensWaitPending) { ctx->sensWaitPending = false; HIPCHK(hipStreamSynchronize(ctx->side)); }   // (the tables of the side stream: not into the next evaluation)
            launch_solve_end(ctx, 1);
            HIPCHK(hipEventRecord(ctx->evRec, st));
            rc = collect_stats(ctx, true);
            return rc ? rc : finish_status(ctx);
        }
        if (!specAdj) {
            ProfScope ps(ctx, 6);
            if (ctx->sensWaitPending) { ctx->sensWaitPending = false; HIPCHK(hipStreamWaitEvent(st, ctx->evSens, 0)); }     // (a solve of fewer than 8 iterations)
            { const int nwbx = (v.nz + v.ny + 127) / 128, ngcx = (v.nCell + 127) / 128;       // (k_wb (+ the adjoint solve's records) + k_gradcell: one launch)
              hipLaunchKernelGGL(k_wb_gradcell, dim3(nwbx * S + ngcx * 2 * GRAD_NG), dim3(128), 0, st, v, solve_rec(ctx, 1), nwbx, ngcx); }
            HIPCHK(hipEventRecord(ctx->evRec, st));                        // behind the records of the last solve
            hipLaunchKernelGGL(k_bcsens_contract, dim3((BCC_L * v.nz + 127) / 128, 2, S), dim3(128), 0, st, v, ctx->ss.lfMom.on ? ctx->ss.lfMom.L.part : (double*)nullptr);
            hipLaunchKernelGGL(k_gradfinal, grid1(GF_L * v.nAC, 128), dim3(128), 0, st, v, ctx->ss.lfMom);
        }
        if (ctx->cfg.wantTicks) ctx->hostUs[2] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hostT2).count();
    }
    HIPCHK(hipGetLastError());
    ctx->ss.haveModel = true;
    return 0;
}

// Meshes whose systems do not all fit the chip at once (cfg5: 64 systems, one per XCD at a time) run them through 8 x slots
// queues, and a queue's time is the SUM of its systems' iterations: taken in index order (XCD x: systems x, x + 8, ..) the longest
// queue of the cfg5 chain holds 3.5 % more iterations than the mean (forward; 2.9 % adjoint) and the other XCDs idle at the end of
// every solve.  The iteration counts of consecutive solves of a chain differ by one or two, so the last solve's counts are the
// next one's costs: longest-first into the least loaded queue that has room (every queue keeps its number of systems: the
// kernel's loop bounds do not change).  A new table is taken when the present one is more than 1 % behind it.
// (the packing alone -- pure arithmetic, also behind hmcmt_persist_pack: position q = queue + NQ * round of the table -> system)
static double queues_makespan(const float* cost, int S, int NQ, const int* tab) {
    double worst = 0;
    for (int j = 0; j < NQ; ++j) { double t = 0; for (int q = j; q < S; q += NQ) t += cost[tab ? tab[q] : q]; worst = std::max(worst, t); }
    return worst;
}
static void pack_queues(const float* cost, int S, int NQ, int* tab) {
    std::vector<int> idx(S), fill(NQ, 0);
    std::vector<double> load(NQ, 0.0);
    for (int i = 0; i < S; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    for (int i = 0; i < S; ++i) {
        int best = -1;
        for (int j = 0; j < NQ; ++j) {
            if (j + NQ * fill[j] >= S) continue;                       // (the queue is full)
            if (best < 0 || load[j] < load[best]) best = j;
        }
        tab[best + NQ * fill[best]] = idx[i];
        ++fill[best]; load[best] += cost[idx[i]];
    }
    // (with queues of unequal length the greedy table can lose to the index order on a handful of systems: then that one)
    if (queues_makespan(cost, S, NQ, tab) > queues_makespan(cost, S, NQ, nullptr)) for (int i = 0; i < S; ++i) tab[i] = i;
}
void persist_balance(hmcmt_ctx* ctx, int kind) {
    const int S = ctx->sv.S, NQ = 8 * ctx->inst.persistSlots;
    if (!ctx->cfg.psBalance || !ctx->d_psOrder || NQ <= 0 || S <= NQ) return;
    // (costs: the mean of the last solve's counts and the costs before it -- the counts of one system wander by one or two from
    //  step to step, and a table made from one solve's noise is a worse guess for the next than one made from several)
    std::vector<float>& cost = ctx->ss.psCost[kind];
    const int* last = ctx->ss.itersLast.data() + (size_t)kind * S;
    if (cost.empty()) cost.assign(last, last + S);
    else for (int i = 0; i < S; ++i) cost[i] = ctx->cfg.psSmooth * cost[i] + (1.f - ctx->cfg.psSmooth) * (float)last[i];
    std::vector<int> tab(S);
    pack_queues(cost.data(), S, NQ, tab.data());
    std::vector<int>& cur = ctx->ss.psOrder[kind];
    const double now = queues_makespan(cost.data(), S, NQ, cur.empty() ? nullptr : cur.data()), lpt = queues_makespan(cost.data(), S, NQ, tab.data());
    if (now <= 1.01 * lpt) return;
    std::memcpy(ctx->h_psOrder + (size_t)kind * S, tab.data(), sizeof(int) * S);
    // (stream order: behind every launch that reads the old table, in front of the next solve)
    if (hipMemcpyAsync(ctx->d_psOrder + (size_t)kind * S, ctx->h_psOrder + (size_t)kind * S, sizeof(int) * S, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    cur = tab;
    ++ctx->ss.psRebalanced;
}

// the per-solve records (written by k_solve_end into mapped pinned memory) -> statistics; the caller has waited for them
void parse_stats(hmcmt_ctx* ctx, bool withAdjoint) {
    const int S = ctx->v.S, nk = withAdjoint ? 2 : 1;
    const int* h_iters = reinterpret_cast<const int*>(ctx->inst.h_rec);
    const int* h_status = h_iters + 2 * S;
    const double* h_err = ctx->inst.h_rec + 2 * S;
    for (int kind = 0; kind < nk; ++kind) {
        int mx = 0, sum = 0;
        for (int s = 0; s < S; ++s) {
            const int itv = h_iters[kind * S + s];
            ctx->ss.itersLast[kind * S + s] = itv;
            mx = std::max(mx, itv); sum += itv;
            if (h_status[kind * S + s] != 0 && ctx->stats.status == 0) ctx->stats.status = h_status[kind * S + s];
            if (h_err[kind * S + s] > ctx->stats.err_est_max) ctx->stats.err_est_max = h_err[kind * S + s];
        }
        if (ctx->evalSampled) ctx->profSerialIts += mx + 1;
        if (kind == 0) { ctx->stats.iters_fwd_max = mx; ctx->stats.iters_fwd_sum = sum; }
        else { ctx->stats.iters_adj_max = mx; ctx->stats.iters_adj_sum = sum; }
        // first convergence poll of the next evaluation: where this one actually finished (the loop itself only
        // knows how many iterations it launched, which includes the empty ones behind the last poll)
        if (ctx->ss.solveDone[kind] && mx > 0) (kind == 0 ? ctx->ss.lastItFwd : ctx->ss.lastItAdj) = mx;
        if (ctx->ss.solveDone[kind] && mx > 0 && ctx->stats.status == 0 && persist_fits(ctx) && ctx->ss.persistOn) persist_balance(ctx, kind);
        // ... and the smoother of the next solve of this kind (pick_sweeps): two sweeps per side when this one was long
        if (ctx->cfg.sweepsMode == 0 && ctx->ss.solveDone[kind] && mx > 0) {
            int& next = ctx->ss.sweepsKind[kind];
            if (ctx->ss.sweepsUsed[kind] == 1) {
                if (ctx->ss.sweepsProbe[kind]) {                 // a probe with one sweep: keep it if it is the cheaper one
                    ctx->ss.sweepsProbe[kind] = false;
                    const double cost2 = (persist_fits(ctx) && ctx->ss.persistOn) ? (ctx->cfg.persistCS > 1 ? SWEEPS2_COST_PERSIST_CS2 : SWEEPS2_COST_PERSIST) : SWEEPS2_COST;
                    next = (double)mx <= cost2 * ctx->ss.sweepsCount2[kind] ? 1 : 2;
                } else if (mx > ctx->cfg.sweepsUp) next = 2;
            } else {
                ctx->ss.sweepsCount2[kind] = mx;
                if (mx < ctx->cfg.sweepsDown) next = 1;
                else if (++ctx->ss.sweepsSince[kind] >= SWEEPS_PROBE_EVERY && mx < ctx->cfg.sweepsUp) {
                    ctx->ss.sweepsSince[kind] = 0; ctx->ss.sweepsProbe[kind] = true; next = 1;
                }
            }
        }
        if (!ctx->ss.solveDone[kind] && ctx->stats.status == 0) ctx->stats.status = HMCMT_ENOCONV;
    }
    if (ctx->stats.status != 0) {
        // a failed evaluation (breakdown, non-finite values, iteration cap) must not seed the next one: its fields may
        // hold Inf/NaN, and so may the extrapolation history -- the next call starts cold
        ctx->ss.haveFwd = ctx->ss.haveAdj = false;
        ctx->ss.lastItFwd = ctx->ss.lastItAdj = 0;
    }
    if (!withAdjoint) for (int s = 0; s < S; ++s) ctx->ss.itersLast[S + s] = 0;
}

// after an evaluation: wait for the whole stream, then the statistics
int collect_stats(hmcmt_ctx* ctx, bool withAdjoint) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    parse_stats(ctx, withAdjoint);
    ctx->statsPending = false;
    return 0;
}

int finish_status(hmcmt_ctx* ctx);

// An asynchronous evaluation (hmcmt_grad_device_async) leaves its records unread: they are picked up -- waiting only
// for the event behind its last k_solve_end, not for its gradient tail -- before the next evaluation is issued
// (its first poll wants the iteration counts, and k_solve_end will overwrite the records) or by hmcmt_wait.
int collect_pending(hmcmt_ctx* ctx) {
    if (!ctx->statsPending) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipEventSynchronize(ctx->evRec));
    if (ctx->cfg.wantTicks) ctx->hostUs[3] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    parse_stats(ctx, ctx->pendingAdj);
    ctx->statsPending = false;
    return finish_status(ctx);
}

int finish_status(hmcmt_ctx* ctx) {
    if (ctx->stats.status == HMCMT_ENOCONV) { ctx->err = "iterative solve did not converge within maxit"; return HMCMT_ENOCONV; }
    if (ctx->stats.status == HMCMT_EBREAKDOWN) { ctx->err = "Krylov breakdown or non-finite values (NaN/Inf model?)"; return HMCMT_EBREAKDOWN; }
    return 0;
}

// test hook (hmcmt_debug_hog): workgroups that hold a CU's whole LDS and spin for a while -- a foreign tenant on the device
__global__ __launch_bounds__(64) void k_hog(long long ticks, int* started) {
    extern __shared__ __attribute__((aligned(16))) char hogmem[];
    hogmem[threadIdx.x] = (char)threadIdx.x;
    if (started && threadIdx.x == 0) __hip_atomic_fetch_add(started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (mapped host word: hmcmt_debug_hog waits for it)
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
    if (hogmem[threadIdx.x] == 77 && ticks < 0) hogmem[0] = 1;
}

}  // namespace

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
extern "C" {

static void chain_release(hmcmt_ctx* ctx);      // (host_chain.h)
static void map_release(hmcmt_ctx* ctx);        // (host_map.h)

void hmcmt_default_options(hmcmt_options* o) {
    if (!o) return;
    o->precond = HMCMT_PRECOND_FDM_JACOBI;
    o->maxit = 2000;
    o->tol = 1e-11;
    o->check_every = 2;
    o->verify = 0;
    o->warm_start = 2;
    o->fdm_precision = 0;
}

const char* hmcmt_last_error(const hmcmt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

int hmcmt_destroy(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    if (ctx->counted) {
        if (ctx->cfg.device >= 0 && ctx->cfg.device < MAXDEV) {
            for (int q = 0; q < 4; ++q) if ((ctx->cfg.shareMask >> q) & 1u) g_quarterUse[ctx->cfg.device][q].fetch_sub(1);
        }
        devlock_unref(ctx->cfg.device); ctx->counted = false;
    }
    hipSetDevice(ctx->cfg.device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->side) hipStreamSynchronize(ctx->side);      // (side-stream work of an evaluation nobody waited for)
    if (ctx->v.ticks) {
        static const char* names[TK_N] = {"k_sigma_rows", "k_bc_fused", "k_extrap_prepare (fwd)", "k_extrap (fwd)", "k_coef_all", "k_pivot",
            "k_resid_pre (fwd)", "k_spmv_fused (first .. last)", "k_update_fused (first .. last)", "k_fdm_fwd (first .. last)",
            "k_back_post (first .. last)", "k_solve_end (first .. last)", "k_rxall", "k_src", "k_resid_pre (adj)", "k_wb", "k_bcsens_contract",
            "k_gradcell", "k_gradfinal", "k_lf_momentum", "k_lf_dmmax", "k_lf_step", "k_sens_profile (side)", "k_cocg_persist (forward)", "k_cocg_persist (adjoint)"};
        std::vector<long long> traw(32 + 64 * TK_N);
        long long t[64] = {0};
        int rate = 100000;                                // kHz
        hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, ctx->cfg.device);
        if (hipMemcpy(traw.data(), ctx->v.ticks, traw.size() * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess) {
            for (int i = 0; i < TK_N; ++i) {
                t[i] = traw[i];
                for (int q = 0; q < 64; ++q) t[32 + i] = std::max(t[32 + i], traw[32 + 64 * i + q]);
            }
            fprintf(stderr, "HMCMT_TICKS: start .. end (us since the first kernel of the last evaluation), duration\n");
            long long t0 = 0x7fffffffffffffffLL;
            for (int i = 0; i < TK_N; ++i) if (t[i] > 0 && t[i] < t0) t0 = t[i];
            std::vector<int> order;
            for (int i = 0; i < TK_N; ++i) if (t[i] > 0) order.push_back(i);
            std::sort(order.begin(), order.end(), [&](int a, int b) { return t[a] < t[b]; });
            for (int i : order) {
                if (t[32 + i] > 0) fprintf(stderr, "  %9.1f %9.1f %8.1f   %s\n", (t[i] - t0) * 1e3 / rate, (t[32 + i] - t0) * 1e3 / rate, (t[32 + i] - t[i]) * 1e3 / rate, names[i]);
                else fprintf(stderr, "  %9.1f         -        -   %s\n", (t[i] - t0) * 1e3 / rate, names[i]);
            }
        }
        if (ctx->hostN) fprintf(stderr, "HMCMT_TICKS: host time of the launch sequences, mean of %ld evaluations: k_sigma .. forward residual %.1f us, "
                                "k_rxall .. adjoint residual %.1f us, gradient tail %.1f us, wait for the previous evaluation's records %.1f us\n", ctx->hostN, ctx->hostUs[0] / ctx->hostN,
                                ctx->hostUs[1] / ctx->hostN, ctx->hostUs[2] / ctx->hostN, ctx->hostUs[3] / ctx->hostN);
        hipFree(ctx->v.ticks);
    }
    if (ctx->d_pstamps) {                                // HMCMT_STAMPS=persist: phases of the third iteration of the last solve
        std::vector<long long> st(16 * 256);
        hipMemcpy(st.data(), ctx->d_pstamps, st.size() * sizeof(long long), hipMemcpyDeviceToHost);
        double acc[12] = {0}, sl[3] = {0}, bt[3] = {0}; long n = 0, nsl = 0, nbt = 0;
        for (int b = 0; b < 256; ++b) {
            const long long* p = &st[16 * b];
            if (!p[0] || !p[11]) continue;
            ++n;
            for (int i = 1; i < 12; ++i) acc[i] += (double)(p[i] - p[i - 1]);
            if (p[14] && p[15]) { ++nbt; bt[0] += (double)(p[14] - p[5]); bt[1] += (double)(p[15] - p[14]); bt[2] += (double)(p[6] - p[15]); }       // (back transform: planes -> LDS | MFMA loop | epilogue)
            if (p[12] && p[13]) { ++nsl; sl[0] += (double)(p[12] - p[3]); sl[1] += (double)(p[13] - p[12]); sl[2] += (double)(p[4] - p[13]); }   // (workgroups with a slab)
        }
#ifdef HMCMT_PS_DBGX
        fprintf(stderr, "HMCMT_PS_DBGX: halo copies that differ from the owners' values, by halo row j = 0..4: z3 %lld %lld %lld %lld %lld | zf %lld %lld %lld %lld %lld | p %lld (total)\n",
                st[16 * 254 + 0], st[16 * 254 + 1], st[16 * 254 + 2], st[16 * 254 + 3], st[16 * 254 + 4], st[16 * 254 + 5], st[16 * 254 + 6], st[16 * 254 + 7], st[16 * 254 + 8], st[16 * 254 + 9], st[16 * 255 + 12]);
        { const double* ex = reinterpret_cast<const double*>(&st[16 * 252]);
          fprintf(stderr, "   example (zf): mesh row %g col %g j %g half %g: owner %.9g %+.9gi, halo copy %.9g %+.9gi; r used by the copy %.9g %+.9gi, r published %.9g %+.9gi; workgroup %g system %g iteration %g\n",
                  ex[0], ex[1], ex[2], ex[3], ex[4], ex[6], ex[5], ex[7], ex[8], ex[13], ex[12], ex[14], ex[9], ex[10], ex[11]); }
#endif
        if (n) {
            int rate = 100000;                                // kHz
            hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, ctx->cfg.device);
            const double us = 1e3 / rate / n;
            double tot = 0; for (int i = 1; i < 12; ++i) tot += acc[i];
            fprintf(stderr, "HMCMT_STAMPS persist: %ld workgroups, third iteration of the last solve, mean us: pre-smooth %.2f fwd-transform %.2f wait-T1 %.2f slabs %.2f wait-T2 %.2f back-transform %.2f "
                            "post-smooth %.2f wait-R1 %.2f scalars+p+q %.2f wait-R2 %.2f update %.2f | iteration %.2f\n", n, acc[1] * us, acc[2] * us, acc[3] * us, acc[4] * us, acc[5] * us, acc[6] * us,
                    acc[7] * us, acc[8] * us, acc[9] * us, acc[10] * us, acc[11] * us, tot * us);
            if (nsl) fprintf(stderr, "   slabs, the %ld workgroups that have one: load %.2f, the two sweeps %.2f, store %.2f us\n", nsl, sl[0] * us * n / nsl, sl[1] * us * n / nsl, sl[2] * us * n / nsl);
            if (nbt) fprintf(stderr, "   back transform: operand planes -> LDS (+ the epilogue operands' loads) %.2f, MFMA loop %.2f, epilogue %.2f us\n", bt[0] * us * n / nbt, bt[1] * us * n / nbt, bt[2] * us * n / nbt);
        }
    }
    if (ctx->sv.stamps) {                                // HMCMT_STAMPS: phase stamps of the last launch that wrote them
        std::vector<long long> st(8 * 4096);
        hipMemcpy(st.data(), ctx->sv.stamps, st.size() * sizeof(long long), hipMemcpyDeviceToHost);
        double acc[8] = {0}; long n = 0; long long t0min = 0x7fffffffffffffffLL, tend = 0;
        for (int b = 0; b < 4096; ++b) {
            const long long* p = &st[8 * b];
            if (!p[0] || !p[6]) continue;
            ++n;
            for (int i = 1; i < 7; ++i) acc[i] += (double)(p[i] - p[i - 1]);
            t0min = std::min(t0min, p[0]); tend = std::max(tend, p[6]);
        }
        if (n) {
            fprintf(stderr, "HMCMT_STAMPS kernel %d: %ld workgroups; mean ticks per phase:", ctx->sv.stampKernel, n);
            for (int i = 1; i < 7; ++i) fprintf(stderr, " %.0f", acc[i] / n);
            fprintf(stderr, " | first entry -> last exit %lld ticks\n", tend - t0min);
        }
        hipFree(ctx->sv.stamps);
    }
    chain_release(ctx);
    map_release(ctx);
    for (void* p : ctx->allocs) hipFree(p);
    for (void* p : ctx->blk.allocs) hipFree(p);
    for (void* p : ctx->blk.hostAllocs) hipHostFree(p);
    for (hipEvent_t e : ctx->evPool) hipEventDestroy(e);
    if (ctx->h_nactive) hipHostFree(ctx->h_nactive);
    if (ctx->h_stall) hipHostFree(ctx->h_stall);
    if (ctx->h_prog) hipHostFree(ctx->h_prog);

    if (ctx->inst.h_rec) hipHostFree(ctx->inst.h_rec);
    if (ctx->h_stage) hipHostFree(ctx->h_stage);
    if (ctx->jac.h_rows) hipHostFree(ctx->jac.h_rows);
    if (ctx->h_lfFlag) hipHostFree(ctx->h_lfFlag);
    if (ctx->h_psOrder) hipHostFree(ctx->h_psOrder);
    if (ctx->evModel) hipEventDestroy(ctx->evModel);
    if (ctx->evSens) hipEventDestroy(ctx->evSens);
    if (ctx->evExtF) hipEventDestroy(ctx->evExtF);
    if (ctx->evPiv) hipEventDestroy(ctx->evPiv);
    if (ctx->evRec) hipEventDestroy(ctx->evRec);
    if (ctx->evExtA) hipEventDestroy(ctx->evExtA);
    if (ctx->side) hipStreamDestroy(ctx->side);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return 0;
}

// Shape of the persistent solve kernel for this problem (kernels_persist.h): a system = GZ row blocks of 14 rows x CS column
// parts = G workgroups, all on one XCD (32 CUs), one workgroup per CU; 2 * CW threads for tiles up to CW columns wide.
// CS = 1 where the whole row fits one tile (its LDS); CS = 2 (two column parts per row block) on wider meshes -- the stress size.
// does the mesh fit the kernel (its LDS, a system's workgroups on one XCD)?  twist: the factorisation the solves will use
struct ShapeDims { int NYP, NZP, nz; };
// (pure arithmetic on the mesh sizes: also behind hmcmt_persist_envelope, which needs no device)
static bool persist_shape_dims(const ShapeDims& k, int twist, int cs, int cuPerXcd, int& G, int& cw, int& mw, size_t& lds) {
    const int GZ = (k.nz - 1 + PS_OWN - 1) / PS_OWN;
    G = GZ * cs;
    const int TW = ps_tile_width(k.NYP, cs);
    if (!twist || TW > 256 || G > cuPerXcd || G > MAXNB) return false;       // (the slab solves are those of the twisted factorisation)
    // threads: 2 x the tile's columns -- more where a tall mesh needs the lanes for its tridiagonal sweeps (every lane takes a
    // chunk of PS_RCMAX rows of one mode and half); modes per slab: 32, or 16 (twice the chunks per half)
    for (cw = TW <= 64 ? 64 : (TW <= 128 ? 128 : 256); cw <= 256; cw *= 2) {
        if (cs > 1) {
            // the MFMA work split of the kernel: at most 4 mode tiles (forward) and 2 tile columns (back) per wave, at most 8 K-groups
            // of own columns, at most 16 in all
            const int NWV = cw / 32, C0 = ps_split_col(k.NYP), NTc = k.NYP / 16, KG = (k.NYP + 31) / 32;
            const int ntb0 = (C0 + PS_HC + 15) / 16, ntb1 = NTc - (C0 - PS_HC) / 16;
            if (k.NYP < 64 || (k.NYP & 15) || NTc > 4 * NWV || std::max(ntb0, ntb1) > 2 * NWV || ps_plane_width(k.NYP) > 256 || KG > 16 || k.NYP > 2 * cw) continue;
            if ((size_t)16 * 4 * ps_plane_width(k.NYP) * 2 > ps_tile_bytes(TW) - (size_t)4 * TW * 8) return false;      // (the forward operand planes live in the first tile)
        }
        for (mw = cs > 1 ? 16 : 32; mw >= 16; mw /= 2) {
            if (!ps_slab_fits(k.nz, mw, 2 * cw)) continue;
            lds = ps_lds_bytes(TW, k.NYP, k.NZP, k.nz, mw, 2 * cw);
            if (lds <= (size_t)160 * 1024) return true;
        }
    }
    return false;
}
static bool persist_shape(const Config& c, const ShapeDims& dims, int twist, int& cuPerXcd, int& G, int& cw, int& mw, size_t& lds, int* csOut = nullptr) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) { (void)hipGetLastError(); return false; }
    cuPerXcd = prop.multiProcessorCount / 8 / std::max(c.shareCnt, 1);        // (this context's share of an XCD's CUs)
    if (cuPerXcd < 1) return false;
    // HMCMT_PERSIST_CS = 1 | 2 forces the column parts (tests: the two-part kernel on meshes one tile would hold)
    for (int cs = 1; cs <= 2; ++cs) {
        if (c.persistCsForce && cs != c.persistCsForce) continue;
        if (persist_shape_dims(dims, twist, cs, cuPerXcd, G, cw, mw, lds)) { if (csOut) *csOut = cs; return true; }
    }
    return false;
}
// the persistent kernel's part of make_config: does it apply to this problem, and in which shape (persistCW = 0: it does not)
static int persist_config(const HostProblem& h, Config& c, std::string& err) {
    int cuPerXcd = 0, G = 0, cw = 0, mw = 32, cs = 1;
    size_t lds = 0;
    if (!persist_shape(c, ShapeDims{h.NYP, h.NZP, h.nz}, c.twist, cuPerXcd, G, cw, mw, lds, &cs)) return 0;
    if ((size_t)h.S * (size_t)h.NZP * (size_t)h.NYP >= ((size_t)1 << 27)) return 0;      // (the kernel's 32-bit lane offsets carry the system's element offset: kernels_persist.h, so32)
    for (const PsKernel& e : g_psKernels)
        if (e.strips == 2 && hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) { (void)hipGetLastError(); return 0; }
    c.persistMW = mw;
    c.persistG = G;
    c.persistCS = cs;
    c.persistGZ = G / cs;
    // the width-specialised instantiations where the table has one for the mesh's padded row width (ps_pick); HMCMT_PERSIST_WIDTHK=0
    // keeps the generic kernels (A/B runs, tests)
    const int wk = c.persistWidthK ? h.NYP : 0;
    c.persistSlots = std::max(1, std::min((h.S + 7) / 8, cuPerXcd / G));
    c.persistFillsShare = c.persistSlots * G >= cuPerXcd;       // (no CU of this context's share left over beside a solve: launch_adjoint_side)
    c.persistLds = lds;
    // the four-strip kernel where it applies: one column part, 32-mode slabs, a column tile of the transforms per wave, the slab
    // sweeps' chunks of four rows covering half the rows; HMCMT_PERSIST_STRIPS=2 keeps the two-half kernel (A/B)
    // (round 6: the four-strip kernel is opt-in -- it measured 530 against 600 steps/s at the headline size)
    int strips = 2;
    const size_t lds4 = ps4_lds_bytes(h.NYP, h.NZP, h.nz, 32, 4 * cw);
    if (c.persistStrips == 4 && cs == 1 && mw == 32 && 4 * cw <= 1024 && h.NYP / 16 <= 4 * cw / 64 && ps4_slab_rc(h.nz, 32, 4 * cw) == 4 && lds4 <= (size_t)160 * 1024) {
        bool ok4 = true;
        for (const PsKernel& e4 : g_psKernels)
            if (e4.strips == 4 && hipFuncSetAttribute(e4.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) { (void)hipGetLastError(); ok4 = false; }
        if (ok4) { strips = 4; c.persistLds = lds4; }
    }
    for (int sw = 1; sw <= 2; ++sw)
        if (!(c.psKern[sw - 1] = ps_pick(strips, cw, mw, cs, wk, c.stamps == STAMPS_PERSIST, sw))) {
            err = "no instantiation of the persistent solve kernel for this shape (g_psKernels)"; return HMCMT_EINVAL;
        }
    c.persistCW = cw;
    return 0;
}
// the persistent kernel's words, records and tables (Config::persistCW > 0)
static int persist_alloc(hmcmt_ctx* ctx) {
    const Solver& k = ctx->sv;
    const Config& c = ctx->cfg;
    if (!c.persistCW) return 0;
    int rc = 0;
    ctx->inst.persistSlots = c.persistSlots;
    ctx->inst.psyncBytes = ((size_t)(32 * 8 * c.persistSlots + 16) * sizeof(unsigned) + 15) & ~(size_t)15;
    if ((rc = dalloc(ctx, &ctx->inst.d_psync, ctx->inst.psyncBytes / sizeof(unsigned)))) return rc;
    if ((rc = dalloc(ctx, &ctx->d_gate, 2))) return rc;
    static_assert(sizeof(u4v) == 16, "a record of the kernel's reductions");
    if ((rc = dalloc(ctx, &ctx->inst.d_prec, (size_t)k.S * MAXNB * 2 * 8))) return rc;
    if ((rc = dalloc(ctx, &ctx->inst.d_psConst, 1, false))) return rc;      // (never cleared: launch_persist writes it whole)
    ctx->inst.psConstValid = false;
    if (k.S > 8 * c.persistSlots) {          // (more than one round of systems: persist_balance)
        if ((rc = dalloc(ctx, &ctx->d_psOrder, 2 * (size_t)k.S, false))) return rc;
        HIPCHK(hipHostMalloc((void**)&ctx->h_psOrder, 2 * sizeof(int) * (size_t)k.S, hipHostMallocDefault));
    }
    if (c.persistCS > 1 && (rc = dalloc(ctx, &ctx->inst.d_yhat2, (size_t)k.S * k.vstride))) return rc;
    if (c.stamps == STAMPS_PERSIST && (rc = dalloc(ctx, &ctx->d_pstamps, 16 * 256))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// What creation decides: the knobs resolved against the mesh and the device.  The device is checked and made current here (the
// kernels' LDS limits are raised on it); the context and its buffers come afterwards (create_impl, persist_alloc).
static int make_config(const HostProblem& h, const hmcmt_options& opt, const Knobs& kn, int32_t device_id, int shareIdx, int shareCnt, Config& c, std::string& err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { err = "no HIP device available (this library has no host compute path)"; return HMCMT_ENODEV; }
    if (device_id < 0 || device_id >= ndev) { err = "device_id out of range"; return HMCMT_ENODEV; }
    if (h.NZP > MAXNZP) { err = "nz too large for the tridiagonal kernel (nz+1 > 1024)"; return HMCMT_EINVAL; }
    // the fp64 eigen-transform kernel (fdm_precision = 1, and the restart of a stagnating mixed-precision solve) holds at most
    // 28 column tiles of 16 nodes.  A wider mesh runs the default mixed-precision path (the reference takes any mesh,
    // readEMModel2D.jl:11-154); it is refused here only where fp64 is ASKED for, and a restart that needs the kernel fails that
    // evaluation with HMCMT_ENOCONV (solve()) -- the safety net is what such a mesh goes without, not the solver.
    if (h.NYP / 16 > 28 && opt.fdm_precision == 1) { err = "fdm_precision = 1 on a mesh wider than 447 cells: the fp64 eigen-transform holds ny + 1 <= 448 nodes (include/hmcmt.h, hmcmt_create)"; return HMCMT_EINVAL; }
    if (const hipError_t e = hipSetDevice(device_id)) { err = std::string("hipSetDevice(device_id): ") + hipGetErrorString(e); return e == hipErrorOutOfMemory ? HMCMT_ENOMEM : HMCMT_EHIP; }
    static_cast<Knobs&>(c) = kn;
    c.device = device_id;
    c.shareIdx = shareIdx; c.shareCnt = shareCnt;
    c.shareMask = quarter_mask(shareIdx, shareCnt);      // (hmcmt_next_cu_share, taken over by hmcmt_create)
    auto raise_lds = [](const void* f, int bytes) { if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) return true; (void)hipGetLastError(); return false; };
#define KFN(...) reinterpret_cast<const void*>(__VA_ARGS__)
    // (this kernel also has a few hundred bytes of static LDS: ask for less than the full 160 KB)
    if (raise_lds(KFN(k_back_post<1, 1>), 152 * 1024)) c.maxLdsBack = 152 * 1024;
    {
        // boundary columns per workgroup of k_bc_fused: all workgroups resident at once (two per CU: registers), else the
        // two-kernel form (HMCMT_BC_FUSED = 0: never, n: n columns per workgroup)
        const int cols = h.ny + 1, nz = h.nz;
        const int cw = kn.bcFusedGiven ? kn.bcFused : std::max(1, (cols * h.nFreq + 511) / 512);
        const int slots = cols <= cw ? 2 : 1;
        const size_t lds = ((size_t)5 * nz * cw + (size_t)slots * 2 * nz) * sizeof(cplx);
        if (cw > 0 && cw <= 256 && lds <= (size_t)80 * 1024 && raise_lds(KFN(k_bc_fused), 80 * 1024)) {
            c.bcCW = cw; c.bcSlots = slots; c.bcLds = lds;
        }
        // otherwise the layer-blocked form (HMCMT_BC_BLOCKED = 0: the two-kernel form; "columns[,threads[,up layers[,down layers]]]"
        // per workgroup and block)
        // default: 1 024 threads (15 producer waves beside the chain wave: the transcendental work needs the occupancy), columns
        // such that the workgroups of a frequency divide its columns evenly and fill the chip at the stress size (401 columns, 32
        // frequencies: 8 x 51 -> 256 workgroups, one per CU), as many layers per bottom -> top block as the producers have threads
        int nt = 1024, cb = 64, lbu = 0, lbd = 8;
        { const int g = (cols + 63) / 64; int per = 256 / std::max(1, h.nFreq); per = std::max(g, std::min(per, (cols + 15) / 16)); cb = (cols + per - 1) / per; }
        int* const field[4] = {&cb, &nt, &lbu, &lbd};
        for (int i = 0; i < kn.bcBlockedN; ++i) *field[i] = kn.bcBlocked[i];
        const bool blockedOff = cb <= 0;
        cb = std::max(1, std::min(cb, 64)); nt = std::max(128, std::min(1024, nt / 64 * 64));
        if (lbu <= 0) lbu = (nt - 64) / cb;
        lbu = std::max(1, std::min(std::min(lbu, nz), (nt - 64) / cb));
        lbd = std::max(1, std::min(std::min(lbd, nz), (nt - 64) / cb));
        const int bslots = cols <= cb ? 2 : 1;
        const size_t blds = ((size_t)2 * std::max(3 * lbu, 5 * lbd) * cb + (size_t)bslots * 2 * nz) * sizeof(cplx);
        if (c.bcCW == 0 && !blockedOff && blds <= (size_t)150 * 1024 && raise_lds(KFN(k_bc_blocked), 150 * 1024)) {
            c.bcbCW = cb; c.bcbSlots = bslots; c.bcbLds = blds; c.bcbNT = nt; c.bcbLBu = lbu; c.bcbLBd = lbd;
        }
    }
    {
        const size_t sl = (size_t)12 * (h.nz + 1) * sizeof(cplx) + (size_t)h.nz * sizeof(double);
        c.sensFusedAlways = kn.sensFusedMode == 1;
        if (kn.sensFusedMode != 0 && sl <= (size_t)150 * 1024 && raise_lds(KFN(k_sens_fused), 150 * 1024)) c.sensFusedLds = sl;
    }
    if (raise_lds(KFN(k_fdm_fwd<FW_NTW>), 160 * 1024) && raise_lds(KFN(k_fdm_fwd<1>), 160 * 1024)) c.maxLds = 160 * 1024;
    // (the separate transform kernel stages LP_NRG row groups: beyond 64 KB on wide meshes with LP_NRG > 2); the stencil kernels'
    // tiles can pass 64 KB on wide meshes
    for (const void* f : {KFN(k_transform_lp<0, 0>), KFN(k_transform_lp<0, 1>), KFN(k_transform_lp<1, 0>), KFN(k_transform_lp<1, 1>),
                          KFN(k_transform_lp<2, 0>), KFN(k_transform_lp<2, 1>),
                          KFN(k_update_fused<1, 256, 6>), KFN(k_update_fused<1, 512, 6>), KFN(k_update_fused<2, 256, 6>), KFN(k_update_fused<2, 512, 4>),
                          KFN(k_update_fused<2, 512, 6>), KFN(k_update_fused<2, 512, 8>), KFN(k_update_fused<2, 1024, 4>),
                          KFN(k_post2), KFN(k_back_post<1, 2>),
                          KFN(k_spmv_fused<1, 256>), KFN(k_spmv_fused<1, 512>), KFN(k_spmv_fused<1, 1024>),
                          KFN(k_spmv_fused<2, 256>), KFN(k_spmv_fused<2, 512>), KFN(k_spmv_fused<2, 1024>),
                          KFN(k_resid_pre<256>), KFN(k_resid_pre<512>), KFN(k_resid_pre<1024>)})
        raise_lds(f, 152 * 1024);
#undef KFN
    // rows per tile of the stencil kernels: about 512 workgroups per launch, at most 8 rows (measured at cfg3:
    // 4 rows 484, 6 rows 489, 8 rows 492, 12 rows 456 steps/s), at least what MAXNB partial sums per system allow
    {
        // ... and few enough that two workgroups of k_update_fused fit a CU's LDS ((2 RT + 2) rows of NYP complex128)
        const int ldsRows = std::max(1, (int)((80 * 1024 / ((size_t)h.NYP * sizeof(cplx)) - 2) / 2));
        const int want = std::min(std::min(8, ldsRows), std::max(2, (int)(((long)(h.nz - 1) * h.S + 511) / 512)));
        c.RT = std::max(kn.rtGiven ? kn.rt : want, (h.nz - 1 + MAXNB - 1) / MAXNB);
    }
    c.RTS = c.RT;      // rows per tile of k_spmv_fused<2> (HMCMT_RTS; headline mesh, steps/s: 7 rows 328, 10 rows 311, 14 rows 325 -- it stays on the short tiles)
    c.RT2 = c.RT;      // rows per tile of k_update_fused<2> (>= RT: its partial sums fill the first slots of the k.NTR the consumers read); set with the launch shapes below
    // launch shapes of the two stencil kernels (launch_update2, launch_spmv).  Measured at the headline size, bench.py, steps/s
    // (round 3, profiles/r03_launch_shapes.md): k_spmv_fused 256 / 512 / 1024 threads 290 / 294 / 275; k_update_fused<2>
    // threads,batch,rows 256,6,7 (round 2) 294 | 512,8,14 304 | 512,6,14 301 | 512,4,14 297 | 1024,4,14 305 | 512,8,18 298 |
    // 512,8,21 279 | 512,8,12 281 | 256,6,14 277: twice the rows with twice the threads -- the same work per thread, 4 halo
    // rows per 14 instead of per 7.
    // ... all of which is for tiles with enough nodes per thread: on the reference's dprism3d example (96x49 cells, 22
    // systems, tiles of 3 rows x 112 nodes) the wide shapes lose 7 % (392 vs 419 evaluations/s, scripts/gpu_example_ab.sh),
    // so small tiles keep the round-2 shapes.
    const int tileNodes = (c.RT + 2) * h.NYP, tile2Nodes = (2 * c.RT + 4) * h.NYP;
    c.spmvThreads = c.upd1Threads = tileNodes >= 1280 ? 512 : 256;     // (cfg3 1872, cfg5 2912 | dprism3d 560, cfg2 256)
    c.residThreads = tileNodes >= 1280 ? 512 : 256;        // (k_resid_pre at the headline size: 16.9 / 13.8 / 18.6 us with 256 / 512 / 1024)
    if (kn.resid) c.residThreads = kn.resid;
    c.upd2Threads = 256; c.upd2Batch = 6;
    if (tile2Nodes >= 2560 && h.NYP <= 256 &&                               // (cfg3 3744 | dprism3d 1120; cfg5: 52.7 vs 51.8 steps/s with the taller tiles)
        (size_t)(3 * 2 * c.RT + 8) * h.NYP * sizeof(float2) <= (size_t)150 * 1024) { c.upd2Threads = 512; c.upd2Batch = 8; c.RT2 = 2 * c.RT; }
    if (kn.rt2Given) c.RT2 = std::max(c.RT, kn.rt2);
    if (kn.rtsGiven) c.RTS = std::max(c.RT, std::min(kn.rts, 64));
    {   // HMCMT_UPD2 = "threads,batch,rows"
        const int a = kn.upd2[0], b = kn.upd2[1], r = kn.upd2[2];
        if (kn.upd2N >= 1 && (a == 256 || a == 512 || a == 1024)) c.upd2Threads = a;
        if (kn.upd2N >= 2 && b > 0) c.upd2Batch = b;
        if (kn.upd2N >= 3 && r >= c.RT) c.RT2 = r;
    }
    if (kn.upd1) c.upd1Threads = kn.upd1;
    if (kn.spmv) c.spmvThreads = kn.spmv;
    // forward half of the FDM stage: the fused kernel where its LDS slabs fit (fdm_fwd_ntw); the operand format goes with the path
    Solver dims{};
    dims.NYP = h.NYP; dims.NZP = h.NZP; dims.nz = h.nz;
    c.fwdNtwFused = fdm_fwd_ntw(dims, true, kn.fusedFwdMode == 2, kn.twistOn, c.maxLds);
    c.fwdNtw = kn.fusedFwdMode ? c.fwdNtwFused : 0;
    c.splitT = c.fwdNtw > 0;
    c.fusedBackFits = c.splitT && back_post_lds(h.NYP) <= c.maxLdsBack && h.NYP <= 256;
    // x += alpha p rides along in k_fdm_fwd where the update kernel's burst is long enough to notice (headline size: +2.4 .. 3.5 %;
    // on dprism3d's 6 160 interior nodes per system it costs 1 %); HMCMT_XFWD=0 / 1 forces it off / on
    c.xInFwd = c.splitT && (kn.xfwd < 0 ? (long)(h.nz - 1) * h.NYP >= 12000 : kn.xfwd != 0);
    {   // the x update is done by the fused kernel's waves 1.. and its per-slab sums fill MAXNB slots: not with one wave, not with more slabs
        const int Gq = (h.NZP + 7) / 8, per = (Gq + 7) / 8, nw = (Gq + per - 1) / per, nslab = ((h.NYP >> 4) + FW_NTW - 1) / FW_NTW;
        if (nw < 2 || nslab > MAXNB) c.xInFwd = 0;
    }
    {   // the twisted factorisation goes with the kernels that sweep both ways at once: the fused forward kernel of the launch-per-phase
        // path, and the persistent kernel (which does not need the fused one to fit: tall meshes)
        int a1, a2, a3, a4; size_t a5;
        const bool pshape = persist_shape(c, ShapeDims{h.NYP, h.NZP, h.nz}, kn.twistOn ? 1 : 0, a1, a2, a3, a4, a5);
        c.twist = (c.splitT || pshape) && kn.twistOn;
    }
    return persist_config(h, c, err);
}

// the context's streams, events and buffers, for the problem and the configuration it was constructed with (the device is current)
static int create_impl(hmcmt_ctx* ctx) {
    const int device_id = ctx->cfg.device;
    ctx->ss.persistOn = ctx->cfg.persist; ctx->ss.guardEvery = ctx->cfg.guardEvery; ctx->ss.dbgFlags = ctx->cfg.debugFlags;      // (their initial values: they change at run time)
    if (ctx->cfg.shareCnt > 1) {
        // a share of EVERY XCD's CUs: mask bit n is CU n / nXCD of XCD n % nXCD (measured, scripts/probe/cumask.hip: a mask that
        // leaves an XCD without a bit leaves that XCD unrestricted), so share i of c takes the CU indices [i, i + 1) * cuPerXcd / c
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device_id));
        const int nxcd = 8, ncu = prop.multiProcessorCount, per = ncu / nxcd;
        std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
        for (int n = 0; n < ncu; ++n) {
            const int cu = n / nxcd;
            if (cu * ctx->cfg.shareCnt / per == ctx->cfg.shareIdx) mask[n / 32] |= 1u << (n % 32);
        }
        HIPCHK(hipExtStreamCreateWithCUMask(&ctx->stream, (uint32_t)mask.size(), mask.data()));
        HIPCHK(hipExtStreamCreateWithCUMask(&ctx->side, (uint32_t)mask.size(), mask.data()));
    } else {
        // The main stream at the HIGHEST priority: streams of one priority are multiplexed onto GPU_MAX_HW_QUEUES (4) hardware queues in the
        // order of their creation, and a host that has created streams before this context -- an initialised RCCL process group, torch --
        // left the main and the side stream on ONE queue: the side stream's 0.33 ms of sensitivity tables per step then ran IN FRONT OF the
        // solves instead of beside them (round 6: bench.py under a process group 519-531 steps/s against 606-625 without; with
        // GPU_MAX_HW_QUEUES=8 626).  Another priority is another set of queues.  HMCMT_STREAM_PRIORITY=0: both streams at the default one.
        int prLeast = 0, prGreatest = 0;
        const bool hiPr = ctx->cfg.streamPriority && hipDeviceGetStreamPriorityRange(&prLeast, &prGreatest) == hipSuccess && prGreatest != prLeast;
        if (hiPr) HIPCHK(hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prGreatest));
        else { (void)hipGetLastError(); HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); }
        HIPCHK(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    }
    // events between the library's own streams: no system-scope fence at the record (HMCMT_EVENT_FLAGS: 0 the default
    // system-scope release, 1 hipEventDisableSystemFence, 2 hipEventReleaseToDevice); evRec is waited for by the host
    const int evMode = ctx->cfg.eventFlags;
    const unsigned evDev = hipEventDisableTiming | (evMode == 1 ? hipEventDisableSystemFence : evMode == 2 ? hipEventReleaseToDevice : 0u);
    HIPCHK(hipEventCreateWithFlags(&ctx->evModel, evDev));
    HIPCHK(hipEventCreateWithFlags(&ctx->evSens, evDev));
    HIPCHK(hipEventCreateWithFlags(&ctx->evExtF, evDev));
    HIPCHK(hipEventCreateWithFlags(&ctx->evPiv, evDev));
    HIPCHK(hipEventCreateWithFlags(&ctx->evRec, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->evExtA, evDev));
    const HostProblem& h = ctx->hp;
    View& v = ctx->v;
    v.ny = h.ny; v.nz = h.nz; v.NYP = h.NYP; v.NZP = h.NZP; v.nFreq = h.nFreq; v.S = h.S; v.nRx = h.nFun; v.nTip = h.nTip;
    v.nData = h.nData; v.nAC = h.nAC; v.nCell = h.nCell; v.zid = h.zid; v.vstride = (long)h.NZP * h.NYP;
    v.dbg = 0; v.ticks = nullptr;
    // (the lateral mean of the FDM background is the geometric mean of sigma for both modes.  Round 3's experiment HMCMT_BGMEAN --
    // the arithmetic mean of the coefficient the operator is linear in -- was removed in round 4: +2 % at the bench, but at the true
    // model the gain was an earlier stop at a 5x looser error, not faster convergence: DESIGN section 9.)
    const size_t VS = (size_t)v.vstride, S = (size_t)h.S;
    int rc;
#define UP(field, vec) { decltype(vec)::value_type* p_ = nullptr; if ((rc = dupload(ctx, &p_, vec))) return rc; v.field = p_; }
    UP(yLen, h.yLen) UP(zLen, h.zLen) UP(omega, h.omega) UP(lam, h.lam) UP(sysOn, h.sysOn)
    UP(cell2act, h.cell2act) UP(bg, h.bg) UP(act, h.act)
    UP(rxIdn, h.rxIdn) UP(rxDy1, h.rxDy1) UP(rxDy2, h.rxDy2) UP(rxKL, h.rxKL) UP(rxKR, h.rxKR) UP(rxWL, h.rxWL) UP(rxWR, h.rxWR)
    UP(predSys, h.predSys) UP(predRx, h.predRx) UP(datSys, h.datSys) UP(datRx, h.datRx) UP(predKind, h.predKind) UP(datKind, h.datKind)
    UP(obs, h.obs) UP(dataW, h.dataW) UP(srStart, h.srStart) UP(srList, h.srList)
    if (h.nTip) { UP(rxCL, h.rxCL) UP(rxCR, h.rxCR) UP(rxVL, h.rxVL) UP(rxVR, h.rxVR) }
#undef UP
    {
        // fragment-order copies of V and V' (see k_transform)
        const int NT = h.NYP / 16, KG = h.NYP / 16;
        auto swz = [&](const std::vector<double>& B) {
            std::vector<double> o((size_t)h.NYP * h.NYP);
            for (int kg = 0; kg < KG; ++kg)
                for (int t = 0; t < NT; ++t)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < 4; ++i)
                            o[(((size_t)kg * NT + t) * 64 + lane) * 4 + i] =
                                B[(size_t)(16 * kg + 4 * (lane / 16) + i) * h.NYP + 16 * t + lane % 16];
            return o;
        };
        if ((rc = dupload(ctx, &ctx->d_V, swz(h.Vpad)))) return rc;
        if ((rc = dupload(ctx, &ctx->d_Vt, swz(h.Vtpad)))) return rc;
        // bf16 fragment order of k_transform_lp (k consumed 32 at a time, zero beyond NYP)
        const int KG32 = (h.NYP + 31) / 32;
        auto bf = [](double x) -> unsigned short {
            float f = (float)x; unsigned u; std::memcpy(&u, &f, 4);
            return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        };
        auto bf2f = [](unsigned short hval) -> float { unsigned u = (unsigned)hval << 16; float f; std::memcpy(&f, &u, 4); return f; };
        auto swzb = [&](const std::vector<double>& B, bool lo) {
            std::vector<unsigned short> o((size_t)KG32 * NT * 64 * 8, 0);
            for (int kg = 0; kg < KG32; ++kg)
                for (int t = 0; t < NT; ++t)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < 8; ++i) {
                            const int k = 32 * kg + 8 * (lane / 16) + i;
                            if (k >= h.NYP) continue;
                            const double x = B[(size_t)k * h.NYP + 16 * t + lane % 16];
                            const unsigned short hi = bf(x);
                            o[(((size_t)kg * NT + t) * 64 + lane) * 8 + i] = lo ? bf(x - (double)bf2f(hi)) : hi;
                        }
            return o;
        };
        unsigned short* tmp = nullptr;
        if ((rc = dupload(ctx, &tmp, swzb(h.Vpad, false)))) return rc;
        ctx->d_Vb = reinterpret_cast<u4v*>(tmp);
        if ((rc = dupload(ctx, &tmp, swzb(h.Vpad, true)))) return rc;
        ctx->d_Vbl = reinterpret_cast<u4v*>(tmp);
        if ((rc = dupload(ctx, &tmp, swzb(h.Vtpad, false)))) return rc;
        ctx->d_Vtb = reinterpret_cast<u4v*>(tmp);
        if ((rc = dupload(ctx, &tmp, swzb(h.Vtpad, true)))) return rc;
        ctx->d_Vtbl = reinterpret_cast<u4v*>(tmp);
    }
#define DA(ptr, n) if ((rc = dalloc(ctx, &(ptr), (n)))) return rc;
    DA(v.sigma, h.nCell) DA(v.sigMeanA, h.nz) DA(v.sigMeanG, h.nz)
    DA(v.cY, 2 * VS) DA(v.cZ, 2 * VS) DA(v.dK, 2 * VS) DA(v.dM, 2 * VS)
    DA(v.mzq, 2 * h.NZP) DA(v.dgz, 2 * h.NZP) DA(v.ofz, 2 * h.NZP) DA(v.mzs, 2 * h.NZP)
    DA(v.invp, S * VS) DA(v.X, S * VS) DA(v.Lam, S * VS) DA(v.R, S * VS)
    DA(v.Zrx, S * h.nFun) DA(v.rxN0, S * h.nFun) DA(v.rxD, S * h.nFun * 11) DA(v.rxCoef, S * h.nFun)
    DA(v.pred, h.nData) DA(v.vbar, h.nData) DA(v.misfitPart, h.nData)
    DA(v.srcB, S * 4) DA(v.wL, S * h.nz) DA(v.wR, S * h.nz) DA(v.colw, S * h.ny)
    DA(v.gL, S * h.nz) DA(v.gR, S * h.nz) DA(v.gMn, S * h.nz) DA(v.dBC, S * 2 * (size_t)h.nz * h.nz) DA(v.bcsL, S * h.nz) DA(v.bcsR, S * h.nz) DA(v.bcsB, S)
    DA(v.fwdTab, S * FWD_NQ * (size_t)h.nz * (h.ny + 1)) DA(v.sensTab, S * 15 * (size_t)(h.nz + 1))
    DA(v.sensEu, S * 3 * (size_t)(h.nz + 1)) DA(v.sensEd, S * 3 * (size_t)(h.nz + 1)) DA(v.sensMix, S * 12 * (size_t)h.nz)
    DA(v.sensDz1, S * 3 * (size_t)h.nz) DA(v.sensZ1, S * 3) DA(v.sensDead, S * 3)
    DA(v.qPart, S * h.ny) DA(v.gPart, 2 * (size_t)h.nCell) DA(v.gPartG, 2 * GRAD_NG * (size_t)h.nCell) DA(v.grad, h.nAC)
    DA(ctx->d_m, h.nAC) DA(ctx->d_misfit, 1) DA(ctx->d_cnt, 1)
    for (int q : h.sysOn) ctx->ss.nSysOn += q;
    for (int kd = 0; kd < 2; ++kd) { DA(ctx->d_prevField[kd], (EXT_NP - 1) * S * VS) DA(ctx->d_mHist[kd], (EXT_NP + 1) * (size_t)h.nAC) DA(ctx->d_ext[kd], EXT_LEN) }
    Solver& k = ctx->sv;
    k.S = h.S; k.NYP = h.NYP; k.NZP = h.NZP; k.ny = h.ny; k.nz = h.nz; k.nFreq = h.nFreq; k.vstride = v.vstride;
    k.NB = std::max(1, std::min(32, (1024 + h.S - 1) / h.S));
    k.chunk = (v.vstride + k.NB - 1) / k.NB;
    // the launch shapes and paths make_config chose, where the kernels take them by value
    k.RT = ctx->cfg.RT; k.RT2 = ctx->cfg.RT2; k.RTS = ctx->cfg.RTS;
    k.NTR = (h.nz - 1 + k.RT - 1) / k.RT;
    k.sweeps = 1;
    k.splitT = ctx->cfg.splitT; k.xInFwd = ctx->cfg.xInFwd; k.twist = v.twist = ctx->cfg.twist;
    k.stamps = nullptr; k.stampKernel = 0;
    k.ticks = nullptr; k.xTickF = v.X;
    if (ctx->cfg.wantTicks && hipMalloc(&ctx->v.ticks, (32 + 64 * TK_N) * sizeof(long long)) == hipSuccess) {
        hipMemset(ctx->v.ticks, 0, (32 + 64 * TK_N) * sizeof(long long));
        k.ticks = ctx->v.ticks;
    }
    if (ctx->cfg.stamps == STAMPS_UPD || ctx->cfg.stamps == STAMPS_SPMV) {
        k.stampKernel = ctx->cfg.stamps;
        HIPCHK(hipMalloc((void**)&k.stamps, sizeof(long long) * 8 * 4096)); HIPCHK(hipMemset(k.stamps, 0, sizeof(long long) * 8 * 4096));
    }
    k.w2 = ctx->cfg.w2;
    k.merged2 = 1;
    k.omega = v.omega; k.cY = v.cY; k.cZ = v.cZ; k.dK = v.dK; k.dM = v.dM; k.ofz = v.ofz; k.invp = v.invp;
    { float4* cf = nullptr; if ((rc = dalloc(ctx, &cf, 2 * 2 * VS))) return rc; k.cf32 = cf; }
    k.r = v.R;
    DA(k.p, S * VS) DA(k.q, S * VS) DA(k.z, S * VS) DA(k.y, S * VS) DA(k.t, S * VS) DA(k.dinv, S * VS)
    DA(k.t32, S * VS + 64) DA(k.y32, S * VS + 64) DA(ctx->inst.d_invp32, S * VS)
    DA(k.z32, S * VS) DA(k.p32a, S * VS) DA(k.p32b, S * VS) DA(k.zs32, S * VS) DA(k.z4_32, S * VS) DA(k.t2_32, S * VS) DA(k.partR, S * MAXNB) DA(k.dinv32, S * VS)
    DA(k.p2, S * VS) DA(k.r2, S * VS) DA(k.partPQ, S * MAXNB) DA(k.rho2, 2 * S)
    k.invp32 = ctx->inst.d_invp32;
    DA(k.partA, S * MAXNB) DA(k.partB, S * MAXNB) DA(ctx->inst.d_partZZ, S * MAXNB)
    DA(ctx->inst.d_partRes, S * MAXNB) DA(ctx->inst.d_partBn, S * MAXNB)
    DA(k.rho, S) DA(k.alphaBeta, S) DA(k.active, S) DA(k.iters, S) DA(k.status, S) DA(k.nactive, 1) DA(k.errEst, S) DA(k.errRef, S) DA(k.errRefIt, S)
    DA(ctx->inst.d_b, S * VS)
    DA(ctx->d_fieldsOut, (size_t)h.nFreq * (h.ny + 1) * (h.nz + 1))
#undef DA
    HIPCHK(hipHostMalloc((void**)&ctx->h_nactive, sizeof(int), hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void**)&k.nactHost, ctx->h_nactive, 0));
    HIPCHK(hipHostMalloc((void**)&ctx->h_stall, HW_WORDS * sizeof(int), hipHostMallocMapped));     // the HostWord block: stagnation, failure status, placement failed, wait timed out
    for (int w = 0; w < HW_WORDS; ++w) ctx->h_stall[w] = 0;
    HIPCHK(hipHostGetDevicePointer((void**)&k.stallHost, ctx->h_stall, 0));
    k.failHost = k.stallHost + HW_FAIL;
    k.stallIt = ctx->cfg.stallIt;       // (HMCMT_STALL_IT: tests force the fp64 restart with a short window)
    HIPCHK(hipHostMalloc((void**)&ctx->h_prog, sizeof(int), hipHostMallocMapped));
    *ctx->h_prog = 0;
    HIPCHK(hipHostGetDevicePointer((void**)&k.progHost, ctx->h_prog, 0));
    HIPCHK(hipHostMalloc((void**)&ctx->inst.h_rec, sizeof(double) * 4 * h.S, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void**)&ctx->inst.d_recHost, ctx->inst.h_rec, 0));
    ctx->stageDoubles = (size_t)h.nAC * 4 + (size_t)h.nData * 2 + 16;
    HIPCHK(hipHostMalloc((void**)&ctx->h_stage, sizeof(double) * ctx->stageDoubles));
    ctx->ss.itersLast.assign(2 * h.S, 0);
    // constant halves of the stencils: TE stiffness (mesh only), TM mass (mesh only)
    const int nodes = v.NZP * (v.ny + 1);
    hipLaunchKernelGGL(k_coef, grid1(nodes, 256), dim3(256), 0, ctx->stream, v, 1, 0, 0, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

static const char* options_error(const hmcmt_options* o) {
    if (o->precond < HMCMT_PRECOND_JACOBI || o->precond > HMCMT_PRECOND_FDM_JACOBI) return "unknown preconditioner";
    if (o->fdm_precision != 0 && o->fdm_precision != 1) return "fdm_precision must be 0 (bf16/fp32) or 1 (fp64)";
    if (!(o->tol > 0) || o->maxit < 1) return "tol must be > 0 and maxit >= 1";
    if (o->warm_start < 0 || o->warm_start > 2) return "warm_start must be 0, 1 or 2";
    return nullptr;
}

int hmcmt_create(hmcmt_ctx** out, int32_t device_id, int64_t ny, int64_t nz, const double* yLen,
                 const double* zLen, const double* origin, int64_t nFreq, const double* freqs, int64_t nRx,
                 const double* rxY, const double* rxZ, int64_t nComp, const int64_t* compMode, int64_t nData,
                 const int64_t* freqID, const int64_t* rxID, const int64_t* dtID, const uint8_t* dataID,
                 const double* obs, const double* dataW, int64_t nAC, const int64_t* activeIdx,
                 const double* bgModel, const hmcmt_options* opts) {
    // (hmcmt_next_cu_share is consumed by THIS call, whatever becomes of it: a create that fails must not leave the share to the next one)
    const int shareIdx = g_nextShareIdx, shareCnt = g_nextShareCnt;
    g_nextShareIdx = 0; g_nextShareCnt = 1;
    if (!out) { g_createError = "null ctx pointer"; return HMCMT_EINVAL; }
    *out = nullptr;
    if (!yLen || !zLen || !origin || !freqs || !rxY || !rxZ || !compMode || !dataID || !activeIdx || !bgModel ||
        (nData > 0 && (!freqID || !rxID || !dtID || !obs || !dataW))) {
        g_createError = "null input array"; return HMCMT_EINVAL;
    }
    if (opts) if (const char* e = options_error(opts)) { g_createError = e; return HMCMT_EINVAL; }
    HostProblem hp;
    if (!hp.build(ny, nz, yLen, zLen, origin, nFreq, freqs, nRx, rxY, rxZ, nComp, compMode, nData, freqID,
                  rxID, dtID, dataID, obs, dataW, nAC, activeIdx, bgModel)) {
        g_createError = hp.error;
        return HMCMT_EINVAL;
    }
    hmcmt_options opt;
    hmcmt_default_options(&opt);
    if (opts) opt = *opts;
    // the configuration first -- knobs, then what they, the mesh and the device decide --, then the context around it: const from here on
    struct { const char* operator()(const char* name) const { return getenv(name); } } env;     // (the library's one look at the environment)
    Config cfg;
    int rc = make_config(hp, opt, read_knobs(env, KnobLimits{EXT_NP, STALL_IT, PS_SPIN_LIMIT}), device_id, shareIdx, shareCnt, cfg, g_createError);
    if (rc) return rc;
    hmcmt_ctx* ctx = new hmcmt_ctx(std::move(hp), opt, cfg);
    if ((rc = create_impl(ctx)) || (rc = persist_alloc(ctx))) { g_createError = ctx->err; hmcmt_destroy(ctx); return rc; }
    if (ctx->cfg.device >= 0 && ctx->cfg.device < MAXDEV) {
        for (int q = 0; q < 4; ++q) if ((ctx->cfg.shareMask >> q) & 1u) g_quarterUse[ctx->cfg.device][q].fetch_add(1);
    }
    devlock_ref(ctx->cfg);
    ctx->counted = true;
    *out = ctx;
    return 0;
}

int hmcmt_set_options(hmcmt_ctx* ctx, const hmcmt_options* o) {
    if (!ctx || !o) return HMCMT_EINVAL;
    if (const char* e = options_error(o)) { ctx->err = e; return HMCMT_EINVAL; }
    if (o->fdm_precision == 1 && ctx->hp.NYP / 16 > 28) { ctx->err = "fdm_precision = 1 on a mesh wider than 447 cells (the fp64 eigen-transform holds ny + 1 <= 448 nodes)"; return HMCMT_EINVAL; }
    ctx->opt = *o;
    ctx->ss.lastItFwd = ctx->ss.lastItAdj = 0;
    ctx->ss.haveFwd = ctx->ss.haveAdj = false;
    ctx->memo[0].valid = ctx->memo[1].valid = false;
    ctx->lfHaveGrad = false;            // (a gradient kept for start_grad = 1 / 2 was computed under the old options)
    ++ctx->stateGen;                    // (... and so was a chain's: hmcmt_chain_step evaluates its start gradient again)
    ctx->jvp.valid = false;
    return 0;
}

int hmcmt_get_stats(const hmcmt_ctx* ctx, hmcmt_stats* out) {
    if (!ctx || !out) return HMCMT_EINVAL;
    *out = ctx->stats;
    return 0;
}

int hmcmt_get_iters(const hmcmt_ctx* ctx, int32_t* iters) {
    if (!ctx || !iters) return HMCMT_EINVAL;
    for (size_t i = 0; i < ctx->ss.itersLast.size(); ++i) iters[i] = ctx->ss.itersLast[i];
    return 0;
}

int hmcmt_profile_counters(hmcmt_ctx* ctx, int64_t* out) {
    if (!ctx || !out) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    prof_collect(ctx);
    unsigned long long c = 0;
    HIPCHK(hipMemcpy(&c, ctx->d_cnt, sizeof c, hipMemcpyDeviceToHost));
    out[0] = (int64_t)c; out[1] = ctx->profStartSys; out[2] = ctx->profEvals; out[3] = ctx->profSolves; out[4] = ctx->profSolves2;
    out[5] = ctx->profSerialIts; out[6] = ctx->profPersistSolves;
    return 0;
}

int hmcmt_dims(const hmcmt_ctx* ctx, int32_t* o) {
    if (!ctx || !o) return HMCMT_EINVAL;
    o[0] = ctx->v.NYP; o[1] = ctx->v.NZP; o[2] = ctx->v.S; o[3] = ctx->v.ny; o[4] = ctx->v.nz; o[5] = ctx->v.zid; o[6] = ctx->sv.NB;
    return 0;
}

int hmcmt_grad_device(hmcmt_ctx* ctx, const double* d_m, double* d_pred, double* d_misfit, double* d_grad) {
    if (!ctx || !d_m || !d_grad) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    int rc = evaluate(ctx, d_m, true, d_pred, d_misfit, d_grad);
    if (rc) return rc;
    if ((rc = collect_stats(ctx, true))) return rc;      // includes the stream synchronisation
    prof_collect(ctx);
    return finish_status(ctx);
}

int hmcmt_grad_device_async(hmcmt_ctx* ctx, const double* d_m, double* d_pred, double* d_misfit, double* d_grad) {
    if (!ctx || !d_m || !d_grad) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    int rc = evaluate(ctx, d_m, true, d_pred, d_misfit, d_grad);
    if (rc) return rc;
    ctx->statsPending = true;
    ctx->pendingAdj = true;
    return 0;
}

static int leapfrog_flag(hmcmt_ctx* ctx);

int hmcmt_wait(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const int rc = collect_pending(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    const int rf = leapfrog_flag(ctx);
    return rc ? rc : rf;
}

int hmcmt_forward_device(hmcmt_ctx* ctx, const double* d_m, double* d_pred, double* d_misfit) {
    if (!ctx || !d_m) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    int rc = evaluate(ctx, d_m, false, d_pred, d_misfit, nullptr);
    if (rc) return rc;
    if ((rc = collect_stats(ctx, false))) return rc;
    prof_collect(ctx);
    return finish_status(ctx);
}

static hmcmt_ctx::Memo* memo_find(hmcmt_ctx* ctx, const double* m, bool needGrad) {
    const size_t bytes = sizeof(double) * ctx->v.nAC;
    for (auto& e : ctx->memo)
        if (e.valid && (!needGrad || e.hasGrad) && std::memcmp(e.m.data(), m, bytes) == 0) return &e;
    return nullptr;
}
static void memo_store(hmcmt_ctx* ctx, const double* m, const double* pred, double misfit, const double* grad) {
    const int nAC = ctx->v.nAC, nData = ctx->v.nData;
    hmcmt_ctx::Memo* e = memo_find(ctx, m, false);
    if (e && e->hasGrad && !grad) return;                 // keep the richer entry of the same model
    if (!e) { e = &ctx->memo[ctx->memoNext]; ctx->memoNext ^= 1; }
    e->m.assign(m, m + nAC);
    e->pred.assign(pred, pred + 2 * nData);
    e->misfit = misfit;
    e->hasGrad = grad != nullptr;
    if (grad) e->grad.assign(grad, grad + nAC);
    e->stats = ctx->stats;
    e->valid = true;
}

static int host_eval(hmcmt_ctx* ctx, const double* m, double* pred, double* misfit, double* grad, bool wantGrad) {
    if (!ctx || !m || (wantGrad && !grad)) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const int nAC = ctx->v.nAC, nData = ctx->v.nData;
    for (int i = 0; i < nAC; ++i)
        if (!std::isfinite(m[i])) { ctx->err = "non-finite model value"; return HMCMT_EBREAKDOWN; }
    if (!ctx->opt.verify)
        if (const hmcmt_ctx::Memo* e = memo_find(ctx, m, wantGrad)) {     // this very model was evaluated a moment ago
            if (pred) std::memcpy(pred, e->pred.data(), sizeof(cplx) * nData);
            if (misfit) *misfit = e->misfit;
            if (wantGrad) std::memcpy(grad, e->grad.data(), sizeof(double) * nAC);
            ctx->stats = e->stats;                                           // (this call itself iterated nothing)
            ctx->stats.iters_fwd_max = ctx->stats.iters_adj_max = ctx->stats.iters_fwd_sum = ctx->stats.iters_adj_sum = 0;
            ++ctx->memoHits;
            ctx->jvp.valid = false;                                          // (an evaluating call, answered or not, ends a linearisation point)
            return 0;
        }
    std::memcpy(ctx->h_stage, m, sizeof(double) * nAC);
    HIPCHK(hipMemcpyAsync(ctx->d_m, ctx->h_stage, sizeof(double) * nAC, hipMemcpyHostToDevice, ctx->stream));
    int rc = evaluate(ctx, ctx->d_m, wantGrad, nullptr, nullptr, nullptr);
    if (rc) return rc;
    double* hs = ctx->h_stage + nAC;
    HIPCHK(hipMemcpyAsync(hs, ctx->v.pred, sizeof(cplx) * nData, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(hs + 2 * nData, ctx->d_misfit, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (wantGrad) HIPCHK(hipMemcpyAsync(hs + 2 * nData + 1, ctx->v.grad, sizeof(double) * nAC, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = collect_stats(ctx, wantGrad))) return rc;   // includes the stream synchronisation
    prof_collect(ctx);
    if (pred) std::memcpy(pred, hs, sizeof(cplx) * nData);
    if (misfit) *misfit = hs[2 * nData];
    if (wantGrad) std::memcpy(grad, hs + 2 * nData + 1, sizeof(double) * nAC);
    rc = finish_status(ctx);
    if (rc == 0) memo_store(ctx, m, hs, hs[2 * nData], wantGrad ? hs + 2 * nData + 1 : nullptr);
    return rc;
}

int hmcmt_grad(hmcmt_ctx* ctx, const double* m, double* pred, double* misfit, double* grad) {
    return host_eval(ctx, m, pred, misfit, grad, true);
}
int hmcmt_forward(hmcmt_ctx* ctx, const double* m, double* pred, double* misfit) {
    return host_eval(ctx, m, pred, misfit, nullptr, false);
}

int hmcmt_get_fields(hmcmt_ctx* ctx, int32_t adjoint, double* exTE, double* hxTM) {
    if (!ctx) return HMCMT_EINVAL;
    if (!ctx->ss.haveModel) { ctx->err = "no evaluation has been run yet"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const View& v = ctx->v;
    const int nn = (v.ny + 1) * (v.nz + 1);
    const cplx* src = adjoint ? v.Lam : v.X;
    for (int mode = 0; mode < 2; ++mode) {
        double* dst = mode == 0 ? exTE : hxTM;
        if (!dst) continue;
        hipLaunchKernelGGL(k_unpad, dim3((nn + 255) / 256, v.nFreq), dim3(256), 0, ctx->stream, v, src, ctx->d_fieldsOut, mode * v.nFreq);
        HIPCHK(hipMemcpyAsync(dst, ctx->d_fieldsOut, sizeof(cplx) * (size_t)nn * v.nFreq, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int hmcmt_profile(hmcmt_ctx* ctx, int32_t enable) {
    if (!ctx) return HMCMT_EINVAL;
    ctx->ss.profMask = 0;
    ctx->evUsed = 0;
    ctx->profOverheadMs = ctx->profOverheadChainMs = 0.0;
    ctx->ivs.clear(); ctx->chainEnd = (size_t)-1;
    if (enable) {
        // An event pair around a launch also times what the command processor does between the two markers beside
        // running the kernel (the marker packets themselves, dispatch latency).  Calibrated on the device's own clock:
        // a one-workgroup kernel that spins for a KNOWN time (SPIN_US on the constant-rate wall clock) is bracketed the
        // same way, back to back, long enough that the queue never runs dry (the host needs ~5 us per launch + record);
        // the bracket overhead is the median period minus the duration rocprofv3 reports for that kernel (spin time +
        // SPIN_EDGE_US of dispatch / completion edges: 12.39 us for a 12.00 us spin, scripts/gpu_spin_calib.sh).  It comes
        // out at 2.57 us run after run.  (Rounds 1-2 calibrated with an EMPTY kernel, whose period is the HOST's launch
        // rate, times a fitted factor: the subtracted value followed the host's speed, 0.3 .. 3.8 us from run to run.
        // A 512-workgroup spin kernel is no better a yardstick: its workgroups start over 6 us.)
        HIPCHK(hipSetDevice(ctx->cfg.device));
        int wallKHz = 100000;
        if (hipDeviceGetAttribute(&wallKHz, hipDeviceAttributeWallClockRate, ctx->cfg.device) != hipSuccess || wallKHz <= 0) wallKHz = 100000;
        constexpr double SPIN_US = 12.0, SPIN_EDGE_US = 0.39;
        const long long ticks = (long long)(SPIN_US * 1e-3 * wallKHz);
        const int N = 48;
        std::vector<hipEvent_t> ev(2 * N);
        for (auto& e : ev) HIPCHK(hipEventCreate(&e));
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, ctx->stream, ticks);
        for (int i = 0; i < N; ++i) {
            HIPCHK(hipEventRecord(ev[2 * i], ctx->stream));
            hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, ctx->stream, ticks);
            HIPCHK(hipEventRecord(ev[2 * i + 1], ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        std::vector<float> t;
        for (int i = 0; i < N; ++i) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1])); t.push_back(ms); }
        std::sort(t.begin(), t.end());
        ctx->profOverheadMs = std::max(0.0, (double)t[t.size() / 2] - (SPIN_US + SPIN_EDGE_US) * 1e-3);
        // ... and of the chained form (one event between consecutive launches: ProfScope)
        HIPCHK(hipEventRecord(ev[0], ctx->stream));
        for (int i = 0; i < N; ++i) {
            hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, ctx->stream, ticks);
            HIPCHK(hipEventRecord(ev[i + 1], ctx->stream));
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        t.clear();
        for (int i = 0; i < N; ++i) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); t.push_back(ms); }
        std::sort(t.begin(), t.end());
        ctx->profOverheadChainMs = std::max(0.0, (double)t[t.size() / 2] - (SPIN_US + SPIN_EDGE_US) * 1e-3);
        for (auto& e : ev) hipEventDestroy(e);
    }
    ctx->ss.profMask = (unsigned)enable;
    for (int i = 0; i < HMCMT_NCAT; ++i) { ctx->profMs[i] = 0; ctx->profN[i] = 0; }
    ctx->profStartSys = ctx->profEvals = ctx->profSolves = ctx->profSolves2 = 0;
    ctx->profSerialIts = ctx->profPersistSolves = 0;
    HIPCHK(hipMemsetAsync(ctx->d_cnt, 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int hmcmt_profile_overhead(const hmcmt_ctx* ctx, double* us) {
    if (!ctx || !us) return HMCMT_EINVAL;
    *us = 1e3 * ctx->profOverheadChainMs;        // (the iteration kernels are sampled in the chained form)
    return 0;
}

int hmcmt_profile_every(hmcmt_ctx* ctx, int32_t n) {
    if (!ctx || n < 1) return HMCMT_EINVAL;
    ctx->profEvery = n;
    return 0;
}

int hmcmt_profile_read(hmcmt_ctx* ctx, double* ms, int64_t* launches) {
    if (!ctx || !ms || !launches) return HMCMT_EINVAL;
    prof_collect(ctx);
    for (int i = 0; i < HMCMT_NCAT; ++i) { ms[i] = ctx->profMs[i]; launches[i] = ctx->profN[i]; }
    return 0;
}

static int set_all_active(hmcmt_ctx* ctx) {
    std::vector<int> one(ctx->v.S, 1);
    HIPCHK(hipMemcpy(ctx->sv.active, one.data(), sizeof(int) * one.size(), hipMemcpyHostToDevice));
    return 0;
}

int hmcmt_debug_transform(hmcmt_ctx* ctx, int32_t which, const double* A, double* C) {
    if (!ctx || !A || !C) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t bytes = (size_t)ctx->v.S * ctx->v.vstride * sizeof(cplx);
    HIPCHK(hipMemcpy(ctx->sv.p, A, bytes, hipMemcpyHostToDevice));
    if (which >= 2) {
        // mixed-precision kernel: q = fp32(A) * V (which == 2) or V' (which == 3), split-bf16 operands, fp32 accumulation
        int rc = set_all_active(ctx);
        if (rc) return rc;
        hipLaunchKernelGGL(k_to_c64, dim3(ctx->sv.NB, ctx->v.S), dim3(VBLOCK), 0, ctx->stream, ctx->sv, ctx->sv.p);
        if ((rc = launch_transform_lp<1>(ctx, ctx->sv.t32, which == 3, ctx->sv.q, nullptr))) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(C, ctx->sv.q, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    launch_transform(ctx, ctx->sv.p, which ? ctx->d_Vt : ctx->d_V, ctx->sv.q, nullptr);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(C, ctx->sv.q, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int hmcmt_debug_flags(hmcmt_ctx* ctx, int32_t flags) {
    if (!ctx || (flags & ~0xff1f) || ((flags & 16) && !(flags & 12)) || ((flags & 0xff00) && !(flags & 4))) return HMCMT_EINVAL;
    if (flags & 8) ctx->dbgPlace = -1;                    // (one-shot: EVERY group of the next persistent launch fails its placement check -- the all-fallback regime of a partitioned device)
    else if (flags & 4) ctx->dbgPlace = 1 + ((flags >> 8) & 0xff);   // (one-shot: the next persistent launch's first system group -- bits 8-15: the group of that index -- fails its placement check)
    if (flags & 12) ctx->dbgPlaceAdj = (flags & 16) != 0;      // (bit 4: ... of the next ADJOINT launch -- forward launches pass it by)
    flags &= 3;
    ctx->ss.dbgFlags = flags;
    ctx->memo[0].valid = ctx->memo[1].valid = false;      // (stored results belong to the flags they were computed under)
    ctx->lfHaveGrad = false;
    return 0;
}

int hmcmt_debug_spmv(hmcmt_ctx* ctx, const double* p, double* q) {
    if (!ctx || !p || !q) return HMCMT_EINVAL;
    if (!ctx->ss.haveModel) { ctx->err = "no evaluation has been run yet"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t bytes = (size_t)ctx->v.S * ctx->v.vstride * sizeof(cplx);
    HIPCHK(hipMemcpy(ctx->sv.p, p, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ctx->sv.q, 0, bytes));
    int rc = set_all_active(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_spmv, dim3(ctx->sv.NB, ctx->v.S), dim3(VBLOCK), 0, ctx->stream, ctx->sv);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(q, ctx->sv.q, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// the extrapolation state of solve kind `kind` as the last evaluation left it: {w_0..w_5, keep, count, field-ring head, model-ring head}
int hmcmt_debug_extrap(hmcmt_ctx* ctx, int32_t kind, double* out) {
    if (!ctx || !out || kind < 0 || kind > 1) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->side));
    HIPCHK(hipMemcpy(out, ctx->d_ext[kind], EXT_PART * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// capture of the initial guesses on / off: while on, every evaluation that extrapolates copies X (Lam) behind k_extrap, on its stream
int hmcmt_debug_guess_capture(hmcmt_ctx* ctx, int32_t enable) {
    if (!ctx) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->side));
    if (enable && !ctx->d_guessCap[0]) {
        const size_t n = (size_t)ctx->v.S * ctx->v.vstride;
        int rc;
        if ((rc = dalloc(ctx, &ctx->d_guessCap[0], n)) || (rc = dalloc(ctx, &ctx->d_guessCap[1], n))) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->guessCapture = enable != 0;
    return 0;
}

// the captured guess of solve kind `kind`: complex [S][NZP][NYP], the padded layout of hmcmt_debug_spmv
int hmcmt_debug_guess(hmcmt_ctx* ctx, int32_t kind, double* out) {
    if (!ctx || !out || kind < 0 || kind > 1) return HMCMT_EINVAL;
    if (!ctx->guessCapture || !ctx->d_guessCap[kind]) { ctx->err = "hmcmt_debug_guess: the capture is off (hmcmt_debug_guess_capture)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->side));
    HIPCHK(hipMemcpy(out, ctx->d_guessCap[kind], (size_t)ctx->v.S * ctx->v.vstride * sizeof(cplx), hipMemcpyDeviceToHost));
    return 0;
}

int hmcmt_debug_precond(hmcmt_ctx* ctx, const double* r, double* z) {
    if (!ctx || !r || !z) return HMCMT_EINVAL;
    if (!ctx->ss.haveModel) { ctx->err = "no evaluation has been run yet"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t bytes = (size_t)ctx->v.S * ctx->v.vstride * sizeof(cplx);
    HIPCHK(hipMemcpy(ctx->sv.r, r, bytes, hipMemcpyHostToDevice));
    int rc = set_all_active(ctx);
    if (rc) return rc;
    {
        const int merged = ctx->sv.merged2;
        AtExit mergedBack([&] { ctx->sv.merged2 = merged; });
        ctx->sv.merged2 = 0;                 // (two sweeps: the last one as a launch of its own, so that z exists in memory)
        ensure_dinv(ctx);
        apply_precond(ctx);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI && ctx->opt.fdm_precision == 0) {
        // the default path leaves its result as complex64 (Solver::z32): widen it for the caller
        const size_t n = (size_t)ctx->v.S * ctx->v.vstride;
        std::vector<float2> h(n);
        HIPCHK(hipMemcpy(h.data(), ctx->sv.z32, n * sizeof(float2), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) { z[2 * i] = h[i].x; z[2 * i + 1] = h[i].y; }
        return 0;
    }
    HIPCHK(hipMemcpy(z, ctx->sv.z, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// production guard on the error-estimate stopping rule: out = {checks so far, largest true residual ||b - A x|| / ||b|| any check has
// seen, the last check's, checks above HMCMT_GUARD_LIMIT (default 1e-6: each prints a warning and makes the next evaluation start cold)}.  Every HMCMT_GUARD_EVERY-th evaluation (default 100; 0: never) forms the true residual of its two solves
// without options.verify, so a chain cannot run unnoticed on an optimistic estimate.
int hmcmt_guard(const hmcmt_ctx* ctx, double* out) {
    if (!ctx || !out) return HMCMT_EINVAL;
    out[0] = (double)ctx->guardChecks; out[1] = ctx->guardWorst; out[2] = ctx->guardLast; out[3] = (double)ctx->guardTrips;
    return 0;
}

// the persistent solve kernel and this context: out = {threads per workgroup / 2 (0: the problem does not fit the kernel),
// workgroups per system, system slots per XCD, enabled (HMCMT_PERSIST, no placement failure so far), solves it has run,
// solves handed back to the launch-per-phase loop because the workgroups of a system were not on one XCD}
int hmcmt_persist_info(const hmcmt_ctx* ctx, int64_t* out, int32_t nout) {
    if (!ctx || !out || nout < 0) return HMCMT_EINVAL;
    // (the caller says how many slots it has: fields are only ever appended, a caller built against an older header gets the ones it knows)
    const int64_t v[HMCMT_PERSIST_INFO_FIELDS] = {
        ctx->cfg.persistCW, ctx->cfg.persistG, ctx->inst.persistSlots, ctx->ss.persistOn ? 1 : 0,
        ctx->persistSolves, ctx->persistFallbacks,
        persist_ok(ctx) ? 1 : 0,              // would the next default-path solve use it (alone on the device, device lock held)
        ctx->cfg.persistCW ? ctx->cfg.persistMW : 0,  // modes per slab
        ctx->cfg.persistCW ? ctx->cfg.persistCS : 0,  // column parts per row block (2: wide meshes)
        ctx->persistTimeouts,                 // timed-out waits (the evaluation was redone with the launch-per-phase loop)
        ctx->cfg.shareIdx, ctx->cfg.shareCnt,         // this context's share of every XCD's CUs (hmcmt_next_cu_share)
        ctx->cfg.persistCW ? ctx->cfg.psKern[0]->strips : 0,   // strips of tile rows per column: 2 (k_cocg_persist) or 4 (k_cocg_persist4: threads = strips x threads_half)
        ctx->ss.persistWhyOff,                   // why the kernel is off: 0 it is not / HMCMT_PERSIST=0, 1 placement (for good), 2 a timed-out wait (tried again after the backoff)
        ctx->fbKind, ctx->fbStalled};         // the last placement fallback: kind of its launch, systems it found started and still active (stalled)
    for (int i = 0; i < nout && i < HMCMT_PERSIST_INFO_FIELDS; ++i) out[i] = v[i];
    return 0;
}

// The compile-time row width of the width-specialised persistent kernel this context launches (112 / 208 / 416 padded nodes per
// row: kernels_persist.h, NYK), 0 = the generic kernel (or no persistent kernel at all).
int hmcmt_persist_width(const hmcmt_ctx* ctx, int32_t* width) {
    if (!ctx || !width) return HMCMT_EINVAL;
    *width = ctx->cfg.persistCW ? ctx->cfg.psKern[0]->nyk : 0;
    return 0;
}

// The order in which the persistent kernel's queues take the systems of a solve of `kind` (0 forward, 1 adjoint): order[q] = the
// system at position q = queue + queues * round (queues = 8 x slots per XCD; persist_balance), the identity while no table is in
// use; *rebalanced = how often this context took a new table.
int hmcmt_persist_order(const hmcmt_ctx* ctx, int32_t kind, int32_t* order, int64_t* rebalanced) {
    if (!ctx || kind < 0 || kind > 1) return HMCMT_EINVAL;
    const std::vector<int>& t = ctx->ss.psOrder[kind];
    if (order) for (int q = 0; q < ctx->sv.S; ++q) order[q] = t.empty() ? q : t[q];
    if (rebalanced) *rebalanced = ctx->ss.psRebalanced;
    return 0;
}

// The packing hmcmt_persist_order's tables are made with, on the caller's costs (no device, no context): nsystems systems of
// cost[s] >= 0 onto `queues` queues that take turns -- position q = queue + queues * round, every queue keeps the number of
// positions the index order gives it --, longest first into the least loaded queue that has room; order[q] = system.
// *makespan (may be NULL) = the largest queue sum of the table; with order == NULL only that of the index order is computed.
int hmcmt_persist_pack(const double* cost, int32_t nsystems, int32_t queues, int32_t* order, double* makespan) {
    if (!cost || nsystems < 1 || queues < 1) return HMCMT_EINVAL;
    std::vector<float> c(nsystems);
    for (int i = 0; i < nsystems; ++i) { if (!(cost[i] >= 0)) return HMCMT_EINVAL; c[i] = (float)cost[i]; }
    if (order) {
        std::vector<int> tab(nsystems);
        pack_queues(c.data(), nsystems, queues, tab.data());
        for (int i = 0; i < nsystems; ++i) order[i] = tab[i];
        if (makespan) *makespan = queues_makespan(c.data(), nsystems, queues, tab.data());
    } else if (makespan) *makespan = queues_makespan(c.data(), nsystems, queues, nullptr);
    return 0;
}

// Would a mesh of ny x nz cells (nz INCLUDING the air layers, as in hmcmt_create) run the one-launch-per-solve kernel on a device
// with `cus_per_xcd` CUs per XCD (32 on MI355X; 16 / 8 for a half / quarter CU share), and in which shape?  Pure arithmetic, no
// device needed: out = {column parts (0: outside the envelope -- the launch-per-phase loop), threads per workgroup / 2,
// workgroups per system, modes per slab, LDS bytes per workgroup, systems per XCD at a time for `nsystems` systems}.
int hmcmt_persist_envelope(int64_t ny, int64_t nz, int32_t cus_per_xcd, int64_t nsystems, int64_t* out) {
    if (!out || ny < 2 || nz < 3 || cus_per_xcd < 1 || nsystems < 1) return HMCMT_EINVAL;
    const ShapeDims k{(int)(((ny + 1) + 15) / 16 * 16), (int)(nz + 1), (int)nz};
    for (int i = 0; i < 6; ++i) out[i] = 0;
    for (int cs = 1; cs <= 2; ++cs) {
        int G = 0, cw = 0, mw = 0; size_t lds = 0;
        if (persist_shape_dims(k, 1, cs, cus_per_xcd, G, cw, mw, lds) && (size_t)nsystems * (size_t)k.NYP * (size_t)k.NZP < ((size_t)1 << 27)) {
            out[0] = cs; out[1] = cw; out[2] = G; out[3] = mw; out[4] = (int64_t)lds;
            out[5] = std::max<int64_t>(1, std::min<int64_t>((nsystems + 7) / 8, cus_per_xcd / G));
            break;
        }
    }
    return 0;
}

// The NEXT hmcmt_create of the calling thread builds a context confined to share `index` of `count` (1, 2 or 4) equal shares of
// the CUs of every XCD of its device: its streams carry a CU mask, and its persistent solve kernel takes that share of the system
// slots -- the persistent kernels of `count` such contexts (independent chains, parallelHMC.jl:23-45 with more chains than
// devices) are co-resident on the device instead of falling back to the launch-per-phase loop (what it buys -- at the
// headline size two chains on halves run at 1.15 x the aggregate steps/s of one chain on the whole device).  The CU-masked streams
// are BLOCKING streams (hipExtStreamCreateWithCUMask takes no flags): they synchronise with the legacy default stream.
int hmcmt_next_cu_share(int32_t index, int32_t count) {
    if ((count != 1 && count != 2 && count != 4) || index < 0 || index >= count) return HMCMT_EINVAL;
    g_nextShareIdx = index; g_nextShareCnt = count;
    return 0;
}

// Test hook: `nblocks` workgroups that each hold 160 KB of LDS (a whole CU) and spin for `ms` milliseconds, on a stream of their
// own -- returns once they are resident (or after 2 s).  What another application on the device does to the persistent kernel's co-residency (tests/test_gpu_persist.py).
int hmcmt_debug_hog(hmcmt_ctx* ctx, int32_t nblocks, int32_t ms) {
    if (!ctx || nblocks < 1 || nblocks > 4096 || ms < 0 || ms > 10000) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    static hipStream_t hogStreams[MAXDEV] = {};                   // (one per device, kept: the kernel outlives this call)
    if (ctx->cfg.device < 0 || ctx->cfg.device >= MAXDEV) return HMCMT_EINVAL;
    hipStream_t& hogStream = hogStreams[ctx->cfg.device];
    if (!hogStream) HIPCHK(hipStreamCreateWithFlags(&hogStream, hipStreamNonBlocking));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_hog), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    // (returns when the hog is RESIDENT -- min(nblocks, the device's CUs) of its workgroups have started, counted in a mapped host
    //  word; a fresh process loads the code object at this first launch, which a fixed sleep in the test did not cover -- or after 2 s)
    static int* hogStarted[MAXDEV] = {};
    int*& started = hogStarted[ctx->cfg.device];
    if (!started) HIPCHK(hipHostMalloc((void**)&started, sizeof(int), hipHostMallocMapped));
    *(volatile int*)started = 0;
    hipLaunchKernelGGL(k_hog, dim3(nblocks), dim3(64), 160 * 1024, hogStream, (long long)ms * 100000ll, started);   // (wall_clock64: 100 MHz)
    HIPCHK(hipGetLastError());
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->cfg.device));
    const int want = std::min(nblocks, ncu > 0 ? ncu : 256);
    const auto t0 = std::chrono::steady_clock::now();
    while (*(volatile int*)started < want && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 2.0) __builtin_ia32_pause();
    return 0;
}

// z = P^-1 r by the persistent solve kernel's own preconditioner (its first application, then it stops): the comparator of
// hmcmt_debug_precond for tests/test_gpu_persist.py.  sweeps = 1 / 2 smoothing sweeps per side.
int hmcmt_debug_persist_precond(hmcmt_ctx* ctx, int32_t sweeps, const double* r, double* z) {
    if (!ctx || !r || !z || (sweeps != 1 && sweeps != 2)) return HMCMT_EINVAL;
    if (!ctx->ss.haveModel) { ctx->err = "no evaluation has been run yet"; return HMCMT_EINVAL; }
    if (!ctx->cfg.persistCW) { ctx->err = "the persistent solve kernel does not apply to this problem"; return HMCMT_EINVAL; }
    if (!persist_alone(ctx)) { ctx->err = "the persistent solve kernel may not run now (another context or process holds the device)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t)ctx->v.S * ctx->v.vstride;
    HIPCHK(hipMemcpy(ctx->sv.r, r, n * sizeof(cplx), hipMemcpyHostToDevice));
    int rc = set_all_active(ctx);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(ctx->sv.z32, 0, n * sizeof(float2), ctx->stream));
    *(volatile int*)ctx->h_prog = 0;
    host_word(ctx, HW_PLACE) = 0;
    ctx->sv.tol2 = ctx->opt.tol * ctx->opt.tol;
    if ((rc = launch_persist(ctx, sweeps, 1, ctx->sv.z32))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (host_word(ctx, HW_PLACE)) { ctx->err = "persistent kernel: the workgroups of a system were not placed on one XCD"; return HMCMT_EHIP; }
    if (host_word(ctx, HW_FAIL) || host_word(ctx, HW_TIMEOUT)) { ctx->err = "persistent kernel: a wait timed out"; return HMCMT_EHIP; }
    std::vector<float2> h(n);
    HIPCHK(hipMemcpy(h.data(), ctx->sv.z32, n * sizeof(float2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { z[2 * i] = h[i].x; z[2 * i + 1] = h[i].y; }
    return 0;
}

// forward half of the mixed-precision FDM stage on a caller-supplied vector: out[0..n) = fused kernel,
// out[n..2n) = separate transform + tridiagonal kernels (complex64 pairs widened to double), n = S*vstride
int hmcmt_debug_fdm_fwd(hmcmt_ctx* ctx, const double* t, double* out) {
    if (!ctx || !t || !out) return HMCMT_EINVAL;
    if (!ctx->ss.haveModel) { ctx->err = "no evaluation has been run yet"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    Solver& k = ctx->sv;
    const size_t n = (size_t)ctx->v.S * ctx->v.vstride;
    HIPCHK(hipMemcpy(k.r, t, n * sizeof(cplx), hipMemcpyHostToDevice));
    int rc = set_all_active(ctx);
    if (rc) return rc;
    std::vector<float2> h(n);
    if (ctx->cfg.fwdStamps) {
        const int gx = (k.NYP / 16 + FW_NTW - 1) / FW_NTW, nb = gx * k.S;
        long long* d_st = nullptr;
        HIPCHK(hipMalloc((void**)&d_st, sizeof(long long) * 8 * nb));
        HIPCHK(hipMemset(d_st, 0, sizeof(long long) * 8 * nb));
        const size_t lds = fdm_fwd_lds(k, FW_NTW, k.twist);
        const int G = (k.NZP + 7) / 8, per = (G + 7) / 8, nw = (G + per - 1) / per;
        hipLaunchKernelGGL(k_to_c64, dim3(k.NB, k.S), dim3(VBLOCK), 0, ctx->stream, k, k.r);
        for (int rep = 0; rep < 3; ++rep)
            hipLaunchKernelGGL(k_fdm_fwd<FW_NTW>, dim3(gx * k.S), dim3(64 * nw), lds, ctx->stream, k, k.t32, ctx->d_Vb, ctx->d_Vbl,
                               ctx->inst.d_invp32, k.y32, d_st);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        std::vector<long long> st(8 * (size_t)nb);
        HIPCHK(hipMemcpy(st.data(), d_st, sizeof(long long) * 8 * nb, hipMemcpyDeviceToHost));
        hipFree(d_st);
        double d[4] = {0, 0, 0, 0};
        long long tmin = st[0], tmax = st[4];
        for (int b = 0; b < nb; ++b) {
            for (int i = 0; i < 4; ++i) d[i] += double(st[8 * b + i + 1] - st[8 * b + i]) / nb;
            tmin = std::min(tmin, st[8 * b]); tmax = std::max(tmax, st[8 * b + 4]);
        }
        fprintf(stderr, "k_fdm_fwd stamps (s_memtime ticks, mean over %d blocks): transform %.0f premul %.0f chain %.0f write %.0f | first start -> last end %lld\n",
                nb, d[0], d[1], d[2], d[3], tmax - tmin);
    }
    const int keepSplit = k.splitT;
    AtExit splitBack([&] { k.splitT = keepSplit; });
    for (int pass = 0; pass < 2; ++pass) {
        k.splitT = pass == 0 && ctx->cfg.fwdNtwFused > 0;      // the operand format goes with the path
        hipLaunchKernelGGL(k_to_c64, dim3(k.NB, k.S), dim3(VBLOCK), 0, ctx->stream, k, k.r);
        HIPCHK(hipMemsetAsync(k.y32, 0xff, n * sizeof(float2), ctx->stream));
        rc = launch_fdm_fwd(ctx, nullptr, pass == 0 ? FdmPath::Fused : FdmPath::Separate);
        const float2* res = k.y32;
        if (!rc && k.splitT) {                              // pre-split result -> complex64 (hi + lo), into t32
            hipLaunchKernelGGL(k_unsplit, dim3(512), dim3(256), 0, ctx->stream, k, k.y32, k.t32);
            res = k.t32;
        }
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(h.data(), res, n * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n; ++i) { out[2 * (pass * n + i)] = h[i].x; out[2 * (pass * n + i) + 1] = h[i].y; }
    }
    return 0;
}

// back half of the FDM stage + post-smoother on caller-supplied vectors: out[0..n) = fused kernel (k_back_post),
// out[n..2n) = k_transform_lp<2> + k_post, n = S*vstride complex; sums[0..2) / [2..4) = sum over systems of the
// r't partials (re, im) of the two paths, sums[4] / [5] = of the |t|^2 partials
int hmcmt_debug_back_post(hmcmt_ctx* ctx, const double* y, const double* r, double* out, double* sums) {
    if (!ctx || !y || !r || !out || !sums) return HMCMT_EINVAL;
    if (!ctx->ss.haveModel) { ctx->err = "no evaluation has been run yet"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    Solver& k = ctx->sv;
    const size_t n = (size_t)ctx->v.S * ctx->v.vstride;
    int rc = set_all_active(ctx);
    if (rc) return rc;
    ensure_dinv(ctx);
    std::vector<cplx> pa((size_t)k.S * MAXNB);
    std::vector<double> pz((size_t)k.S * MAXNB);
    for (int pass = 0; pass < 2; ++pass) {
        // y -> y32 in the operand format of the path (through t32, the buffer k_to_c64 writes), r -> k.r
        HIPCHK(hipMemcpy(k.r, y, n * sizeof(cplx), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_to_c64, dim3(k.NB, k.S), dim3(VBLOCK), 0, ctx->stream, k, k.r);
        HIPCHK(hipMemcpyAsync(k.y32, k.t32, n * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(k.r, r, n * sizeof(cplx), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(k.z32, 0xff, n * sizeof(float2), ctx->stream));
        const FdmPath path = pass == 0 ? FdmPath::Fused : FdmPath::Separate;
        rc = launch_back_post(ctx, path);
        if (!rc && pass == 0 && ctx->cfg.backStamps) {
            const int nb = ((k.nz - 1 + BP_OWN - 1) / BP_OWN) * k.S;
            long long* d_st = nullptr;
            HIPCHK(hipMalloc((void**)&d_st, sizeof(long long) * 8 * nb));
            HIPCHK(hipMemset(d_st, 0, sizeof(long long) * 8 * nb));
            for (int rep = 0; rep < 3 && !rc; ++rep) rc = launch_back_post(ctx, path, d_st);
            HIPCHK(hipStreamSynchronize(ctx->stream));
            std::vector<long long> st(8 * (size_t)nb);
            HIPCHK(hipMemcpy(st.data(), d_st, sizeof(long long) * 8 * nb, hipMemcpyDeviceToHost));
            hipFree(d_st);
            double d[7] = {0, 0, 0, 0, 0, 0, 0};
            long long tmin = st[0], tmax = st[6];
            for (int b = 0; b < nb; ++b) {
                for (int i = 0; i < 6; ++i) d[i] += double(st[8 * b + i + 1] - st[8 * b + i]) / nb;
                d[6] += double(st[8 * b + 7] - st[8 * b]) / nb;
                tmin = std::min(tmin, st[8 * b]); tmax = std::max(tmax, st[8 * b + 6]);
            }
            fprintf(stderr, "k_back_post stamps (s_memtime ticks, mean over %d blocks): stage %.0f mfma(first pair) %.0f epilogue+rest %.0f barrier %.0f stencil %.0f reduce %.0f | start -> loads issued %.0f | first start -> last end %lld\n",
                    nb, d[0], d[1], d[2], d[3], d[4], d[5], d[6], tmax - tmin);
        }
        if (rc) return rc;
        std::vector<float2> hz(n);                              // both paths leave the result as complex64 in z32
        HIPCHK(hipMemcpyAsync(hz.data(), k.z32, n * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(pa.data(), k.partA, pa.size() * sizeof(cplx), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(pz.data(), ctx->inst.d_partZZ, pz.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n; ++i) { out[2 * (pass * n + i)] = hz[i].x; out[2 * (pass * n + i) + 1] = hz[i].y; }
        double are = 0, aim = 0, zz = 0;
        for (int s = 0; s < k.S; ++s)
            for (int b = 0; b < k.NB; ++b) { are += pa[(size_t)s * MAXNB + b].re; aim += pa[(size_t)s * MAXNB + b].im; zz += pz[(size_t)s * MAXNB + b]; }
        sums[2 * pass] = are; sums[2 * pass + 1] = aim; sums[4 + pass] = zz;
    }
    return 0;
}

// ---- mass matrix (hmcmt_set_mass / hmcmt_mass_apply, kernels_mass.h) --------------------------------------------------------
constexpr int MASS_PCG_MAXIT = 1000;
constexpr double MASS_PCG_TOL = 1e-13;

// the buffers of the low-rank mass alone (a Wm factor stays)
static void mass_lr_free(hmcmt_ctx* ctx, std::initializer_list<void*> bufs) {
    for (void* old : bufs) {
        if (!old) continue;
        auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), old);
        if (it != ctx->allocs.end()) ctx->allocs.erase(it);
        hipFree(old);
    }
}
static void mass_lr_release(hmcmt_ctx* ctx) {
    auto& M = ctx->mass;
    mass_lr_free(ctx, {M.d_lrS, M.d_lrU, M.d_lrC, M.d_lrPart});
    M.d_lrS = M.d_lrU = M.d_lrC = M.d_lrPart = nullptr;
    M.lrRank = M.lrCap = 0;
    M.lrLambda.clear();
    M.lrInvM.clear();
}

static void mass_release(hmcmt_ctx* ctx) {
    auto& M = ctx->mass;
    mass_lr_release(ctx);
    for (void* old : {(void*)M.d_L, (void*)M.d_Qz, (void*)M.d_QzT, (void*)M.d_Qy, (void*)M.d_QyT, (void*)M.d_lz, (void*)M.d_ly,
                      (void*)M.d_T1, (void*)M.d_T2, (void*)M.d_x, (void*)M.d_in, (void*)M.d_out, (void*)M.d_r, (void*)M.d_z,
                      (void*)M.d_pp, (void*)M.d_q, (void*)M.d_s, (void*)M.d_map}) {
        if (!old) continue;
        auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), old);
        if (it != ctx->allocs.end()) ctx->allocs.erase(it);
        hipFree(old);
    }
    const int kind = M.kind;
    M = hmcmt_ctx::Mass{};
    M.kind = kind;
}

// Banded Cholesky of Wm (the CSR of hmcmt_set_prior) in the natural order, row by row (Cholesky-Banachiewicz; the dot products
// run over contiguous stretches of two rows of the band).  Lb[i*(b+1) + j - i + b] = L[i][j].  Returns -1 - i for a pivot <= 0.
static long long mass_factor(int n, int b, const std::vector<long long>& row, const std::vector<long long>& col,
                             const std::vector<double>& val, std::vector<double>& Lb) {
    const long long w = b + 1;
    Lb.assign((size_t)n * w, 0.0);
    for (int i = 0; i < n; ++i)
        for (long long t = row[i]; t < row[i + 1]; ++t)
            if (col[t] <= i) Lb[(size_t)i * w + (col[t] - i + b)] += val[t];
    for (int i = 0; i < n; ++i) {
        double* Li = &Lb[(size_t)i * w];
        const int j0 = std::max(0, i - b);
        for (int j = j0; j <= i; ++j) {
            const double* Lj = &Lb[(size_t)j * w];
            double s = Li[j - i + b];
            // sum over k = j0 .. j-1 of L[i][k] L[j][k]
            const double* a = Li + (j0 - i + b);
            const double* c = Lj + (j0 - j + b);
            double acc = 0.0;
            for (int k = 0; k < j - j0; ++k) acc += a[k] * c[k];
            s -= acc;
            if (j < i) Li[j - i + b] = s / Lj[b];
            else {
                if (!(s > 0.0)) return -1 - (long long)i;
                Li[b] = std::sqrt(s);
            }
        }
    }
    return 0;
}

// Does Wm equal I (x) T_y + T_z (x) I on the active box (kernels_mass.h)?  Exact comparison of every stored entry.
static bool mass_separable(int n, int nzb, int nyb, const std::vector<int>& map, const std::vector<long long>& row,
                           const std::vector<long long>& col, const std::vector<double>& val) {
    if ((long long)nzb * nyb != n) return false;
    for (int iz = 0; iz < nzb; ++iz)
        for (int jy = 0; jy < nyb; ++jy) {
            const int a = map[(size_t)iz * nyb + jy];
            int nb[4], cnt = 0;
            if (jy > 0) nb[cnt++] = map[(size_t)iz * nyb + jy - 1];
            if (jy < nyb - 1) nb[cnt++] = map[(size_t)iz * nyb + jy + 1];
            if (iz > 0) nb[cnt++] = map[(size_t)(iz - 1) * nyb + jy];
            if (iz < nzb - 1) nb[cnt++] = map[(size_t)(iz + 1) * nyb + jy];
            double want[5], have[5] = {0, 0, 0, 0, 0};
            int who[5];
            who[0] = a; want[0] = cnt + (iz == 0 ? 1.0 : 0.0);
            for (int q = 0; q < cnt; ++q) { who[q + 1] = nb[q]; want[q + 1] = -1.0; }
            for (long long t = row[a]; t < row[a + 1]; ++t) {
                int q = 0;
                while (q <= cnt && who[q] != col[t]) ++q;
                if (q > cnt) { if (val[t] != 0.0) return false; continue; }
                have[q] += val[t];
            }
            for (int q = 0; q <= cnt; ++q) if (have[q] != want[q]) return false;
        }
    return true;
}

// the eigenpairs of T_y (Neumann, DCT-II) and T_z (air above the top row), columns = eigenvectors, unit 2-norm
static void mass_eigen(int n, bool topDirichlet, std::vector<double>& Q, std::vector<double>& lam) {
    const double pi = 3.14159265358979323846;
    Q.assign((size_t)n * n, 0.0);
    lam.assign(n, 0.0);
    for (int k = 0; k < n; ++k) {
        const double th = topDirichlet ? pi * (2 * k + 1) / (2.0 * n + 1.0) : pi * k / n;
        lam[k] = 2.0 - 2.0 * std::cos(th);
        double nn = 0.0;
        for (int i = 0; i < n; ++i) {
            const double q = topDirichlet ? std::sin(th * (i + 1)) : std::cos(th * (i + 0.5));
            Q[(size_t)i * n + k] = q;
            nn += q * q;
        }
        const double s = 1.0 / std::sqrt(nn);
        for (int i = 0; i < n; ++i) Q[(size_t)i * n + k] *= s;
    }
}
static std::vector<double> transposed(const std::vector<double>& Q, int n) {
    std::vector<double> T(Q.size());
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) T[(size_t)k * n + i] = Q[(size_t)i * n + k];
    return T;
}

static int mass_build(hmcmt_ctx* ctx) {
    auto& M = ctx->mass;
    const int n = ctx->v.nAC, ny = ctx->v.ny;
    const auto& row = ctx->wmRowH; const auto& col = ctx->wmColH; const auto& val = ctx->wmValH;
    mass_release(ctx);
    int b = 0;
    for (int i = 0; i < n; ++i)
        for (long long t = row[i]; t < row[i + 1]; ++t) b = std::max<long long>(b, std::llabs(col[t] - i));
    std::vector<double> Lb;
    const auto t0 = std::chrono::steady_clock::now();
    const long long fr = mass_factor(n, b, row, col, val, Lb);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (fr) {
        ctx->err = "hmcmt_set_mass: Wm is not positive definite (Cholesky pivot <= 0 at active cell " + std::to_string(-1 - fr) + ")";
        return HMCMT_EINVAL;
    }
    // the box of the active cells and its map
    int kz0 = 1 << 30, kz1 = -1, ky0 = 1 << 30, ky1 = -1;
    for (int a = 0; a < n; ++a) {
        const int c = ctx->hp.act[a], kz = c / ny, ky = c % ny;
        kz0 = std::min(kz0, kz); kz1 = std::max(kz1, kz); ky0 = std::min(ky0, ky); ky1 = std::max(ky1, ky);
    }
    const int nzb = kz1 - kz0 + 1, nyb = ky1 - ky0 + 1;
    std::vector<int> map((size_t)nzb * nyb, -1);
    for (int a = 0; a < n; ++a) {
        const int c = ctx->hp.act[a];
        map[(size_t)(c / ny - kz0) * nyb + (c % ny - ky0)] = a;
    }
    std::vector<double> Qz, lz, Qy, ly;
    mass_eigen(nzb, true, Qz, lz);
    mass_eigen(nyb, false, Qy, ly);
    int rc;
    if ((rc = dupload(ctx, &M.d_L, Lb))) return rc;
    if ((rc = dupload(ctx, &M.d_map, map))) return rc;
    if ((rc = dupload(ctx, &M.d_Qz, Qz))) return rc;
    if ((rc = dupload(ctx, &M.d_QzT, transposed(Qz, nzb)))) return rc;
    if ((rc = dupload(ctx, &M.d_Qy, Qy))) return rc;
    if ((rc = dupload(ctx, &M.d_QyT, transposed(Qy, nyb)))) return rc;
    if ((rc = dupload(ctx, &M.d_lz, lz))) return rc;
    if ((rc = dupload(ctx, &M.d_ly, ly))) return rc;
    for (double** p : {&M.d_T1, &M.d_T2})
        if ((rc = dalloc(ctx, p, (size_t)nzb * nyb))) return rc;
    for (double** p : {&M.d_x, &M.d_in, &M.d_out, &M.d_r, &M.d_z, &M.d_pp, &M.d_q})
        if ((rc = dalloc(ctx, p, (size_t)n))) return rc;
    if ((rc = dalloc(ctx, &M.d_s, (size_t)8))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    M.bw = b; M.nzb = nzb; M.nyb = nyb; M.factorSec = sec;
    M.separable = mass_separable(n, nzb, nyb, map, row, col, val) ? 1 : 0;
    M.keyRow = row; M.keyCol = col; M.keyVal = val;
    M.ready = true;
    return 0;
}

// y = B^-1 x restricted to the active cells, B the box operator: four fp64 GEMMs (x, y [nAC] device; y may be x)
static void mass_box_inv(hmcmt_ctx* ctx, const double* x, double* y) {
    const auto& M = ctx->mass;
    hipStream_t st = ctx->stream;
    const int nz = M.nzb, ny = M.nyb;
    const dim3 grid((ny + MG_T - 1) / MG_T, (nz + MG_T - 1) / MG_T), blk(256);
    MassGemm g{nz, ny, nz, M.d_QzT, nullptr, M.d_T1, M.d_map, x, nullptr, M.d_lz, M.d_ly};
    hipLaunchKernelGGL(k_mass_gemm<MG_SCATTER_B>, grid, blk, 0, st, g);               // Q_z' X
    g = MassGemm{nz, ny, ny, M.d_T1, M.d_Qy, M.d_T2, M.d_map, nullptr, nullptr, M.d_lz, M.d_ly};
    hipLaunchKernelGGL(k_mass_gemm<MG_DIVIDE>, grid, blk, 0, st, g);                  // (.. Q_y) ./ (lz_i + ly_j)
    g = MassGemm{nz, ny, nz, M.d_Qz, M.d_T2, M.d_T1, M.d_map, nullptr, nullptr, M.d_lz, M.d_ly};
    hipLaunchKernelGGL(k_mass_gemm<0>, grid, blk, 0, st, g);                          // Q_z ..
    g = MassGemm{nz, ny, ny, M.d_T1, M.d_QyT, nullptr, M.d_map, nullptr, y, M.d_lz, M.d_ly};
    hipLaunchKernelGGL(k_mass_gemm<MG_GATHER_C>, grid, blk, 0, st, g);                // (.. Q_y') restricted
}

// y = Wm^-1 b by PCG (fp64; preconditioner mass_box_inv).  Synchronises with the device once per iteration.
static int mass_pcg(hmcmt_ctx* ctx, const double* b, double* y) {
    auto& M = ctx->mass;
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    const dim3 g1((n + 255) / 256), b1(256);
    const size_t bytes = sizeof(double) * n;
    M.pcgIters = 0;
    double h[8];
    HIPCHK(hipMemcpyAsync(M.d_r, b, bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(M.d_out, 0, bytes, st));
    mass_box_inv(ctx, M.d_r, M.d_z);
    HIPCHK(hipMemcpyAsync(M.d_pp, M.d_z, bytes, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_mass_dot, dim3(1), dim3(1024), 0, st, n, M.d_r, M.d_z, M.d_s, 0);
    hipLaunchKernelGGL(k_mass_dot, dim3(1), dim3(1024), 0, st, n, M.d_r, M.d_r, M.d_s, 3);
    HIPCHK(hipMemcpyAsync(h, M.d_s, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const double bnorm = std::sqrt(h[3]);
    if (!std::isfinite(bnorm)) { ctx->err = "hmcmt_mass_apply: non-finite input"; return HMCMT_EBREAKDOWN; }
    int it = 0;
    if (bnorm > 0.0) {
        for (;;) {
            if (it == MASS_PCG_MAXIT) {
                ctx->err = "hmcmt_mass_apply: PCG on Wm did not reach its tolerance within " + std::to_string(MASS_PCG_MAXIT) + " iterations";
                M.pcgIters = it;
                return HMCMT_ENOCONV;
            }
            ++it;
            hipLaunchKernelGGL(k_mass_spmv, g1, b1, 0, st, n, ctx->d_wmRow, ctx->d_wmCol, ctx->d_wmVal, M.d_pp, M.d_q);
            hipLaunchKernelGGL(k_mass_dot, dim3(1), dim3(1024), 0, st, n, M.d_pp, M.d_q, M.d_s, 1);
            hipLaunchKernelGGL(k_mass_xr, g1, b1, 0, st, n, M.d_s, M.d_pp, M.d_q, M.d_out, M.d_r);
            mass_box_inv(ctx, M.d_r, M.d_z);
            hipLaunchKernelGGL(k_mass_dot, dim3(1), dim3(1024), 0, st, n, M.d_r, M.d_z, M.d_s, 2);
            hipLaunchKernelGGL(k_mass_dot, dim3(1), dim3(1024), 0, st, n, M.d_r, M.d_r, M.d_s, 4);
            HIPCHK(hipMemcpyAsync(h, M.d_s, sizeof(double) * 5, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!(h[1] > 0.0) || !std::isfinite(h[2]) || !std::isfinite(h[4])) {
                ctx->err = "hmcmt_mass_apply: PCG breakdown (p'Wm p <= 0 or non-finite values)";
                M.pcgIters = it;
                return HMCMT_EBREAKDOWN;
            }
            if (std::sqrt(h[4]) <= MASS_PCG_TOL * bnorm) break;
            hipLaunchKernelGGL(k_mass_p, g1, b1, 0, st, n, M.d_s, M.d_z, M.d_pp);
            HIPCHK(hipMemcpyAsync(M.d_s, M.d_s + 2, sizeof(double), hipMemcpyDeviceToDevice, st));
        }
    }
    M.pcgIters = it;
    HIPCHK(hipMemcpyAsync(y, M.d_out, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

// y = M^-1 x or L x on device vectors, enqueued on the context's stream (PCG: complete on return)
static int mass_apply_dev(hmcmt_ctx* ctx, int op, const double* x, double* y) {
    auto& M = ctx->mass;
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    if (M.kind == HMCMT_MASS_DIAGONAL) {
        hipLaunchKernelGGL(k_mass_diag, dim3((n + 255) / 256), dim3(256), 0, st, n, ctx->d_invM, x, y, op);
        return 0;
    }
    if (M.kind == HMCMT_MASS_LOWRANK) {
        const MassLr m{n, M.lrRank, op, M.d_lrS, M.d_lrU, M.d_lrC + (op == HMCMT_MASS_OP_INV ? 0 : M.lrRank), M.d_lrPart};
        hipLaunchKernelGGL(k_mass_lr_project, dim3(LFNB), dim3(256), 0, st, m, x);
        hipLaunchKernelGGL(k_mass_lr_expand, dim3(LFNB), dim3(256), 0, st, m, x, y);
        return 0;
    }
    if (op == HMCMT_MASS_OP_SQRT) {
        double* out = (x == y) ? M.d_out : y;
        hipLaunchKernelGGL(k_mass_lmul, dim3((n + 3) / 4), dim3(256), 0, st, n, M.bw, M.d_L, x, out);
        if (out != y) HIPCHK(hipMemcpyAsync(y, out, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (M.separable) { M.pcgIters = 0; mass_box_inv(ctx, x, y); return 0; }
    return mass_pcg(ctx, x, y);
}

int hmcmt_set_prior(hmcmt_ctx* ctx, const double* mref, const int64_t* rowptr, const int64_t* colind,
                    const double* val, const double* invM) {
    if (!ctx || !mref || !rowptr || !colind || !val || !invM) return HMCMT_EINVAL;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const int n = ctx->v.nAC;
    const int64_t nnz = rowptr[n];
    if (rowptr[0] != 0 || nnz < 0) { ctx->err = "Wm row pointer must be 0-based CSR"; return HMCMT_EINVAL; }
    for (int64_t t = 0; t < nnz; ++t)
        if (colind[t] < 0 || colind[t] >= n) { ctx->err = "Wm column index out of range"; return HMCMT_EINVAL; }
    std::vector<double> v_mref(mref, mref + n), v_invM(invM, invM + n), v_val(val, val + nnz);
    std::vector<long long> v_row(rowptr, rowptr + n + 1), v_col(colind, colind + nnz);
    int rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));              // (a trajectory may still be reading the previous prior)
    chain_release(ctx);                                     // (a chain belongs to the prior it began with)
    map_release(ctx);                                       // (... and so does a MAP run)
    mass_lr_release(ctx);                                   // (... and so does a low-rank mass: its scales default to this prior's invM)
    if (ctx->mass.kind == HMCMT_MASS_LOWRANK) ctx->mass.kind = HMCMT_MASS_DIAGONAL;
    // a repeated call replaces the previous prior: its buffers are released, not kept until hmcmt_destroy
    for (void* old : {(void*)ctx->d_mref, (void*)ctx->d_invM, (void*)ctx->d_wmVal, (void*)ctx->d_wmRow, (void*)ctx->d_wmCol}) {
        if (!old) continue;
        auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), old);
        if (it != ctx->allocs.end()) ctx->allocs.erase(it);
        hipFree(old);
    }
    ctx->d_mref = ctx->d_invM = ctx->d_wmVal = nullptr; ctx->d_wmRow = ctx->d_wmCol = nullptr;
    ctx->havePrior = false;
    if ((rc = dupload(ctx, &ctx->d_mref, v_mref))) return rc;
    if ((rc = dupload(ctx, &ctx->d_invM, v_invM))) return rc;
    if ((rc = dupload(ctx, &ctx->d_wmVal, v_val))) return rc;
    if ((rc = dupload(ctx, &ctx->d_wmRow, v_row))) return rc;
    if ((rc = dupload(ctx, &ctx->d_wmCol, v_col))) return rc;
    if (!ctx->d_p) {
        if ((rc = dalloc(ctx, &ctx->d_p, (size_t)n))) return rc;
        if ((rc = dalloc(ctx, &ctx->d_mcur, (size_t)n))) return rc;
        if ((rc = dalloc(ctx, &ctx->d_g, (size_t)n))) return rc;
        if ((rc = dalloc(ctx, &ctx->d_lfPart, (size_t)LFNB))) return rc;
        if ((rc = dalloc(ctx, &ctx->d_lfScal, (size_t)4))) return rc;
        if ((rc = dalloc(ctx, &ctx->d_lfFlag, (size_t)1))) return rc;
        if ((rc = dalloc(ctx, &ctx->d_lfDone, (size_t)n))) return rc;
        if ((rc = dalloc(ctx, &ctx->d_gStart, (size_t)n))) return rc;
        HIPCHK(hipHostMalloc((void**)&ctx->h_lfFlag, sizeof(int), hipHostMallocDefault));
        *ctx->h_lfFlag = 0;
    }
    ctx->lfHaveGrad = false;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->wmRowH = std::move(v_row); ctx->wmColH = std::move(v_col); ctx->wmValH = std::move(v_val);
    ctx->mass.kind = HMCMT_MASS_DIAGONAL;                   // (hmcmt_set_mass chooses again; a factor of the same Wm is kept)
    ctx->havePrior = true;
    return 0;
}

int hmcmt_set_mass(hmcmt_ctx* ctx, int32_t kind) {
    if (!ctx) return HMCMT_EINVAL;
    if (!ctx->havePrior) { ctx->err = "hmcmt_set_mass: hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (kind != HMCMT_MASS_DIAGONAL && kind != HMCMT_MASS_WM) {
        ctx->err = kind == HMCMT_MASS_LOWRANK ? "hmcmt_set_mass: HMCMT_MASS_LOWRANK is set by hmcmt_set_mass_lowrank, which takes its scales and directions"
                                              : "hmcmt_set_mass: kind must be HMCMT_MASS_DIAGONAL or HMCMT_MASS_WM";
        return HMCMT_EINVAL;
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));              // (a trajectory may still be reading the mass buffers)
    chain_release(ctx);                                     // (... and to the mass)
    map_release(ctx);
    ctx->mass.kind = HMCMT_MASS_DIAGONAL;
    mass_lr_release(ctx);
    if (kind == HMCMT_MASS_DIAGONAL) return 0;
    auto& M = ctx->mass;
    if (!(M.ready && M.keyRow == ctx->wmRowH && M.keyCol == ctx->wmColH && M.keyVal == ctx->wmValH)) {
        const int rc = mass_build(ctx);
        if (rc) { mass_release(ctx); return rc; }
    }
    M.kind = HMCMT_MASS_WM;
    return 0;
}

// max |U U' - I| of rank directions ALREADY ON THE DEVICE, with the projection kernel: row j of U projected onto every row (d_s and d_c
// are only carried along: HMCMT_MASS_OP_SQRT reads neither).  One wait.
static int mass_lr_defect(hmcmt_ctx* ctx, int rank, const double* d_s, const double* d_U, const double* d_c, double* d_part, double* defect) {
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    std::vector<double> part((size_t)rank * rank * LFNB);
    const MassLr m{n, rank, HMCMT_MASS_OP_SQRT, d_s, d_U, d_c, d_part};
    for (int j = 0; j < rank; ++j) {
        hipLaunchKernelGGL(k_mass_lr_project, dim3(LFNB), dim3(256), 0, st, m, d_U + (size_t)j * n);
        HIPCHK(hipMemcpyAsync(&part[(size_t)j * rank * LFNB], d_part, sizeof(double) * rank * LFNB, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    double worst = 0.0;
    for (int j = 0; j < rank; ++j)
        for (int k = 0; k < rank; ++k) {
            const double g = item_chain_total(&part[((size_t)j * rank + k) * LFNB]) - (j == k ? 1.0 : 0.0);
            worst = std::isfinite(g) ? std::max(worst, std::fabs(g)) : INFINITY;
        }
    *defect = worst;
    return 0;
}
// the low-rank mass's own buffers for `rank` directions (nothing uploaded), and the three vectors every non-diagonal mass shares
static int mass_lr_alloc(hmcmt_ctx* ctx, int rank, double** d_s, double** d_U, double** d_c, double** d_part) {
    const int n = ctx->v.nAC;
    int rc;
    if ((rc = dalloc(ctx, d_s, (size_t)n, false))) return rc;             // (s, U and c are written before they are read)
    if ((rc = dalloc(ctx, d_U, (size_t)rank * n, false))) return rc;
    if ((rc = dalloc(ctx, d_c, (size_t)2 * rank, false))) return rc;
    if ((rc = dalloc(ctx, d_part, (size_t)rank * LFNB))) return rc;
    for (double** p : {&ctx->mass.d_x, &ctx->mass.d_in, &ctx->mass.d_out})
        if (!*p && (rc = dalloc(ctx, p, (size_t)n))) return rc;
    return 0;
}
// allocates, uploads s, U, the two coefficient rows and checks U U' = I
static int mass_lr_build(hmcmt_ctx* ctx, int rank, const std::vector<double>& s, const double* U, const std::vector<double>& c,
                         double** d_s, double** d_U, double** d_c, double** d_part, double* defect) {
    const int n = ctx->v.nAC;
    int rc;
    if ((rc = mass_lr_alloc(ctx, rank, d_s, d_U, d_c, d_part))) return rc;
    HIPCHK(hipMemcpy(*d_s, s.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(*d_U, U, sizeof(double) * rank * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(*d_c, c.data(), sizeof(double) * 2 * rank, hipMemcpyHostToDevice));
    return mass_lr_defect(ctx, rank, *d_s, *d_U, *d_c, *d_part, defect);
}

int hmcmt_set_mass_lowrank(hmcmt_ctx* ctx, const double* invM, int32_t rank, const double* U, const double* lambda) {
    const char* fn = "hmcmt_set_mass_lowrank";
    if (!ctx) return HMCMT_EINVAL;
    if (!ctx->havePrior) { ctx->err = std::string(fn) + ": hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (!U || !lambda) { ctx->err = std::string(fn) + (!U ? ": U is NULL" : ": lambda is NULL"); return HMCMT_EINVAL; }
    if (rank < 1 || rank > HMCMT_MASS_RANK_MAX) {
        ctx->err = std::string(fn) + ": rank " + std::to_string(rank) + " is outside 1 .. HMCMT_MASS_RANK_MAX = " + std::to_string(HMCMT_MASS_RANK_MAX);
        return HMCMT_EINVAL;
    }
    const int n = ctx->v.nAC;
    std::vector<double> s((size_t)n), c((size_t)2 * rank);
    for (int k = 0; k < rank; ++k) {
        if (!std::isfinite(lambda[k]) || !(lambda[k] > 0.0)) {
            ctx->err = std::string(fn) + ": lambda[" + std::to_string(k) + "] is not finite and positive";
            return HMCMT_EINVAL;
        }
        c[k] = lambda[k] - 1.0;
        c[rank + k] = 1.0 / std::sqrt(lambda[k]) - 1.0;
    }
    for (size_t i = 0; i < (size_t)rank * n; ++i)
        if (!std::isfinite(U[i])) {
            ctx->err = std::string(fn) + ": U[" + std::to_string(i / n) + "][" + std::to_string(i % n) + "] is not finite";
            return HMCMT_EINVAL;
        }
    if (invM)
        for (int a = 0; a < n; ++a) s[a] = invM[a];
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));              // (a trajectory may still be reading the mass buffers)
    if (!invM) HIPCHK(hipMemcpy(s.data(), ctx->d_invM, sizeof(double) * n, hipMemcpyDeviceToHost));   // (the diagonal in force)
    for (int a = 0; a < n; ++a) {
        if (!std::isfinite(s[a]) || !(s[a] > 0.0)) {
            ctx->err = std::string(fn) + ": invM[" + std::to_string(a) + "] is not finite and positive";
            return HMCMT_EINVAL;
        }
        s[a] = std::sqrt(s[a]);
    }
    auto& M = ctx->mass;
    double *d_s = nullptr, *d_U = nullptr, *d_c = nullptr, *d_part = nullptr, defect = 0.0;
    const int rc = mass_lr_build(ctx, rank, s, U, c, &d_s, &d_U, &d_c, &d_part, &defect);
    if (rc || !(defect <= 1e-8)) {
        const std::string e = ctx->err;
        mass_lr_free(ctx, {d_s, d_U, d_c, d_part});
        if (rc) {                                           // (out of memory: the context is left on the diagonal mass)
            chain_release(ctx);
            map_release(ctx);
            mass_lr_release(ctx);
            M.kind = HMCMT_MASS_DIAGONAL;
            ctx->err = e;
            return rc;
        }
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.3e", defect);
        ctx->err = std::string(fn) + ": the rows of U are not orthonormal (max |U'U - I| = " + buf + " > 1e-8)";
        return HMCMT_EINVAL;                                // (nothing has changed: the mass and a running chain stay)
    }
    chain_release(ctx);                                     // (a chain belongs to the mass it began with)
    map_release(ctx);
    mass_lr_release(ctx);
    M.d_lrS = d_s; M.d_lrU = d_U; M.d_lrC = d_c; M.d_lrPart = d_part;
    M.lrRank = M.lrCap = rank;
    M.lrLambda.assign(lambda, lambda + rank);
    if (invM) M.lrInvM.assign(invM, invM + n);
    M.kind = HMCMT_MASS_LOWRANK;
    return 0;
}

int hmcmt_mass_apply(hmcmt_ctx* ctx, int32_t op, const double* x, double* y, int32_t on_device) {
    if (!ctx || !x || !y) return HMCMT_EINVAL;
    if (!ctx->havePrior) { ctx->err = "hmcmt_mass_apply: hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (op != HMCMT_MASS_OP_INV && op != HMCMT_MASS_OP_SQRT) { ctx->err = "hmcmt_mass_apply: op must be HMCMT_MASS_OP_INV or HMCMT_MASS_OP_SQRT"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const int n = ctx->v.nAC;
    int rc;
    if (ctx->mass.kind == HMCMT_MASS_DIAGONAL && !ctx->mass.d_in) {
        if ((rc = dalloc(ctx, &ctx->mass.d_in, (size_t)n))) return rc;
        if ((rc = dalloc(ctx, &ctx->mass.d_out, (size_t)n))) return rc;
    }
    if (on_device) {
        if ((rc = mass_apply_dev(ctx, op, x, y))) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    auto& M = ctx->mass;
    HIPCHK(hipMemcpyAsync(M.d_in, x, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = mass_apply_dev(ctx, op, M.d_in, M.d_in))) return rc;
    HIPCHK(hipMemcpyAsync(y, M.d_in, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

int hmcmt_mass_info(const hmcmt_ctx* ctx, double* out) {
    if (!ctx || !out) return HMCMT_EINVAL;
    const auto& M = ctx->mass;
    const double v[HMCMT_MASS_INFO_FIELDS] = {(double)M.kind, M.factorSec, (double)M.bw, (double)M.separable, (double)M.pcgIters,
                                              (double)M.nzb, (double)M.nyb};
    // (the fields behind the kind describe the Wm factor: 0 under HMCMT_MASS_LOWRANK, also while a factor is kept)
    for (int i = 0; i < HMCMT_MASS_INFO_FIELDS; ++i) out[i] = (i > 0 && M.kind == HMCMT_MASS_LOWRANK) ? 0.0 : v[i];
    return 0;
}

// One trajectory on device vectors d_m, d_p (updated in place).  startGrad: 0 evaluate the gradient at the start
// model, 1 ctx->d_g holds it (the start model is the end model of the previous trajectory), 2 ctx->d_gStart holds it
// (the start model is the start model of the previous trajectory: a rejected proposal).  Returns with everything
// enqueued on the context's stream and the solver status of every evaluation collected.
static int leapfrog_core(hmcmt_ctx* ctx, double* d_m, double* d_p, double dt, int32_t L, double regParam, double lnSigMin,
                         double lnSigMax, int startGrad, double* d_pred, double* d_misfit, int* evalsOut) {
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemsetAsync(ctx->d_lfFlag, 0, sizeof(int), st));
    LfView lf{n, ctx->d_mref, ctx->d_invM, ctx->d_wmVal, ctx->d_wmRow, ctx->d_wmCol, d_m, d_p, ctx->d_g,
              ctx->d_lfPart, ctx->d_lfScal, ctx->d_lfFlag, ctx->v.ticks};
    const dim3 g1((n + 127) / 128), b1(128);
    int evals = 0;
    int rc = 0;
    if (startGrad == 0) {
        rc = evaluate(ctx, d_m, true, d_pred, d_misfit, ctx->d_g);
        if (rc) return rc;
        if ((rc = collect_stats(ctx, true))) return rc;
        if ((rc = finish_status(ctx))) return rc;
    } else if (startGrad == 2) {
        HIPCHK(hipMemcpyAsync(ctx->d_g, ctx->d_gStart, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    }
    if (startGrad != 2) HIPCHK(hipMemcpyAsync(ctx->d_gStart, ctx->d_g, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    ++evals;                                                 // counted as the reference counts it (hmcprior.nfevals, :217)
    // (momentum update and the step bound of the position update behind it in one launch)
    hipLaunchKernelGGL(k_lf_momentum_max, dim3(LFNB), dim3(256), 0, st, lf, regParam, 0.5 * dt, dt);
    // M = Wm (hmcmt_set_mass): x = Wm^-1 p after every momentum update, the step bound and the position update read x.  The
    // position and momentum updates are then launches of their own (k_mass_step in front of the evaluation, k_lf_momentum_max
    // behind it); the fused forms of the diagonal mass stay as they are.
    // The low-rank mass (hmcmt_set_mass_lowrank) takes the same route with x = M^-1 p from its two kernels, everything enqueued.
    const bool wm = ctx->mass.kind != HMCMT_MASS_DIAGONAL;
    auto mass_x_bound = [&]() -> int {
        if (ctx->mass.kind == HMCMT_MASS_WM && !ctx->mass.separable) {   // (PCG synchronises: the records of the evaluation in flight are read first)
            const int r = collect_pending(ctx);
            if (r) return r;
        }
        const int r = mass_apply_dev(ctx, HMCMT_MASS_OP_INV, d_p, ctx->mass.d_x);
        if (r) return r;
        hipLaunchKernelGGL(k_mass_bound, dim3(LFNB), dim3(256), 0, st, n, ctx->mass.d_x, dt, ctx->d_lfPart);
        return 0;
    };
    if (wm && (rc = mass_x_bound())) return rc;
    for (int k = 1; k <= L; ++k) {
        if (wm) {
            hipLaunchKernelGGL(k_mass_step, g1, b1, 0, st, lf, ctx->mass.d_x, dt, lnSigMin, lnSigMax);
        } else {
            ctx->ss.lfStep = LfStep{1, lf, dt, lnSigMin, lnSigMax};            // (the position update: performed by the evaluation's first kernel)
            // (... and the momentum update behind the gradient, with the step bound of the next position update, by its last one)
            ctx->ss.lfMom = LfMom{1, lf, regParam, (k < L ? 1.0 : 0.5) * dt, dt, ++ctx->lfGen, ctx->d_lfDone};
        }
        rc = evaluate(ctx, d_m, true, d_pred, d_misfit, ctx->d_g);      // (reports a failure of the step before)
        ctx->ss.lfStep.on = 0;
        ctx->ss.lfMom.on = 0;
        if (rc) return rc;
        // asynchronous, as hmcmt_grad_device_async: the next step's launches overlap this step's gradient tail
        ctx->statsPending = true;
        ctx->pendingAdj = true;
        ++evals;
        if (wm) {
            hipLaunchKernelGGL(k_lf_momentum_max, dim3(LFNB), dim3(256), 0, st, lf, regParam, (k < L ? 1.0 : 0.5) * dt, dt);
            if (k < L && (rc = mass_x_bound())) return rc;
        }
    }
    if ((rc = collect_pending(ctx))) return rc;
    hipLaunchKernelGGL(k_lf_mnorm, dim3(LFNB), dim3(256), 0, st, lf, regParam);
    hipLaunchKernelGGL(k_lf_mnorm_final, dim3(1), dim3(1), 0, st, lf, regParam);
    HIPCHK(hipMemcpyAsync(ctx->h_lfFlag, ctx->d_lfFlag, sizeof(int), hipMemcpyDeviceToHost, st));
    ctx->lfFlagPending = true;
    if (evalsOut) *evalsOut = evals;
    return 0;
}

// after a synchronisation: did a trajectory meet a non-finite model value?
static int leapfrog_flag(hmcmt_ctx* ctx) {
    if (!ctx->lfFlagPending) return 0;
    ctx->lfFlagPending = false;
    if (*(volatile int*)ctx->h_lfFlag) {
        *ctx->h_lfFlag = 0;
        ctx->ss.haveFwd = ctx->ss.haveAdj = false;
        ctx->err = "non-finite model value during the trajectory";
        return HMCMT_EBREAKDOWN;
    }
    return 0;
}

int hmcmt_leapfrog_device(hmcmt_ctx* ctx, double* d_m, double* d_p, double dt, int32_t L, double regParam,
                          double lnSigMin, double lnSigMax, int32_t start_grad, double* d_pred, double* d_misfit,
                          double* d_mnorm, int32_t* nfevals) {
    if (!ctx || !d_m || !d_p) return HMCMT_EINVAL;
    if (!ctx->havePrior) { ctx->err = "hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (L < 1 || !(dt > 0) || !(lnSigMax > lnSigMin)) { ctx->err = "need L >= 1, dt > 0, lnSigMax > lnSigMin"; return HMCMT_EINVAL; }
    if (start_grad < 0 || start_grad > 2) { ctx->err = "start_grad must be 0, 1 or 2"; return HMCMT_EINVAL; }
    if (start_grad != 0 && !ctx->lfHaveGrad) { ctx->err = "start_grad != 0 needs a previous trajectory on this context"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    int evals = 0;
    ctx->lfHaveGrad = false;
    int rc = leapfrog_core(ctx, d_m, d_p, dt, L, regParam, lnSigMin, lnSigMax, start_grad, d_pred, d_misfit, &evals);
    if (rc) return rc;
    if (d_mnorm) HIPCHK(hipMemcpyAsync(d_mnorm, ctx->d_lfScal, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipGetLastError());
    ctx->lfHaveGrad = true;
    if (nfevals) *nfevals = evals;
    return 0;
}

int hmcmt_leapfrog(hmcmt_ctx* ctx, const double* m0, const double* p0, double dt, int32_t L, double regParam,
                   double lnSigMin, double lnSigMax, double* m1, double* p1, double* pred, double* misfit,
                   double* mnorm, int32_t* nfevals) {
    if (!ctx || !m0 || !p0 || !m1 || !p1) return HMCMT_EINVAL;
    if (!ctx->havePrior) { ctx->err = "hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (L < 1 || !(dt > 0) || !(lnSigMax > lnSigMin)) { ctx->err = "need L >= 1, dt > 0, lnSigMax > lnSigMin"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(m0[i]) || !std::isfinite(p0[i])) { ctx->err = "non-finite model or momentum"; return HMCMT_EBREAKDOWN; }
    hipStream_t st = ctx->stream;
    std::memcpy(ctx->h_stage, m0, sizeof(double) * n);
    std::memcpy(ctx->h_stage + n, p0, sizeof(double) * n);
    HIPCHK(hipMemcpyAsync(ctx->d_mcur, ctx->h_stage, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->d_p, ctx->h_stage + n, sizeof(double) * n, hipMemcpyHostToDevice, st));
    int evals = 0, startGrad = 0;
    if (const hmcmt_ctx::Memo* e = ctx->opt.verify ? nullptr : memo_find(ctx, m0, true)) {
        // the gradient at the start model is known (end of the previous trajectory, or its start after a rejection)
        std::memcpy(ctx->h_stage + 2 * n, e->grad.data(), sizeof(double) * n);
        HIPCHK(hipMemcpyAsync(ctx->d_g, ctx->h_stage + 2 * n, sizeof(double) * n, hipMemcpyHostToDevice, st));
        ++ctx->memoHits;
        startGrad = 1;
    }
    ctx->lfHaveGrad = false;
    int rc = leapfrog_core(ctx, ctx->d_mcur, ctx->d_p, dt, L, regParam, lnSigMin, lnSigMax, startGrad, nullptr, nullptr, &evals);
    if (rc) return rc;
    double* hs = ctx->h_stage;
    HIPCHK(hipMemcpyAsync(hs, ctx->d_mcur, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs + n, ctx->d_p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs + 2 * n, ctx->v.pred, sizeof(cplx) * nData, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs + 2 * n + 2 * nData, ctx->d_misfit, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs + 2 * n + 2 * nData + 1, ctx->d_lfScal, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs + 2 * n + 2 * nData + 2, ctx->d_g, sizeof(double) * n, hipMemcpyDeviceToHost, st));   // for the memo
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    prof_collect(ctx);
    if ((rc = leapfrog_flag(ctx))) return rc;
    ctx->lfHaveGrad = true;
    memo_store(ctx, hs, hs + 2 * n, hs[2 * n + 2 * nData], hs + 2 * n + 2 * nData + 2);   // the end model's data gradient
    std::memcpy(m1, hs, sizeof(double) * n);
    std::memcpy(p1, hs + n, sizeof(double) * n);
    if (pred) std::memcpy(pred, hs + 2 * n, sizeof(cplx) * nData);
    if (misfit) *misfit = hs[2 * n + 2 * nData];
    if (mnorm) *mnorm = hs[2 * n + 2 * nData + 1];
    if (nfevals) *nfevals = evals;
    return 0;
}

#include "host_chain.h"
#include "host_map.h"

}  // extern "C"

#include "host_jacobian.h"
