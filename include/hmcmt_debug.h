/* hmcmt_debug.h -- instrumentation, introspection and test hooks of libhmcmt_hip.so (round 6: split off include/hmcmt.h, whose
 * entry points are the drop-in boundary of INTEGRATION.md section 1).  Nothing here is needed to run the hot path; the
 * measurement harness (bench.py), the profiling scripts and tests/ use it.  Same library, same calling conventions (return 0 or
 * a negative HMCMT_E* code).  Stability: fields of the out-arrays are only ever appended.
 * Replaces nothing in the reference: the reference's instrumentation is `@time` / `@elapsed` around proposeLeapfrog and the
 * chain (HMCSampler.jl:136, examples/dprism3d/runHMCscript.jl:26). */
#ifndef HMCMT_DEBUG_H
#define HMCMT_DEBUG_H

#include "hmcmt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel-time accounting with HIP events on the context's stream.
 * categories: 0 fdm-transform (MFMA), 1 tridiagonal, 2 stencil SpMV, 3 vector ops,
 *             4 assembly+boundary, 5 receivers+sources, 6 gradient accumulation */
#define HMCMT_NCAT 8
int hmcmt_profile(hmcmt_ctx* ctx, int32_t category_mask);     /* bit c enables category c; 0 = off; resets the counters */
int hmcmt_profile_every(hmcmt_ctx* ctx, int32_t n);           /* time only every n-th evaluation (event brackets cost ~20 % when always on) */
int hmcmt_profile_read(hmcmt_ctx* ctx, double* ms /*[HMCMT_NCAT]*/, int64_t* launches /*[HMCMT_NCAT]*/);
/* the per-launch bracket overhead (microseconds) hmcmt_profile calibrated -- a kernel that spins for a known time on the
 * device's wall clock, bracketed back to back -- and subtracts from every sampled launch */
int hmcmt_profile_overhead(const hmcmt_ctx* ctx, double* us);

/* What the sampled launches worked on (roofline numerators): out[0] = sum over the sampled iterations of the number of
 * systems still active (device counter, incremented by k_spmv_fused), out[1] = sum over the sampled solves of the systems
 * active at their start (the preconditioner is applied once before the first iteration), out[2] = evaluations sampled,
 * out[3] = solves sampled, out[4] = those of them that ran two smoothing sweeps per side (hmcmt_stats.smoother_sweeps).
 * out[5] = sum over the sampled solves of (iterations of the slowest system + 1): the serial length of the solves; out[6] = sampled
 * solves run by the persistent solve kernel (one launch per solve).  Reset by hmcmt_profile. */
int hmcmt_profile_counters(hmcmt_ctx* ctx, int64_t* out /*[7]*/);

/* sizes the roofline accounting needs: out = {NYP, NZP, S, ny, nz, zid, nblk} */
int hmcmt_dims(const hmcmt_ctx* ctx, int32_t* out);

/* Test hooks (exercise single kernels through the ABI).
 * hmcmt_debug_transform: C = A*V (which=0) or A*V' (which=1) with the context's FDM matrices (fp64 kernel);
 *   which=2/3: the mixed-precision kernels (bf16 operands, fp32 accumulation), same products;
 *   A, C: host complex[S*NZP*NYP] in the padded nodal layout.
 * hmcmt_debug_spmv: q = A_s p for all systems at the model of the last evaluation. */
int hmcmt_debug_transform(hmcmt_ctx* ctx, int32_t which, const double* A, double* C);
/* hmcmt_debug_flags (for the gradient pin, tests/test_gradient_pin.py): bit 0 -- the Dirichlet values of all four sides
 *   (mt2DTE.jl:100-134, mt2DTM.jl:100-134) are NOT recomputed from the model but stay those of the previous evaluation;
 *   bit 1 -- the boundary-derivative terms dBC^T w (compJacTMatVec.jl:237-242, :309-313, :316) are left out of the
 *   gradient.  A frozen-boundary finite difference of the misfit must then equal the gradient with bit 1 set.
 *   bit 2 (one-shot, not stored) -- the first system group of the NEXT persistent launch fails its placement check, as if its
 *   workgroups were not on one XCD (tests/test_gpu_persist.py: the other groups finish, the launch-per-phase loop takes the rest).
 *   bit 3 (one-shot) -- EVERY group of the next persistent launch fails it: the all-fallback regime of a device in another partition
 *   mode or a driver with another dispatch order (the whole evaluation then runs the launch-per-phase loop, one line on stderr).
 *   bits 8-15 (with bit 2) -- not the first group but the group of that index (xcd x slots per XCD + slot: the group that takes the
 *   systems xcd + 8 slot, ... -- hmcmt_persist_info) fails it.
 *   bit 4 (with bit 2 or 3) -- not the next persistent launch but the next ADJOINT one (forward launches pass the one-shot failure
 *   by): a misplaced group beside systems the adjoint solve has started and stalled (tests/test_gpu_persist.py).
 *   0 restores the product behaviour; stored results of earlier calls are dropped. */
int hmcmt_debug_flags(hmcmt_ctx* ctx, int32_t flags);
int hmcmt_debug_spmv(hmcmt_ctx* ctx, const double* p, double* q);
int hmcmt_debug_precond(hmcmt_ctx* ctx, const double* r, double* z);
int hmcmt_persist_envelope(int64_t ny, int64_t nz, int32_t cus_per_xcd, int64_t nsystems, int64_t* out6);   /* no device needed: would a mesh of ny x nz cells (nz incl. air
                                                             layers) run the one-launch-per-solve kernel on a device with cus_per_xcd CUs per XCD (MI355X: 32; a half / quarter CU
                                                             share: 16 / 8), and how: {column parts (0 = outside its envelope: the launch-per-phase loop), threads / 2, workgroups per
                                                             system, modes per slab, LDS bytes per workgroup, systems per XCD at a time} */
#define HMCMT_PERSIST_INFO_FIELDS 16
int hmcmt_persist_info(const hmcmt_ctx* ctx, int64_t* out, int32_t nout);  /* writes min(nout, HMCMT_PERSIST_INFO_FIELDS) values -- fields are only ever APPENDED, so a caller built against an
                                                                   older header passes its own count and gets the fields it knows --:
                                                                   {threads per strip (0: not applicable), workgroups per system, slots per XCD, enabled, solves, placement fallbacks,
                                                                   usable now (this context alone on its device in the process AND the process holds the device's advisory lock),
                                                                   modes per slab of its tridiagonal solves (32; 16 on tall meshes and with column parts),
                                                                   column parts per row block (1; 2 on meshes wider than one tile: the stress size),
                                                                   timed-out waits (each one: the evaluation redone with the launch-per-phase loop),
                                                                   CU share index, CU share count (hmcmt_next_cu_share),
                                                                   strips of tile rows per column (2: k_cocg_persist, 4: k_cocg_persist4; threads per workgroup = strips x threads per strip),
                                                                   why the kernel is off (0: it is not, or HMCMT_PERSIST=0; 1: a placement fallback, for good; 2: a timed-out wait, tried again later),
                                                                   the last placement fallback: kind of its launch (0 forward, 1 adjoint; -1: none yet),
                                                                   ... and the systems that launch had started itself and left active -- stalled, the host continues them from their
                                                                   own x and r -- (-1: a launch that did not form the residual itself, where they are not told apart)} */
int hmcmt_persist_order(const hmcmt_ctx* ctx, int32_t kind, int32_t* order, int64_t* rebalanced);   /* meshes whose systems take turns on the chip (more systems than 8 x
                                                             slots per XCD: cfg5): the order in which the persistent kernel's queues take the systems of a solve of
                                                             `kind` (0 forward, 1 adjoint) -- order[nsystems], position queue + queues * round -> system --, balanced from
                                                             the previous solve's iteration counts (HMCMT_PERSIST_BALANCE=0: never; the same systems, the same results);
                                                             *rebalanced = tables taken so far.  Either pointer may be NULL */
int hmcmt_persist_pack(const double* cost, int32_t nsystems, int32_t queues, int32_t* order, double* makespan);   /* no device needed: the packing behind
                                                             hmcmt_persist_order on the caller's costs -- nsystems systems onto `queues` queues that take turns (position
                                                             queue + queues * round), longest first into the least loaded queue that has room; order[nsystems] = system at
                                                             each position, *makespan = the largest queue sum (order NULL: that of the index order) */
int hmcmt_persist_width(const hmcmt_ctx* ctx, int32_t* width);   /* the compile-time row width (padded nodes: 112 / 208 / 416) of the width-specialised persistent
                                                                     kernel this context launches; 0: the generic kernel (HMCMT_PERSIST_WIDTHK=0 forces it) */
int hmcmt_debug_hog(hmcmt_ctx* ctx, int32_t nblocks, int32_t ms);   /* test hook: nblocks workgroups that each hold a CU's LDS for ms milliseconds on a stream of their own (a foreign tenant on the device); returns once they are resident, without waiting for them to end */
int hmcmt_debug_persist_precond(hmcmt_ctx* ctx, int32_t sweeps, const double* r, double* z);   /* the persistent solve kernel's preconditioner (tests) */
int hmcmt_debug_fdm_fwd(hmcmt_ctx* ctx, const double* t, double* out);   /* [2][S*vstride] complex: fused kernel | separate kernels */
int hmcmt_debug_back_post(hmcmt_ctx* ctx, const double* y, const double* r, double* out, double* sums);   /* out: [2][S*vstride] complex (fused | separate), sums[6] */

/* The mass matrix of hmcmt_set_mass: out = {kind, seconds the host took to factor Wm (0: not factored), bandwidth of Wm,
 * separable (1: Wm^-1 is the fast diagonalisation of the active box; 0: PCG), PCG iterations of the last Wm^-1 application
 * (0 on the direct path), box rows, box columns} */
#define HMCMT_MASS_INFO_FIELDS 7
int hmcmt_mass_info(const hmcmt_ctx* ctx, double* out /*[HMCMT_MASS_INFO_FIELDS]*/);

/* Measurement only: HIP-event pairs round every k_chain_acov launch of the running autocovariance accumulator (hmcmt_chain_acov_begin),
 * in place in the chain's commit.  ms[2], launches[2] (each may be NULL) receive the sums since the last switch; then enable = 1 / 0
 * switches on / off and zeroes the sums, enable = -1 leaves them (read only).  Of each pair [0] the commits in which some lag still fills its H_k (count < maxlag), [1] the
 * steady commits (count >= maxlag: every lag reads the ring and updates S_k).  An interval includes the cost of its two event records */
int hmcmt_debug_chain_acov_time(hmcmt_ctx* ctx, int32_t enable, double* ms /*[2]*/, int64_t* launches /*[2]*/);

/* Measurement only: the same for the running covariance accumulator (hmcmt_chain_cov_begin): of each pair [0] the k_chain_cov_commit
 * launches, [1] the k_chain_cov_flush launches (a read-out's flush of a partly filled batch included).  It changes no result */
int hmcmt_debug_chain_cov_time(hmcmt_ctx* ctx, int32_t enable, double* ms /*[2]*/, int64_t* launches /*[2]*/);

/* Test hooks of the initial-guess extrapolation (options.warm_start == 2; DESIGN 4.4, tests/test_gpu_extrap.py).  Read-only: they
 * wait for the context's streams and change no result.
 * hmcmt_debug_extrap: the extrapolation state of solve kind `kind` (0 forward, 1 adjoint) as the last evaluation left it,
 *   out = {w_0 .. w_5 (weights of x_k, x_{k-1}, ..., x_{k-5}), keep (1: the model was a repeat, nothing moved), count (models in the
 *   history after the call, <= 6), head of the field ring (5 slots), head of the model ring (7 slots)}.
 * hmcmt_debug_guess_capture: enable = 1 / 0 switches the capture of the initial guesses on / off.  While on, every evaluation that
 *   extrapolates copies X (and, with a gradient, Lam) device-to-device behind the extrapolation kernel, on that kernel's stream, into
 *   buffers allocated when the capture is first enabled; while off there is no launch, no copy and no allocation.
 * hmcmt_debug_guess: the captured guess of solve kind `kind`, the vector the last evaluation's solve started from: out = host
 *   complex[S*NZP*NYP] in the padded nodal layout of hmcmt_debug_spmv (system s = mode * nFreq + f, node iz * NYP + iy).  Defined on
 *   the interior nodes 1 <= iy <= ny-1, 1 <= iz <= nz-1 only: the forward solve's boundary nodes are written by the boundary-value
 *   kernel on another stream at the same time, so the copy may hold either their old or their new values.  On a cold start the
 *   guess is the zero fill.  An evaluation that does not extrapolate (warm_start != 2, options.verify) leaves the capture as it was. */
int hmcmt_debug_extrap(hmcmt_ctx* ctx, int32_t kind, double* out /*[10]*/);
int hmcmt_debug_guess_capture(hmcmt_ctx* ctx, int32_t enable);
int hmcmt_debug_guess(hmcmt_ctx* ctx, int32_t kind, double* out);

/* Test hook of the No-U-turn sampler's two kernels (k_nuts_leaf, k_nuts_final; tests/test_gpu_chain_nuts.py): one leaf's pass over n
 * cells on the caller's DEVICE vectors, so that the kernels are tested without a solve.  The context lends its device and stream only;
 * n need not be its nAC (1 <= n <= HMCMT_NUTS_HOOK_NMAX: the kernels index cells by int, one grid stride past n included).  backward / other_backward: the end stores its momentum (and x) negated.  x, x_other NULL: the diagonal inv_m.
 * first: rho_s = p, else rho_s += p.  ck_write: the three vectors (p, x, rho_s) of an even leaf's checkpoint, or NULLs.  ck_due[c]: the
 * c-th due checkpoint's three vectors, c < ndue <= HMCMT_NUTS_CK_MAX.  merged: rho_next = rho + rho_s and the merged tree's pair.
 * sums[HMCMT_NUTS_SUMS]: [0] p.x, [1] x.rho_next, [2] x_other.rho_next, [3 + 2c] x_ck.span, [4 + 2c] x.span; rows that are not due
 * are 0.  Complete on return. */
#define HMCMT_NUTS_CK_MAX 9
#define HMCMT_NUTS_SUMS 21
#define HMCMT_NUTS_HOOK_NMAX 0x40000000
typedef struct hmcmt_debug_nuts_args {
    int64_t n;
    int32_t backward, other_backward, first, merged, ndue, reserved_;
    const double *p, *x, *inv_m;
    double* rho_s;
    double* ck_write[3];
    const double* ck_due[HMCMT_NUTS_CK_MAX][3];
    const double* rho;
    double* rho_next;
    const double *p_other, *x_other;
} hmcmt_debug_nuts_args;
int hmcmt_debug_nuts_leaf(hmcmt_ctx* ctx, const hmcmt_debug_nuts_args* args, double* sums /*[HMCMT_NUTS_SUMS]*/);

/* Measurement only: the solver's work in the leaves of the chain's NUTS samples since the last reset, split by whether a leaf follows
 * a change of direction (its solves' extrapolated guesses then come from the other end's path).  out[4] (may be NULL) = {iterations,
 * solves of the leaves that follow a change; iterations, solves of the others}, forward and adjoint together; reset != 0 zeroes the
 * sums.  It changes no result */
int hmcmt_debug_nuts_iters(hmcmt_ctx* ctx, int64_t* out /*[4]*/, int32_t reset);

/* Test hooks of the low-rank mass adaptation (hmcmt_chain_adapt_lowrank; tests/test_gpu_chain_adapt_lowrank.py).
 * hmcmt_debug_adapt_lowrank runs the window end's kernels on rows the caller hands in, without a chain or a solve (the context needs
 * its prior: the rows have nAC cells): X, G [n][nAC] and invM [nAC] from the host, 4 <= n <= 128; K_out [2n][2n] = W W' (k_adapt_lr_mean,
 * k_adapt_lr_gram); with B [2n][r], 1 <= r <= HMCMT_MASS_RANK_MAX, also U_out [r][nAC] = B' W (k_adapt_lr_lift, then k_adapt_lr_sign);
 * B NULL or r = 0: the Gram matrix only.  Complete on return; nothing of the context changes.
 * hmcmt_debug_adapt_lowrank_rows reads the OPEN window's stores of a running upgraded adaptation: *n pairs, X and G [*n][nAC] (room for
 * max_samples rows each); while the open window holds none, the rows of the window that closed last, which stay in the stores until
 * the next pair.  HMCMT_EINVAL without such an adaptation. */
int hmcmt_debug_adapt_lowrank(hmcmt_ctx* ctx, int32_t n, const double* X, const double* G, const double* invM, double* K_out,
                              const double* B, int32_t r, double* U_out);
int hmcmt_debug_adapt_lowrank_rows(hmcmt_ctx* ctx, int32_t* n, double* X, double* G);
/* Measurement only: the last closed window end of a running upgraded adaptation.  out[4] = {ms of k_adapt_lr_mean + k_adapt_lr_gram,
 * ms of k_adapt_lr_lift + k_adapt_lr_sign (0 where no direction was lifted) -- HIP events on the context's stream --, host ms from the
 * first launch to K on the host (the window end's wait), host ms of the uploads, the lift and the orthonormality check with its wait}.
 * It changes no result */
int hmcmt_debug_adapt_lowrank_time(hmcmt_ctx* ctx, double* out /*[4]*/);

/* Test hook of the row sketch (hmcmt_chain_sketch_begin; tests/test_gpu_chain_sketch.py): feeds the n host rows[n][nAC] (1 <= n <=
 * 65536) as committed models through the chain's very commit and shrink launches, without a chain or a solve (the context needs its
 * prior: the rows have nAC cells); pivot as for hmcmt_chain_sketch_begin.  info and, each may be NULL, x0, tot, q [nAC] and
 * B_out [info->fill][nAC] (room for 2 ell rows) are the sketch behind the last row; of the first max_shrinks shrinks K_out
 * [max_shrinks][2 ell][2 ell] receives the Gram matrix and T_out [max_shrinks][ell][2 ell] the host's T (both needed with
 * max_shrinks > 0).  Complete on return; nothing of the context changes.  HMCMT_EBREAKDOWN where a shrink's eigensolver gave up. */
int hmcmt_debug_chain_sketch(hmcmt_ctx* ctx, int32_t ell, int64_t n, const double* rows, const double* pivot, hmcmt_sketch_info* info,
                             double* x0, double* tot, double* q, double* B_out, int32_t max_shrinks, double* K_out, double* T_out);
/* The three vectors the running sketch's mean and variance are made of: x0 (the pivot), tot (the sum of y) and q (the sum of y^2), nAC
 * doubles each (each may be NULL; device pointers with on_device).  sampler.pcaFromSketch and mergeSketches work from them.  A
 * read-out: nothing changes.  HMCMT_EINVAL without a sketch */
int hmcmt_debug_chain_sketch_sums(hmcmt_ctx* ctx, double* x0, double* tot, double* q, int32_t on_device);
/* Measurement only: the same as hmcmt_debug_chain_cov_time for the running sketch: of each pair [0] the k_chain_sketch_commit launches,
 * [1] the k_chain_sketch_gram and k_chain_sketch_shrink launches (two per shrink); *host_ms (may be NULL) the host milliseconds of
 * the shrinks' eigenproblems since the last switch.  It changes no result */
int hmcmt_debug_chain_sketch_time(hmcmt_ctx* ctx, int32_t enable, double* ms /*[2]*/, int64_t* launches /*[2]*/, double* host_ms);

/* Test hooks of the MAP optimiser (hmcmt_map_*; tests/test_gpu_map.py).  hmcmt_debug_map_direction runs the direction's three kernels
 * (k_map_project, k_map_coef, k_map_expand) on HOST vectors, without a run or a solve: the context lends its device and stream only, n
 * need not be its nAC (1 <= n <= HMCMT_MAP_HOOK_NMAX).  The ring: history slots, rows [2 history][n] (row k the s of slot k, row
 * history + k its y), pair i of count, oldest first, in slot (head + i) % history; sy, yy [history][history] = S'Y and Y'Y by slot
 * (rows, sy, yy may be NULL with count = 0).  Outputs (each may be NULL): pg, d, mt [n]; sums [HMCMT_MAP_SUMS] = the coefficient block
 * {gamma, flag "not a descent direction", g'd, |pg|inf, |pg|2^2, |B|, pairs used, 0, a [32], w = -gamma p [32]}, then the 2 count
 * projections S'pg, Y'pg (0 beyond).  Complete on return; nothing of the context changes.
 * hmcmt_debug_map_rows reads a live run: info [4] = {history, head, count, iterations}; rows [2 history][nAC], sy, yy
 * [history][history] (each may be NULL).  HMCMT_EINVAL without a run. */
#define HMCMT_MAP_HOOK_NMAX 0x40000000
#define HMCMT_MAP_SUMS 136
typedef struct hmcmt_debug_map_args {
    int64_t n;
    int32_t history, head, count, reserved_;
    const double *rows, *sy, *yy, *m, *g;
    double lo, hi, alpha;
    double *pg, *d, *mt, *sums;
} hmcmt_debug_map_args;
int hmcmt_debug_map_direction(hmcmt_ctx* ctx, const hmcmt_debug_map_args* args);
int hmcmt_debug_map_rows(hmcmt_ctx* ctx, int32_t* info /*[4]*/, double* rows, double* sy, double* yy);

#ifdef __cplusplus
}
#endif
#endif /* HMCMT_DEBUG_H */
