// host_jacobian.h -- the calls that borrow the context, solve, and give it back: the explicit Jacobian (kernels_jac.h) and the
// matrix-free Jacobian products of one direction or a block of them (kernels_jvp.h).  Host code of hmcmt_hip.hip's translation
// unit, included at its end: behind the context, solve() and evaluate().
//
// All of them run between one bracket (Borrowed) and through one solve loop (borrowed_solve); DESIGN.md 4.6-4.8.

// ----------------------------------------------------------------------------------------------
// what the family shares
// ----------------------------------------------------------------------------------------------
// The bracket of a call that borrows the context.  Everything the call's evaluation and solves move in the host solve state --
// hmcmt_ctx::SolveState, and View, Solver, options and statistics whole -- is saved in front and put back behind, on every way
// out, so the context's next evaluation computes what it would have.  The configuration needs no saving: hmcmt_ctx::cfg is const (a
// block call's instance without sync words is seen by persist_fits, not written into it).  What remains loose in the context --
// resources, counters, the per-evaluation protocol flags -- is left alone or reset below.  `st` collects the call's own
// statistics for the caller.
struct Borrowed {
    hmcmt_ctx* const ctx;
    hmcmt_stats* const stOut;
    hmcmt_stats st{};
    hmcmt_ctx::SolveState ss;
    const View v; const Solver sv; const hmcmt_options opt; const hmcmt_stats stats;
    const long long timeouts, fallbacks;
    Borrowed(hmcmt_ctx* c, hmcmt_stats* out)
        : ctx(c), stOut(out), ss(c->ss), v(c->v), sv(c->sv), opt(c->opt), stats(c->stats), timeouts(c->persistTimeouts), fallbacks(c->persistFallbacks) {
        // no guard, no sampled profiling, no test hooks, no leapfrog update in the call's evaluation and solves
        c->ss.guardEvery = 0; c->ss.profMask = 0; c->ss.dbgFlags = 0;
        c->ss.lfStep.on = 0; c->ss.lfMom.on = 0;
        c->sv.cntActive = nullptr;
        c->stats = hmcmt_stats{};
    }
    Borrowed(const Borrowed&) = delete;
    ~Borrowed() {
        hmcmt_ctx* c = ctx;
        const std::string e = c->err;
        (void)hipStreamSynchronize(c->stream);
        // the persistent kernel's backoff after a timed-out wait counts the context's own solves: the call's do not count.  A timeout
        // or placement failure DURING the call is an event of the device, not of the call: its state (kernel off, a new backoff) stays
        if (c->persistTimeouts != timeouts || c->persistFallbacks != fallbacks) {
            ss.persistOn = c->ss.persistOn; ss.persistWhyOff = c->ss.persistWhyOff; ss.persistBackoff = c->ss.persistBackoff;
        }
        c->ss = std::move(ss);
        c->v = v; c->sv = sv; c->opt = opt; c->stats = stats;
        c->psStart = hmcmt_ctx::PsStart{};
        c->solveBegun = c->preDone = false;
        c->specValid = false; c->solveFail = 0; c->lpFallback = false;
        c->err = e;
        if (stOut) *stOut = st;
    }
};

// the context's View for kernels launched outside an evaluation, at model `m`: no gate, no stamps, no test hooks
static View quiet_view(const hmcmt_ctx* ctx, const double* m) {
    View vj = ctx->v;
    vj.m = m; vj.gate = nullptr; vj.ticks = nullptr; vj.dbg = 0;
    return vj;
}
// ... with the adjoint solution, right-hand side and boundary-weight arrays `a` and the residual r
static void adjoint_arrays(View& vj, const hmcmt_ctx::AdjArrays& a, cplx* r) {
    vj.Lam = a.lam; vj.R = r; vj.srcB = a.srcB; vj.wL = a.wL; vj.wR = a.wR; vj.colw = a.colw; vj.gL = a.gL; vj.gR = a.gR;
}
// ... with the products' work arrays `w`; J v goes to `jv` where it is the call's result
static View product_view(const hmcmt_ctx* ctx, const hmcmt_ctx::ProdArrays& w, cplx* jv) {
    View vj = quiet_view(ctx, ctx->jvp.m);
    vj.dSig = w.dSig; vj.dbcL = w.dbcL; vj.dbcR = w.dbcR; vj.dbcB = w.dbcB;
    vj.vbar = w.vbar; vj.rxCoef = w.rxCoef; vj.qPart = w.qPart; vj.gPartG = w.gPartG;
    vj.jv = jv ? jv : w.jv;
    vj.tanV = w.vin; vj.uData = w.u; vj.tanScale = w.scale;
    return vj;
}

// behind a cold forward evaluation, what the gradient's side stream and k_rxall(wantGrad) provide: the boundary-derivative
// tables and the receiver functionals
static void launch_post_forward(hmcmt_ctx* ctx, const View& vj) {
    hipStream_t strm = ctx->stream;
    const int S = vj.S;
    hipLaunchKernelGGL(k_sens_layers, dim3((vj.nz + 1 + 63) / 64, 3, S), dim3(64), 0, strm, vj);
    hipLaunchKernelGGL(k_sens_profile, dim3((3 * S + 63) / 64), dim3(64), 0, strm, vj);
    hipLaunchKernelGGL(k_bcsens_pre, dim3((vj.nz + 63) / 64, 3, S), dim3(64), 0, strm, vj);
    hipLaunchKernelGGL(k_rx, grid1(S * vj.nRx, 64), dim3(64), 0, strm, vj, 1);
}

// sweeps per side of the family's solves (cold: well above the two-sweep threshold)
static int cold_sweeps(const hmcmt_ctx* ctx) { return (ctx->cfg.sweepsMode == 1 || !sweeps2_ok(ctx)) ? 1 : 2; }

static int model_finite(hmcmt_ctx* ctx, const double* m) {
    for (int i = 0; i < ctx->v.nAC; ++i)
        if (!std::isfinite(m[i])) { ctx->err = "non-finite model value"; return HMCMT_EBREAKDOWN; }
    return 0;
}

// the argument checks of the family's entry points (`family` starts the message, `input` names the first pointer)
static int family_check(hmcmt_ctx* ctx, const char* family, const char* input, const void* in, const void* out, int32_t wrt) {
    const std::string f = family;
    if (!in || !out) { ctx->err = f + ": null " + input + " or output pointer"; return HMCMT_EINVAL; }
    if (wrt != HMCMT_JAC_WRT_SIGMA && wrt != HMCMT_JAC_WRT_LNSIGMA) { ctx->err = f + ": wrt must be HMCMT_JAC_WRT_SIGMA or HMCMT_JAC_WRT_LNSIGMA"; return HMCMT_EINVAL; }
    if (ctx->statsPending) { ctx->err = f + ": an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    return 0;
}

// the records k_solve_end left for solve kind `kind` (the caller has synchronised) -> totals of the Jacobian's statistics
static void jac_records(hmcmt_ctx* ctx, int kind, const int* on, hmcmt_stats& st) {
    const int S = ctx->v.S;
    const int* it = reinterpret_cast<const int*>(ctx->inst.h_rec);
    const int* status = it + 2 * S;
    const double* err = ctx->inst.h_rec + 2 * S;
    for (int s = 0; s < S; ++s) {
        if (!on[s]) continue;
        const int n = it[kind * S + s];
        if (kind == 0) { st.iters_fwd_max = std::max(st.iters_fwd_max, n); st.iters_fwd_sum += n; }
        else { st.iters_adj_max = std::max(st.iters_adj_max, n); st.iters_adj_sum += n; }
        st.err_est_max = std::max(st.err_est_max, err[kind * S + s]);
        if (status[kind * S + s] != 0 && st.status == 0) st.status = status[kind * S + s];
    }
}

// One solve of the family, into x from a zero guess: `fill` writes the right-hand side (again after a timed-out persistent launch,
// which destroys it; its argument: the persistent kernel starts the solve, so the residual needs no clearing); sparseRow >= 0: the
// adjoint's sparse start on node rows sparseRow, sparseRow + 1 there.  `on`: [ctx->v.S] the systems solved.  A solve that ended
// clean has its records read here behind a synchronisation -- or, with recordsLater, by the caller behind its own (jac_records);
// one that did not is the error "<subject> solve broke down / did not converge".
template <class Fill>
static int borrowed_solve(hmcmt_ctx* ctx, cplx* x, int kind, int sweeps, int sparseRow, const Fill& fill, hmcmt_stats& st, const int* on,
                          const char* subject, bool recordsLater = false) {
    hipStream_t strm = ctx->stream;
    const size_t vecBytes = (size_t)ctx->v.S * ctx->v.vstride * sizeof(cplx);
    for (int attempt = 0;; ++attempt) {
        HIPCHK(hipMemsetAsync(x, 0, vecBytes, strm));
        const bool inKernelStart = ctx->cfg.psInKernelStart && ctx->opt.precond == HMCMT_PRECOND_FDM_JACOBI && ctx->opt.fdm_precision == 0 &&
                                   !ctx->opt.verify && persist_ok(ctx);
        fill(inKernelStart);
        ctx->sv.sweeps = sweeps;
        ctx->preDone = false;
        if (inKernelStart) { ctx->psStart.resid = sparseRow >= 0 ? 2 + sparseRow : 0; ctx->psStart.begin = 1; ctx->solveBegun = true; }
        else ctx->solveBegun = false;
        ctx->guardNow = false;
        ctx->persistTimedOut = false;
        const int fb0 = ctx->stats.fallback_solves;
        int rc = solve(ctx, x, kind);
        if (rc) return rc;
        if (ctx->persistTimedOut && attempt == 0) {
            // (a wait of the persistent kernel timed out: the context is on the launch-per-phase loop now -- the solve again, there)
            ctx->persistTimedOut = false;
            (void)hipStreamSynchronize(strm); (void)hipGetLastError();
            ctx->solveFail = 0; host_word(ctx, HW_FAIL) = 0;
            ctx->stats.fallback_solves = fb0;
            continue;
        }
        if (ctx->stats.fallback_solves > fb0) ++st.fallback_solves;
        break;
    }
    const bool failed = ctx->solveFail || !ctx->ss.solveDone[kind];
    if (recordsLater && !failed) return 0;
    HIPCHK(hipStreamSynchronize(strm));
    jac_records(ctx, kind, on, st);
    if (failed) {
        if (st.status == 0) st.status = ctx->solveFail ? ctx->solveFail : HMCMT_ENOCONV;
        ctx->err = std::string(subject) + (st.status == HMCMT_EBREAKDOWN ? " solve broke down" : " solve did not converge");
        return st.status == HMCMT_EBREAKDOWN ? HMCMT_EBREAKDOWN : HMCMT_ENOCONV;
    }
    return 0;
}

// ----------------------------------------------------------------------------------------------
// explicit Jacobian (kernels_jac.h): batches by receiver -- receiver j in every system is the shape and right-hand-side sparsity of
// the gradient's adjoint solve, so every batch is one solve of the adjoint kind with the in-kernel sparse start and the same
// fallbacks.  The forward fields come from a cold evaluate() at the model; the bracket puts back what that evaluation and the batch
// solves move in the host state, and the call itself saves and puts back the warm-start fields and the extrapolation state.
// ----------------------------------------------------------------------------------------------
static int jac_alloc(hmcmt_ctx* ctx) {
    hmcmt_ctx::Jac& J = ctx->jac;
    if (J.ready) return 0;
    const View& v = ctx->v;
    const int S = v.S;
    const size_t vec = (size_t)S * v.vstride;
    std::vector<int> perRx(v.nRx, 0);
    for (int p = 0; p < v.nData; ++p) ++perRx[ctx->hp.datRx[p]];
    J.maxRows = std::max(1, *std::max_element(perRx.begin(), perRx.end()));
    int rc = 0;
    if ((rc = dalloc(ctx, &J.lam, vec)) || (rc = dalloc(ctx, &J.xSave, vec, false)) || (rc = dalloc(ctx, &J.srcB, (size_t)S * 4)) ||
        (rc = dalloc(ctx, &J.wL, (size_t)S * v.nz)) || (rc = dalloc(ctx, &J.wR, (size_t)S * v.nz)) || (rc = dalloc(ctx, &J.colw, (size_t)S * v.ny)) ||
        (rc = dalloc(ctx, &J.gL, (size_t)S * v.nz)) || (rc = dalloc(ctx, &J.gR, (size_t)S * v.nz)) || (rc = dalloc(ctx, &J.qJ, (size_t)S * v.ny)) ||
        (rc = dalloc(ctx, &J.pred, (size_t)v.nData)) || (rc = dalloc(ctx, &J.extSave, (size_t)EXT_LEN, false)) || (rc = dalloc(ctx, &J.misfit, 1)) ||
        (rc = dalloc(ctx, &J.m, (size_t)v.nAC)) || (rc = dalloc(ctx, &J.sens, (size_t)v.nAC)) ||
        (rc = dalloc(ctx, &J.rows, (size_t)J.maxRows * v.nAC * 2)) || (rc = dalloc(ctx, &J.list, (size_t)v.nData)) ||
        (rc = dalloc(ctx, &J.groups, (size_t)v.nData)) ||
        (rc = dalloc(ctx, &J.sysOn, (size_t)v.nRx * S)))
        return rc;
    HIPCHK(hipHostMalloc((void**)&J.h_rows, sizeof(double) * (size_t)J.maxRows * v.nAC * 2));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    J.ready = true;
    return 0;
}

// rows [row0, row0 + nrows) of J (hostJ: host memory, else device memory; null: the sensitivity into ctx->jac.sens instead)
static int jac_run(hmcmt_ctx* ctx, const double* d_m, int64_t row0, int64_t nrows, int wrt, double* outJ, bool hostJ, bool sens,
                   hmcmt_stats* stOut) {
    hmcmt_ctx::Jac& J = ctx->jac;
    const View& v0 = ctx->v;
    const int S = v0.S, nAC = v0.nAC, nRx = v0.nRx;
    const bool cplxOut = !ctx->hp.rhoPhase;             // (the two data families cannot be mixed; TZY rows are complex too)
    const int width = cplxOut ? 2 : 1;
    // the batches: the receivers of the rows, in receiver order; per batch the data (in data order) and the systems they need
    std::vector<std::vector<JacEntry>> lists(nRx);
    std::vector<int> on((size_t)nRx * S, 0);
    for (int64_t p = row0; p < row0 + nrows; ++p) {
        const int j = ctx->hp.datRx[p], s = ctx->hp.datSys[p];
        lists[j].push_back(JacEntry{(int)p, 0, s, ctx->hp.datKind[p]});
        on[(size_t)j * S + s] = 1;
    }
    // (within a batch the data are grouped by system, in data order inside a group: one dZ row per system, JacGroup)
    std::vector<JacEntry> flat;
    std::vector<JacGroup> groups;
    std::vector<int> gfirst(nRx, 0), ngroups(nRx, 0);
    for (int j = 0; j < nRx; ++j) {
        std::stable_sort(lists[j].begin(), lists[j].end(), [](const JacEntry& x, const JacEntry& y) { return x.s < y.s; });
        gfirst[j] = (int)groups.size();
        for (size_t q = 0; q < lists[j].size(); ++q) {
            JacEntry e = lists[j][q];
            e.row = hostJ ? (int)q : (int)(e.p - row0);      // (host: the batch's compact staging rows)
            if (q == 0 || e.s != lists[j][q - 1].s) groups.push_back(JacGroup{(int)flat.size(), 0});
            ++groups.back().count;
            flat.push_back(e);
        }
        ngroups[j] = (int)groups.size() - gfirst[j];
    }
    if (flat.empty()) { if (stOut) { *stOut = hmcmt_stats{}; stOut->nsystems = S; } return 0; }
    hipStream_t strm = ctx->stream;
    HIPCHK(hipMemcpyAsync(J.list, flat.data(), sizeof(JacEntry) * flat.size(), hipMemcpyHostToDevice, strm));
    HIPCHK(hipMemcpyAsync(J.sysOn, on.data(), sizeof(int) * on.size(), hipMemcpyHostToDevice, strm));
    HIPCHK(hipMemcpyAsync(J.groups, groups.data(), sizeof(JacGroup) * groups.size(), hipMemcpyHostToDevice, strm));
    HIPCHK(hipStreamSynchronize(strm));                  // (host vectors: the copies are complete before they go out of scope)
    const size_t vecBytes = (size_t)S * v0.vstride * sizeof(cplx);

    Borrowed b(ctx, stOut);
    hmcmt_stats& st = b.st;
    st.nsystems = S;
    // the context's forward fields and extrapolation state: the Jacobian's cold forward evaluation overwrites them
    HIPCHK(hipMemcpyAsync(J.xSave, v0.X, vecBytes, hipMemcpyDeviceToDevice, strm));
    HIPCHK(hipMemcpyAsync(J.extSave, ctx->d_ext[0], sizeof(double) * EXT_LEN, hipMemcpyDeviceToDevice, strm));
    AtExit fieldsBack([&] {
        (void)hipMemcpyAsync(ctx->v.X, J.xSave, vecBytes, hipMemcpyDeviceToDevice, strm);
        (void)hipMemcpyAsync(ctx->d_ext[0], J.extSave, sizeof(double) * EXT_LEN, hipMemcpyDeviceToDevice, strm);
    });

    // 1. forward fields at the model: a cold forward evaluation
    ctx->opt.warm_start = 0;
    int rc = evaluate(ctx, d_m, false, reinterpret_cast<double*>(J.pred), J.misfit, nullptr);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(strm));
    jac_records(ctx, 0, ctx->hp.sysOn.data(), st);
    if (st.status) { ctx->err = st.status == HMCMT_EBREAKDOWN ? "Jacobian: the forward solve broke down" : "Jacobian: the forward solve did not converge"; return st.status; }
    // 2. the boundary-derivative tables and the receiver functionals
    View vj = quiet_view(ctx, d_m);
    launch_post_forward(ctx, vj);
    adjoint_arrays(vj, J, ctx->sv.r);
    if (sens) HIPCHK(hipMemsetAsync(J.sens, 0, sizeof(double) * nAC, strm));
    const int sweeps = cold_sweeps(ctx);
    ctx->stats.smoother_sweeps = 0;
    const int nsrc = (2 * (v0.ny + 1) + 127) / 128;
    // 3. one batch per receiver
    for (int j = 0; j < nRx; ++j) {
        const int n = (int)lists[j].size();
        if (n == 0) continue;
        const int* onj = on.data() + (size_t)j * S;
        vj.sysOn = J.sysOn + (size_t)j * S;
        ctx->v.sysOn = vj.sysOn;
        ctx->ss.nSysOn = (int)std::count(onj, onj + S, 1);
        auto fill = [&](bool sparse) {
            if (!sparse) (void)hipMemsetAsync(vj.R, 0, vecBytes, strm);       // (the whole right-hand side is the residual)
            hipLaunchKernelGGL(k_jac_src, dim3(nsrc + (v0.ny + 127) / 128, S), dim3(128), 0, strm, vj, j, J.qJ, nsrc);
        };
        // (the records of a batch that ended clean: behind the batch's one synchronisation, below)
        if ((rc = borrowed_solve(ctx, J.lam, 1, sweeps, v0.zid, fill, st, onj, "Jacobian: an adjoint", true))) return rc;
        // (the products' kernels, one direction)
        hipLaunchKernelGGL(k_dir_wb, dim3((v0.nz + v0.ny + 127) / 128, S), dim3(128), 0, strm, vj, 1);
        hipLaunchKernelGGL(k_contract<1>, dim3((BCC_L * v0.nz + 127) / 128, 2, S), dim3(128), 0, strm, vj, 1);
        const JacGroup* gl = J.groups + gfirst[j];
        const dim3 ga((nAC + 127) / 128);
        if (sens) hipLaunchKernelGGL(k_jac_sens, ga, dim3(128), 0, strm, vj, J.list, gl, ngroups[j], j, J.qJ, wrt, J.sens);
        else hipLaunchKernelGGL(k_jac_rows, dim3(ga.x, ngroups[j]), dim3(128), 0, strm, vj, J.list, gl, j, J.qJ, wrt, cplxOut ? 1 : 0, hostJ ? J.rows : outJ);
        if (!sens && hostJ) HIPCHK(hipMemcpyAsync(J.h_rows, J.rows, sizeof(double) * (size_t)n * nAC * width, hipMemcpyDeviceToHost, strm));
        HIPCHK(hipStreamSynchronize(strm));
        jac_records(ctx, 1, onj, st);
        if (!sens && hostJ)
            for (int q = 0; q < n; ++q)
                std::memcpy(outJ + (size_t)(lists[j][q].p - row0) * nAC * width, J.h_rows + (size_t)q * nAC * width, sizeof(double) * nAC * width);
    }
    if (sens) hipLaunchKernelGGL(k_jac_sens_final, dim3((nAC + 127) / 128), dim3(128), 0, strm, J.sens, nAC);
    HIPCHK(hipGetLastError());
    st.smoother_sweeps = 10 * ctx->ss.sweepsUsed[0] + sweeps;
    return 0;
}

static int jac_check(hmcmt_ctx* ctx, const void* m, int64_t row0, int64_t nrows, int32_t wrt, const void* out) {
    if (int rc = family_check(ctx, "Jacobian", "model", m, out, wrt)) return rc;
    if (row0 < 0 || nrows < 0 || row0 > ctx->v.nData || nrows > ctx->v.nData - row0) { ctx->err = "Jacobian: row range outside [0, nData]"; return HMCMT_EINVAL; }
    return 0;
}

extern "C" {
int hmcmt_jacobian_device(hmcmt_ctx* ctx, const double* d_m, int64_t row0, int64_t nrows, int32_t wrt, double* d_J, hmcmt_stats* st) {
    if (!ctx) return HMCMT_EINVAL;
    if (int rc = jac_check(ctx, d_m, row0, nrows, wrt, d_J)) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (int rc = jac_alloc(ctx)) return rc;
    return jac_run(ctx, d_m, row0, nrows, wrt, d_J, false, false, st);
}

int hmcmt_jacobian(hmcmt_ctx* ctx, const double* m, int64_t row0, int64_t nrows, int32_t wrt, double* J, hmcmt_stats* st) {
    if (!ctx) return HMCMT_EINVAL;
    if (int rc = jac_check(ctx, m, row0, nrows, wrt, J)) return rc;
    if (int rc = model_finite(ctx, m)) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (int rc = jac_alloc(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->jac.m, m, sizeof(double) * ctx->v.nAC, hipMemcpyHostToDevice, ctx->stream));
    return jac_run(ctx, ctx->jac.m, row0, nrows, wrt, J, true, false, st);
}

int hmcmt_sensitivity(hmcmt_ctx* ctx, const double* m, int32_t wrt, double* sens, hmcmt_stats* st) {
    if (!ctx) return HMCMT_EINVAL;
    if (int rc = jac_check(ctx, m, 0, ctx->v.nData, wrt, sens)) return rc;
    if (int rc = model_finite(ctx, m)) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (int rc = jac_alloc(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->jac.m, m, sizeof(double) * ctx->v.nAC, hipMemcpyHostToDevice, ctx->stream));
    int rc = jac_run(ctx, ctx->jac.m, 0, ctx->v.nData, wrt, nullptr, false, true, st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(sens, ctx->jac.sens, sizeof(double) * ctx->v.nAC, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------
// matrix-free Jacobian products (kernels_jvp.h).  hmcmt_linearize is an ordinary cold forward evaluation plus what the gradient
// computes in front of its adjoint solve (boundary-derivative tables, receiver functionals); a product of nvec directions is small
// launches around ONE solve per route -- forward kind for the tangent fields (dense right-hand sides, zero guess), adjoint kind for
// J^T U (the gradient's sparse start) -- inside the bracket (Borrowed).  A product runs no evaluation: the context's fields, history
// and memo are not touched at all.
//   nvec = 1  the solve is the context's own, of its S systems with the problem's own flags, on the work arrays of hmcmt_ctx::Jvp
//             and the explicit Jacobian's solution and boundary arrays (hmcmt_ctx::Jac).
//   nvec > 1  the solve is over the nvec * S virtual systems, on a second solver instance (hmcmt_ctx::Blk): the context's Solver
//             with S and nFreq multiplied by nvec, the frequency list and the inverse pivots repeated per direction, per-system
//             arrays, sync words, reduction records, constant block and host records of its own (hmcmt_ctx::Inst); the stencil
//             coefficients and eigen-transforms are per mode and shared.  It is put in the context's place for the call (inside the
//             bracket, blk_enter), so solve(), the kernel table and the fallbacks see an ordinary problem.  The flags of the virtual
//             systems -- (direction not identically zero) and (system carries data) -- are made on the device and read back.
// ----------------------------------------------------------------------------------------------
static int jvp_alloc(hmcmt_ctx* ctx) {
    if (int rc = jac_alloc(ctx)) return rc;
    hmcmt_ctx::Jvp& P = ctx->jvp;
    if (P.ready) return 0;
    const View& v = ctx->v;
    const size_t S = (size_t)v.S;
    int rc = 0;
    if ((rc = dalloc(ctx, &P.m, (size_t)v.nAC)) || (rc = dalloc(ctx, &P.vin, (size_t)v.nAC)) || (rc = dalloc(ctx, &P.dSig, (size_t)v.nCell)) ||
        (rc = dalloc(ctx, &P.out, (size_t)v.nAC)) || (rc = dalloc(ctx, &P.gPartG, (size_t)2 * GRAD_NG * v.nCell)) ||
        (rc = dalloc(ctx, &P.qPart, S * v.ny)) || (rc = dalloc(ctx, &P.misfit, 1)) || (rc = dalloc(ctx, &P.scale, 4)) ||
        (rc = dalloc(ctx, &P.dbcL, S * v.nz)) || (rc = dalloc(ctx, &P.dbcR, S * v.nz)) || (rc = dalloc(ctx, &P.dbcB, S * (v.ny + 1))) ||
        (rc = dalloc(ctx, &P.jv, (size_t)v.nData)) || (rc = dalloc(ctx, &P.u, (size_t)v.nData)) || (rc = dalloc(ctx, &P.vbar, (size_t)v.nData)) ||
        (rc = dalloc(ctx, &P.rxCoef, S * v.nRx)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    P.ready = true;
    return 0;
}

static int linearize_run(hmcmt_ctx* ctx) {
    hmcmt_ctx::Jvp& P = ctx->jvp;
    hipStream_t strm = ctx->stream;
    P.valid = false;
    ctx->ss.haveFwd = false;                                // (always from a zero guess: the warm-start history starts again here)
    int rc = evaluate(ctx, P.m, false, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if ((rc = collect_stats(ctx, false))) return rc;     // (includes the stream synchronisation)
    prof_collect(ctx);
    if ((rc = finish_status(ctx))) return rc;
    launch_post_forward(ctx, quiet_view(ctx, P.m));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(strm));
    P.valid = true;
    ++P.gen;
    return 0;
}

static int linearize_check(hmcmt_ctx* ctx, const void* m) {
    if (!m) { ctx->err = "linearize: null model pointer"; return HMCMT_EINVAL; }
    if (ctx->statsPending) { ctx->err = "linearize: an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    return 0;
}

static int prod_check(hmcmt_ctx* ctx, const void* in, int32_t wrt, const void* out) {
    if (int rc = family_check(ctx, "Jacobian product", "input", in, out, wrt)) return rc;
    if (!ctx->jvp.ready || !ctx->jvp.valid) {
        ctx->err = "Jacobian product: no valid linearisation point (call hmcmt_linearize; every evaluating call and hmcmt_set_options ends it)";
        return HMCMT_EINVAL;
    }
    return 0;
}

extern "C" {
int hmcmt_linearize(hmcmt_ctx* ctx, const double* m) {
    if (!ctx) return HMCMT_EINVAL;
    if (int rc = linearize_check(ctx, m)) return rc;
    if (int rc = model_finite(ctx, m)) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (int rc = jvp_alloc(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->jvp.m, m, sizeof(double) * ctx->v.nAC, hipMemcpyHostToDevice, ctx->stream));
    return linearize_run(ctx);
}
int hmcmt_linearize_device(hmcmt_ctx* ctx, const double* d_m) {
    if (!ctx) return HMCMT_EINVAL;
    if (int rc = linearize_check(ctx, d_m)) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (int rc = jvp_alloc(ctx)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->jvp.m, d_m, sizeof(double) * ctx->v.nAC, hipMemcpyDeviceToDevice, ctx->stream));
    return linearize_run(ctx);
}
}  // extern "C"

// ----------------------------------------------------------------------------------------------
// the second solver instance of products of nvec > 1 directions
// ----------------------------------------------------------------------------------------------
static void blk_release(hmcmt_ctx* ctx) {
    hmcmt_ctx::Blk& B = ctx->blk;
    for (void* p : B.allocs) hipFree(p);
    for (void* p : B.hostAllocs) hipHostFree(p);
    B = hmcmt_ctx::Blk{};
}
static int blk_dalloc(hmcmt_ctx* ctx, void** p, size_t bytes) {       // (zeroed, on the block instance's own list)
    void* q = nullptr;
    bytes = std::max<size_t>(bytes, 16);
    HIPCHK(hipMalloc(&q, bytes));
    ctx->blk.allocs.push_back(q);
    HIPCHK(hipMemsetAsync(q, 0, bytes, ctx->stream));
    *p = q;
    return 0;
}
static int blk_alloc_impl(hmcmt_ctx* ctx, int nvec) {
    hmcmt_ctx::Blk& B = ctx->blk;
    const View& v = ctx->v;
    const size_t K = (size_t)nvec, S = (size_t)v.S, SV = K * S, VS = (size_t)v.vstride;
    Solver& k = B.sv;
    k = ctx->sv;                                         // (tile shapes, launch-invariant pointers, the per-mode coefficients)
    k.S = (int)SV; k.nFreq = nvec * v.nFreq;
    k.cntActive = nullptr;
    int rc = 0;
#define BA(ptr, n) { void* q_ = nullptr; if ((rc = blk_dalloc(ctx, &q_, (size_t)(n) * sizeof(*(ptr))))) return rc; (ptr) = reinterpret_cast<decltype(ptr)>(q_); }
    BA(B.omega, SV) BA(B.invp, SV * VS) BA(B.inst.d_invp32, SV * VS) BA(B.lam, SV * VS) BA(k.r, SV * VS) BA(B.inst.d_b, SV * VS) BA(B.inst.d_sw, SV * VS)
    BA(k.p, SV * VS) BA(k.q, SV * VS) BA(k.z, SV * VS) BA(k.y, SV * VS) BA(k.t, SV * VS) BA(k.dinv, SV * VS)
    BA(k.t32, SV * VS + 64) BA(k.y32, SV * VS + 64)
    BA(k.z32, SV * VS) BA(k.p32a, SV * VS) BA(k.p32b, SV * VS) BA(k.zs32, SV * VS) BA(k.z4_32, SV * VS) BA(k.t2_32, SV * VS) BA(k.partR, SV * MAXNB) BA(k.dinv32, SV * VS)
    BA(k.p2, SV * VS) BA(k.r2, SV * VS) BA(k.partPQ, SV * MAXNB) BA(k.rho2, 2 * SV)
    BA(k.partA, SV * MAXNB) BA(k.partB, SV * MAXNB) BA(B.inst.d_partZZ, SV * MAXNB) BA(B.inst.d_partRes, SV * MAXNB) BA(B.inst.d_partBn, SV * MAXNB)
    BA(k.rho, SV) BA(k.alphaBeta, SV) BA(k.active, SV) BA(k.iters, SV) BA(k.status, SV) BA(k.nactive, 1) BA(k.errEst, SV) BA(k.errRef, SV) BA(k.errRefIt, SV)
    BA(B.dirOn, K) BA(B.sysOnDir, SV) BA(B.sysOnV, SV)
    BA(B.vin, K * v.nAC) BA(B.out, K * v.nAC) BA(B.dSig, K * v.nCell) BA(B.gPartG, K * 2 * GRAD_NG * v.nCell) BA(B.qPart, SV * v.ny) BA(B.scale, 4 * K)
    BA(B.dbcL, SV * v.nz) BA(B.dbcR, SV * v.nz) BA(B.dbcB, SV * (v.ny + 1)) BA(B.jv, K * v.nData) BA(B.u, K * v.nData) BA(B.vbar, K * v.nData) BA(B.rxCoef, SV * v.nRx)
    BA(B.srcB, SV * 4) BA(B.wL, SV * v.nz) BA(B.wR, SV * v.nz) BA(B.colw, SV * v.ny) BA(B.gL, SV * v.nz) BA(B.gR, SV * v.nz)
    k.omega = B.omega; k.invp = B.invp; k.invp32 = B.inst.d_invp32;
    // the persistent kernel's own words for this instance (persist_alloc): more system slots where the share has the CUs for them;
    // its 32-bit lane offsets carry the system's element offset, so a block beyond 2^27 elements runs the launch-per-phase loop
    if (ctx->cfg.persistCW > 0 && SV * VS < ((size_t)1 << 27)) {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, ctx->cfg.device));
        const int cuPerXcd = prop.multiProcessorCount / 8 / std::max(ctx->cfg.shareCnt, 1);
        B.slots = std::max(1, std::min((int)((SV + 7) / 8), cuPerXcd / std::max(ctx->cfg.persistG, 1)));
        B.inst.psyncBytes = ((size_t)(32 * 8 * B.slots + 16) * sizeof(unsigned) + 15) & ~(size_t)15;
        unsigned char* ps = nullptr; BA(ps, B.inst.psyncBytes) B.inst.d_psync = reinterpret_cast<unsigned*>(ps);
        unsigned char* pr = nullptr; BA(pr, SV * MAXNB * 2 * 8 * 16) B.inst.d_prec = reinterpret_cast<u4v*>(pr);
        unsigned char* pc = nullptr; BA(pc, sizeof(PsConst)) B.inst.d_psConst = reinterpret_cast<PsConst*>(pc);
        if (ctx->cfg.persistCS > 1) BA(B.inst.d_yhat2, SV * VS)
    }
#undef BA
    HIPCHK(hipHostMalloc((void**)&B.inst.h_rec, sizeof(double) * 4 * SV, hipHostMallocMapped));
    B.hostAllocs.push_back(B.inst.h_rec);
    HIPCHK(hipHostGetDevicePointer((void**)&B.inst.d_recHost, B.inst.h_rec, 0));
    HIPCHK(hipHostMalloc((void**)&B.h_onV, sizeof(int) * SV, hipHostMallocMapped));
    B.hostAllocs.push_back(B.h_onV);
    HIPCHK(hipHostGetDevicePointer((void**)&B.d_onVHost, B.h_onV, 0));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    B.cap = nvec;
    return 0;
}
static int blk_alloc(hmcmt_ctx* ctx, int nvec) {
    if (ctx->blk.cap >= nvec) return 0;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    blk_release(ctx);
    const int rc = blk_alloc_impl(ctx, nvec);
    if (rc) {                                            // (out of memory: nothing of the block instance is kept, the context goes on)
        const std::string e = ctx->err;
        (void)hipStreamSynchronize(ctx->stream);
        blk_release(ctx);
        (void)hipGetLastError();
        ctx->err = "block Jacobian product: " + e;
    }
    return rc;
}

// the inverse pivots of the linearisation point per direction (again after a new point, or for another nvec), and the frequency
// list repeated per direction
static int blk_pivots(hmcmt_ctx* ctx, int nvec) {
    hmcmt_ctx::Blk& B = ctx->blk;
    hipStream_t strm = ctx->stream;
    if (B.gen == ctx->jvp.gen && B.genVec == nvec) return 0;
    const unsigned gx = (unsigned)std::min<long>(64, (ctx->v.vstride + 255) / 256);
    hipLaunchKernelGGL(k_blk_replicate, dim3(gx, ctx->v.S, nvec), dim3(256), 0, strm, (const cplx*)ctx->v.invp, (const float2*)ctx->inst.d_invp32,
                       B.invp, B.inst.d_invp32, ctx->v.nFreq, nvec, ctx->v.vstride);
    HIPCHK(hipGetLastError());
    if (B.genVec != nvec) {
        const int nF = ctx->v.nFreq;
        std::vector<double> om((size_t)nvec * 2 * nF);
        for (int j = 0; j < nvec; ++j)
            for (int f = 0; f < nF; ++f) {
                om[(size_t)j * nF + f] = ctx->hp.omega[f];
                om[((size_t)nvec + j) * nF + f] = ctx->hp.omega[nF + f];
            }
        HIPCHK(hipStreamSynchronize(strm));
        HIPCHK(hipMemcpy(B.omega, om.data(), sizeof(double) * om.size(), hipMemcpyHostToDevice));
    }
    B.gen = ctx->jvp.gen; B.genVec = nvec;
    return 0;
}

// the block instance in the context's place, and the virtual problem's Solver and View, for solve() (inside the bracket, which puts
// View, Solver and the queue tables back; blk_leave: the instance)
static void blk_enter(hmcmt_ctx* ctx, int nvec) {
    hmcmt_ctx::Blk& B = ctx->blk;
    std::swap(ctx->inst, B.inst);                        // (its psShadow / psConstValid come along, and go back with it: they survive between calls)
    // (no sync words: no persistent kernel for this block -- persist_fits)
    if (ctx->inst.d_psync) ctx->inst.persistSlots = std::max(1, std::min(B.slots, (nvec * ctx->v.S + 7) / 8));   // (words of the largest block seen, this call's count of systems)
    ctx->inst.dinvValid = false;                         // (the instance's Jacobi diagonals: written where a launch-per-phase kernel needs them)
    ctx->ss.psOrder[0].clear(); ctx->ss.psOrder[1].clear();    // (the queue tables are the context's problem's: the kernel's own order here)
    ctx->sv = B.sv;
    ctx->v.S *= nvec; ctx->v.nFreq *= nvec; ctx->v.omega = B.omega; ctx->v.invp = B.invp; ctx->v.sysOn = B.sysOnV;
    ctx->v.Lam = B.lam; ctx->v.R = B.sv.r;
    ctx->sv.S = ctx->v.S; ctx->sv.nFreq = ctx->v.nFreq;  // (arrays of the largest block seen, this call's count of systems)
}
static void blk_leave(hmcmt_ctx* ctx) { std::swap(ctx->inst, ctx->blk.inst); }

// the directions k_dir_norm found not identically zero -> the system flags by direction and by virtual system, made on the device
// (k_blk_flags); the host reads the flags by virtual system from mapped memory.  One synchronisation, no copy.
static int blk_systems(hmcmt_ctx* ctx, const int* d_realOn, int S, int nvec, int& nOn) {
    hmcmt_ctx::Blk& B = ctx->blk;
    const int n = nvec * S;
    hipLaunchKernelGGL(k_blk_flags, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const int*)B.dirOn, d_realOn, B.sysOnDir, B.sysOnV, B.d_onVHost, S / 2, nvec);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    nOn = 0;
    for (int i = 0; i < n; ++i) nOn += B.h_onV[i];
    ctx->ss.nSysOn = nOn;
    return 0;
}

// ----------------------------------------------------------------------------------------------
// the products' one pipeline.  vr: the REAL problem's View on the call's work arrays; the directions' systems (vr.sysOn, and `on`
// for the records) are the problem's own for nvec = 1 -- no flags to make, no synchronisation or read-back in front of the solve:
// an all-zero direction is a zero right-hand side, which leaves the solve at iteration 0 -- and blk_systems' for nvec > 1.
// ----------------------------------------------------------------------------------------------
static const int* prod_on(const hmcmt_ctx* ctx, int nvec) { return nvec > 1 ? ctx->blk.h_onV : ctx->hp.sysOn.data(); }
// the work arrays of a call: one direction's (hmcmt_ctx::Jvp), or the block's
static const hmcmt_ctx::ProdArrays& prod_arrays(const hmcmt_ctx* ctx, int nvec) {
    if (nvec > 1) return ctx->blk;
    return ctx->jvp;
}

// J V -> vr.jv (d_V: device, [nvec][nAC])
static int prod_tangent(hmcmt_ctx* ctx, View vr, const int* d_realOn, const double* d_V, int nvec, int wrt, int sweeps, hmcmt_stats& st, int& nOn) {
    hipStream_t strm = ctx->stream;
    const int S = vr.S;
    vr.tanV = d_V;
    HIPCHK(hipMemsetAsync(vr.jv, 0, sizeof(cplx) * (size_t)nvec * vr.nData, strm));
    hipLaunchKernelGGL(k_dir_dsig, dim3((vr.nCell + 255) / 256, nvec), dim3(256), 0, strm, vr, wrt, nvec);
    hipLaunchKernelGGL(k_dir_norm, dim3(nvec), dim3(1024), 0, strm, vr.dSig, (const double*)vr.sigma, (long)vr.nCell, (long)vr.nCell,
                       prod_arrays(ctx, nvec).scale, 0, nvec > 1 ? ctx->blk.dirOn : nullptr);
    if (nvec > 1) {
        if (int rc = blk_systems(ctx, d_realOn, S, nvec, nOn)) return rc;
        if (nOn == 0) return 0;                          // (every direction zero: J V = 0 stands)
    }
    const dim3 gd((2 * vr.nz + vr.ny - 1 + DBC_WAVES - 1) / DBC_WAVES, S, nvec > 1 ? (nvec + BLK_KB - 1) / BLK_KB : 1);
    const auto kdbc = nvec > 1 ? k_dbc<BLK_KB> : k_dbc<1>;
    hipLaunchKernelGGL(kdbc, gd, dim3(64 * DBC_WAVES), 0, strm, vr, nvec);
    auto fill = [&](bool) {
        hipLaunchKernelGGL(k_dir_rhs, dim3((unsigned)((vr.vstride + 255) / 256), S, nvec), dim3(256), 0, strm, vr, nvec);
    };
    if (int rc = borrowed_solve(ctx, vr.Lam, 0, sweeps, -1, fill, st, prod_on(ctx, nvec), "Jacobian product: the tangent")) return rc;
    hipLaunchKernelGGL(k_dir_data, dim3((vr.nRx + 63) / 64, S), dim3(64), 0, strm, vr, nvec);
    HIPCHK(hipGetLastError());
    return 0;
}

// Re(J^T conj(U)) -> d_out (d_U: device, complex [nvec][nData]; d_out: device, [nvec][nAC])
static int prod_adjoint(hmcmt_ctx* ctx, View vr, const int* d_realOn, const cplx* d_U, int nvec, int wrt, int sweeps, double* d_out, hmcmt_stats& st, int& nOn) {
    hipStream_t strm = ctx->stream;
    const int S = vr.S;
    vr.uData = d_U;
    hipLaunchKernelGGL(k_dir_vbar, grid1(vr.nData, 256), dim3(256), 0, strm, vr, nvec);
    hipLaunchKernelGGL(k_dir_norm, dim3(nvec), dim3(1024), 0, strm, reinterpret_cast<double*>(vr.vbar), (const double*)nullptr, 2l * vr.nData, 2l * vr.nData,
                       prod_arrays(ctx, nvec).scale, 2, nvec > 1 ? ctx->blk.dirOn : nullptr);
    if (nvec > 1) {
        if (int rc = blk_systems(ctx, d_realOn, S, nvec, nOn)) return rc;
        if (nOn == 0) { HIPCHK(hipMemsetAsync(d_out, 0, sizeof(double) * (size_t)nvec * vr.nAC, strm)); return 0; }
    }
    hipLaunchKernelGGL(k_dir_rxcoef, dim3((vr.nRx + 63) / 64, S), dim3(64), 0, strm, vr, nvec);
    const int nsrc = (2 * (vr.ny + 1) + 127) / 128;
    const size_t vecBytes = (size_t)nvec * S * vr.vstride * sizeof(cplx);
    auto fill = [&](bool sparse) {
        if (!sparse) (void)hipMemsetAsync(vr.R, 0, vecBytes, strm);           // (the whole right-hand side is the residual)
        // (one direction: the gradient's own k_src, with the receiver table in LDS -- the one place with two kernels, k_blk_src)
        if (nvec > 1) hipLaunchKernelGGL(k_blk_src, dim3(nsrc + (vr.ny + 127) / 128, S, nvec), dim3(128), 0, strm, vr, nsrc, nvec);
        else hipLaunchKernelGGL(k_src, dim3(nsrc + (vr.ny + 127) / 128, S), dim3(128), 0, strm, vr, ctx->jvp.misfit, nsrc);
    };
    if (int rc = borrowed_solve(ctx, vr.Lam, 1, sweeps, vr.zid, fill, st, prod_on(ctx, nvec), "Jacobian product: the adjoint")) return rc;
    hipLaunchKernelGGL(k_dir_wb, dim3((vr.nz + vr.ny + 127) / 128, S, nvec), dim3(128), 0, strm, vr, nvec);
    const dim3 gc((BCC_L * vr.nz + 127) / 128, nvec > 1 ? 2 * ((nvec + BLK_KB - 1) / BLK_KB) : 2, S);
    const auto kcontract = nvec > 1 ? k_contract<BLK_KB> : k_contract<1>;
    hipLaunchKernelGGL(kcontract, gc, dim3(128), 0, strm, vr, nvec);
    hipLaunchKernelGGL(k_dir_gradcell, dim3((vr.nCell + 127) / 128, 2 * GRAD_NG, nvec), dim3(128), 0, strm, vr, nvec);
    hipLaunchKernelGGL(k_dir_final, grid1(vr.nAC, 128), dim3(128), 0, strm, vr, wrt, d_out, nvec);
    HIPCHK(hipGetLastError());
    return 0;
}

enum { PROD_JVP = 0, PROD_JTVP = 1, PROD_GN = 2 };
// d_in / d_out: device pointers, [nvec] times (jvp: v[nAC] -> Jv complex[nData]; jtvp: u complex[nData] -> [nAC]; gn: v[nAC] -> [nAC]).
// Statistics: nsystems is S from the single entry points and the count of systems solved from the block ones (blockStats).
static int prod_run(hmcmt_ctx* ctx, int what, const double* d_in, int nvec, int wrt, double* d_out, bool blockStats, hmcmt_stats* stOut) {
    hmcmt_ctx::Blk& B = ctx->blk;
    hipStream_t strm = ctx->stream;
    if (nvec > 1)
        if (int rc = blk_pivots(ctx, nvec)) return rc;
    Borrowed b(ctx, stOut);
    hmcmt_stats& st = b.st;
    // the REAL problem's View on the work arrays, for the products' kernels ...
    const hmcmt_ctx::ProdArrays& W = prod_arrays(ctx, nvec);
    View vr = product_view(ctx, W, what == PROD_JVP ? reinterpret_cast<cplx*>(d_out) : nullptr);
    const int* d_realOn = ctx->v.sysOn;                  // (the problem's own flags, [S])
    int nOn = ctx->ss.nSysOn;                            // (one direction: the systems that carry data)
    st.nsystems = !blockStats ? vr.S : nvec == 1 ? nOn : 0;
    // ... and for solve(): the context itself for one direction -- no second solver instance --, the block instance in its place
    AtExit instanceBack([&] { if (nvec > 1) blk_leave(ctx); });
    if (nvec > 1) { blk_enter(ctx, nvec); vr.sysOn = B.sysOnDir; }
    if (nvec > 1) adjoint_arrays(vr, B, ctx->sv.r);
    else adjoint_arrays(vr, ctx->jac, ctx->sv.r);        // (one direction: the explicit Jacobian's arrays)
    vr.dF = vr.Lam;
    const int sweeps = cold_sweeps(ctx);
    if (what == PROD_JVP || what == PROD_GN) {
        if (int rc = prod_tangent(ctx, vr, d_realOn, d_in, nvec, wrt, sweeps, st, nOn)) return rc;
        if (blockStats) st.nsystems = nOn;
        st.smoother_sweeps = 10 * sweeps;
    }
    if (what == PROD_GN) hipLaunchKernelGGL(k_dir_w2, grid1(vr.nData, 256), dim3(256), 0, strm, vr, W.u, nvec);
    if (what == PROD_JTVP || what == PROD_GN) {
        const cplx* u = what == PROD_GN ? W.u : reinterpret_cast<const cplx*>(d_in);
        if (int rc = prod_adjoint(ctx, vr, d_realOn, u, nvec, wrt, sweeps, d_out, st, nOn)) return rc;
        if (blockStats && what == PROD_JTVP) st.nsystems = nOn;
        st.smoother_sweeps += sweeps;
    }
    return 0;
}

// (one direction allocates nothing: a context that only ever makes single products has no block arrays)
static int prod_ready(hmcmt_ctx* ctx, int nvec) {
    HIPCHK(hipSetDevice(ctx->cfg.device));
    return nvec > 1 ? blk_alloc(ctx, nvec) : 0;
}
// host pointers: stage the input, run on the device buffers, bring the result back
static int prod_host(hmcmt_ctx* ctx, int what, const double* in, int nvec, int wrt, double* out, bool blockStats, hmcmt_stats* st) {
    const size_t nAC = ctx->v.nAC, nData = ctx->v.nData;
    const bool inData = what == PROD_JTVP, outData = what == PROD_JVP;
    const size_t nin = (size_t)nvec * (inData ? 2 * nData : nAC), nout = (size_t)nvec * (outData ? 2 * nData : nAC);
    for (size_t i = 0; i < nin; ++i)
        if (!std::isfinite(in[i])) { ctx->err = std::string(nvec > 1 ? "block " : "") + "Jacobian product: non-finite input value"; return HMCMT_EINVAL; }
    if (int rc = prod_ready(ctx, nvec)) return rc;
    // (staging: u in the set's u, v in vin; J v comes back through u, the cell vectors through out)
    const hmcmt_ctx::ProdArrays& W = prod_arrays(ctx, nvec);
    double* d_in = inData ? reinterpret_cast<double*>(W.u) : W.vin;
    double* d_out = outData ? reinterpret_cast<double*>(W.u) : W.out;
    HIPCHK(hipMemcpyAsync(d_in, in, sizeof(double) * nin, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = prod_run(ctx, what, d_in, nvec, wrt, d_out, blockStats, st)) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}
// the entry points: nvec directions; a block of one direction IS the single product (the contract defines direction j as the
// single call's result) -- the two kinds of entry point differ in their argument check and in what nsystems counts
static int prod_entry(hmcmt_ctx* ctx, bool host, bool block, int what, const double* in, int32_t nvec, int32_t wrt, double* out, hmcmt_stats* st) {
    if (!ctx) return HMCMT_EINVAL;
    if (nvec < 1 || nvec > HMCMT_BLOCK_MAX) { ctx->err = "block Jacobian product: nvec must be 1 .. HMCMT_BLOCK_MAX (32)"; return HMCMT_EINVAL; }
    if (int rc = prod_check(ctx, in, wrt, out)) return rc;
    if (host) return prod_host(ctx, what, in, nvec, wrt, out, block, st);
    if (int rc = prod_ready(ctx, nvec)) return rc;
    return prod_run(ctx, what, in, nvec, wrt, out, block, st);
}

extern "C" {
int hmcmt_jvp(hmcmt_ctx* ctx, const double* v, int32_t wrt, double* Jv, hmcmt_stats* st) { return prod_entry(ctx, true, false, PROD_JVP, v, 1, wrt, Jv, st); }
int hmcmt_jtvp(hmcmt_ctx* ctx, const double* u, int32_t wrt, double* JTu, hmcmt_stats* st) { return prod_entry(ctx, true, false, PROD_JTVP, u, 1, wrt, JTu, st); }
int hmcmt_gn_hessvec(hmcmt_ctx* ctx, const double* v, int32_t wrt, double* Hv, hmcmt_stats* st) { return prod_entry(ctx, true, false, PROD_GN, v, 1, wrt, Hv, st); }
int hmcmt_jvp_device(hmcmt_ctx* ctx, const double* d_v, int32_t wrt, double* d_Jv, hmcmt_stats* st) { return prod_entry(ctx, false, false, PROD_JVP, d_v, 1, wrt, d_Jv, st); }
int hmcmt_jtvp_device(hmcmt_ctx* ctx, const double* d_u, int32_t wrt, double* d_JTu, hmcmt_stats* st) { return prod_entry(ctx, false, false, PROD_JTVP, d_u, 1, wrt, d_JTu, st); }
int hmcmt_gn_hessvec_device(hmcmt_ctx* ctx, const double* d_v, int32_t wrt, double* d_Hv, hmcmt_stats* st) { return prod_entry(ctx, false, false, PROD_GN, d_v, 1, wrt, d_Hv, st); }
int hmcmt_jvp_block(hmcmt_ctx* ctx, const double* V, int32_t nvec, int32_t wrt, double* JV, hmcmt_stats* st) { return prod_entry(ctx, true, true, PROD_JVP, V, nvec, wrt, JV, st); }
int hmcmt_jtvp_block(hmcmt_ctx* ctx, const double* U, int32_t nvec, int32_t wrt, double* JTU, hmcmt_stats* st) { return prod_entry(ctx, true, true, PROD_JTVP, U, nvec, wrt, JTU, st); }
int hmcmt_gn_hessvec_block(hmcmt_ctx* ctx, const double* V, int32_t nvec, int32_t wrt, double* HV, hmcmt_stats* st) { return prod_entry(ctx, true, true, PROD_GN, V, nvec, wrt, HV, st); }
int hmcmt_jvp_block_device(hmcmt_ctx* ctx, const double* d_V, int32_t nvec, int32_t wrt, double* d_JV, hmcmt_stats* st) { return prod_entry(ctx, false, true, PROD_JVP, d_V, nvec, wrt, d_JV, st); }
int hmcmt_jtvp_block_device(hmcmt_ctx* ctx, const double* d_U, int32_t nvec, int32_t wrt, double* d_JTU, hmcmt_stats* st) { return prod_entry(ctx, false, true, PROD_JTVP, d_U, nvec, wrt, d_JTU, st); }
int hmcmt_gn_hessvec_block_device(hmcmt_ctx* ctx, const double* d_V, int32_t nvec, int32_t wrt, double* d_HV, hmcmt_stats* st) { return prod_entry(ctx, false, true, PROD_GN, d_V, nvec, wrt, d_HV, st); }
}  // extern "C"
