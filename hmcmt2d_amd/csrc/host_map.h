// host_map.h -- the device-resident MAP optimiser behind hmcmt_map_* (include/hmcmt.h has the algorithm): host code of hmcmt_hip.hip's
// translation unit, included inside its extern "C" block behind host_chain.h (whose chain_acc_alloc / ChainReadout it uses); kernels in
// kernels_map.h, arithmetic in hmcmt_items.h (item_map_*).
//
// Launches of one iteration without a backtrack (beyond the evaluation's own): k_map_project, k_map_coef, k_map_expand in front of the
// trial's evaluation; k_map_trial, k_lf_mnorm, k_lf_mnorm_final, k_map_trial_final behind it; MAP_COEF + MAP_SCAL doubles down and ONE
// wait, behind which the host decides the Armijo test and the pair test; an accepted step that stores its pair adds k_map_pair and
// k_map_pair_final, enqueued and not waited for.  A backtrack is k_map_clip, the evaluation and the four kernels behind it.  The
// non-descent test is decided on the device (k_map_coef falls back to the direction without pairs and raises the flag), so that no
// wait stands between the projection and the trial; the host learns the flag with the trial's scalars.  The three sums of the pair test
// (s'y, s's, y'y) come with the trial's pass for the same reason: the pair kernel runs only once the host has decided to store.

static void map_release(hmcmt_ctx* ctx) {
    auto& P = ctx->map;
    if (!P.allocs.empty() || P.h_rec) {
        hipSetDevice(ctx->cfg.device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        chain_acc_free(P.allocs);
        if (P.h_rec) hipHostFree(P.h_rec);
    }
    P = hmcmt_ctx::Map{};
}

static int map_ready(hmcmt_ctx* ctx, const char* fn, bool needRun) {
    if (ctx->statsPending) { ctx->err = std::string(fn) + ": an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    if (needRun && !ctx->map.active) {
        ctx->err = std::string(fn) + ": no MAP run (hmcmt_map_begin first; hmcmt_set_prior and hmcmt_set_mass end a run)";
        return HMCMT_EINVAL;
    }
    return 0;
}

void hmcmt_map_default_options(hmcmt_map_options* o) {
    if (!o) return;
    o->history = 8; o->max_backtracks = 10;
    o->c1 = 1e-4; o->shrink = 0.5; o->curv_eps = 1e-10; o->gtol = 1e-5;
}

static const char* map_options_error(const hmcmt_map_options& o) {
    if (o.history < 1 || o.history > HMCMT_MAP_HISTORY_MAX) return "need 1 <= history <= HMCMT_MAP_HISTORY_MAX";
    if (o.max_backtracks < 0 || o.max_backtracks > 15) return "need 0 <= max_backtracks <= 15";
    if (!(o.c1 > 0 && o.c1 < 1)) return "need 0 < c1 < 1";
    if (!(o.shrink > 0 && o.shrink < 1)) return "need 0 < shrink < 1";
    if (!(o.curv_eps >= 0) || !std::isfinite(o.curv_eps)) return "need a finite curv_eps >= 0";
    if (!(o.gtol >= 0) || !std::isfinite(o.gtol)) return "need a finite gtol >= 0";
    return nullptr;
}

static MapRing map_ring(const hmcmt_ctx::Map& P, long long n) { return MapRing{P.d_ring, n, P.opt.history, P.head, P.count}; }

// an evaluation of the run that failed: everything in flight is drained, the run's state stays (chain_fail's rule)
static int map_fail(hmcmt_ctx* ctx, int rc) {
    const std::string e = ctx->err;
    (void)collect_pending(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    prof_collect(ctx);
    ctx->err = e;
    return rc;
}

// The evaluation of d_m[t] with everything behind it, and the one wait: leaves the full gradient in d_g[t], the predicted data in
// d_pred[t] and the block [MAP_COEF + MAP_SCAL] in h_rec.  first: there is no state yet (hmcmt_map_begin).
static int map_evaluate(hmcmt_ctx* ctx, int t, bool first) {
    auto& P = ctx->map;
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    double* scal = P.d_cs + MAP_COEF;
    ctx->lfHaveGrad = false;                                 // (the evaluation arrays leave a trajectory's end point)
    int rc = evaluate(ctx, P.d_m[t], true, P.d_pred[t], scal + MS_D, P.d_gd);
    if (rc) return map_fail(ctx, rc);
    MapTrial T{n, first ? nullptr : P.d_m[P.cur], first ? nullptr : P.d_g[P.cur], P.d_m[t], P.d_gd, P.d_g[t], P.regParam,
               ctx->d_mref, ctx->d_wmVal, ctx->d_wmRow, ctx->d_wmCol, P.lo, P.hi, P.d_part};
    hipLaunchKernelGGL(k_map_trial, dim3(LFNB), dim3(256), 0, st, T);
    LfView lf{n, ctx->d_mref, ctx->d_invM, ctx->d_wmVal, ctx->d_wmRow, ctx->d_wmCol, P.d_m[t], nullptr, ctx->d_g,
              ctx->d_lfPart, ctx->d_lfScal, ctx->d_lfFlag, ctx->v.ticks};
    hipLaunchKernelGGL(k_lf_mnorm, dim3(LFNB), dim3(256), 0, st, lf, P.regParam);
    hipLaunchKernelGGL(k_lf_mnorm_final, dim3(1), dim3(1), 0, st, lf, P.regParam);
    hipLaunchKernelGGL(k_map_trial_final, dim3(1), dim3(64), 0, st, P.d_part, ctx->d_lfScal, scal);
    if (hipMemcpyAsync(P.h_rec, P.d_cs, sizeof(double) * (MAP_COEF + MAP_SCAL), hipMemcpyDeviceToHost, st) != hipSuccess) {
        ctx->err = "hmcmt_map: the record's copy failed";
        return map_fail(ctx, HMCMT_EHIP);
    }
    if ((rc = collect_stats(ctx, true))) return map_fail(ctx, rc);          // the trial's one wait
    prof_collect(ctx);
    if ((rc = finish_status(ctx))) return map_fail(ctx, rc);
    if (hipGetLastError() != hipSuccess) { ctx->err = "hmcmt_map: a launch failed"; return map_fail(ctx, HMCMT_EHIP); }
    return 0;
}

static void map_fill_record(const hmcmt_ctx::Map& P, hmcmt_map_record* rec) {
    rec->iter = (int32_t)P.iter; rec->status = P.status; rec->npairs = P.count; rec->nbound = P.nbound;
    rec->phi = P.phi; rec->D = P.D; rec->M = P.M; rec->pg_inf = P.pginf; rec->pg_2 = std::sqrt(P.pg2);
}
static void map_blank_record(hmcmt_map_record* rec) {
    *rec = hmcmt_map_record{};
    for (double& v : rec->phi_trial) v = std::nan("");
}

int hmcmt_map_begin(hmcmt_ctx* ctx, const double* m_start, double regParam, double lnSigMin, double lnSigMax, const hmcmt_map_options* options,
                    hmcmt_map_record* rec0) {
    const char* fn = "hmcmt_map_begin";
    if (!ctx) return HMCMT_EINVAL;
    if (!m_start) { ctx->err = std::string(fn) + ": m_start is NULL"; return HMCMT_EINVAL; }
    int rc = map_ready(ctx, fn, false);
    if (rc) return rc;
    if (!ctx->havePrior) { ctx->err = std::string(fn) + ": hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (!std::isfinite(regParam) || !std::isfinite(lnSigMin) || !std::isfinite(lnSigMax) || !(lnSigMax > lnSigMin)) {
        ctx->err = std::string(fn) + ": need finite regParam and lnSigMax > lnSigMin";
        return HMCMT_EINVAL;
    }
    hmcmt_map_options o;
    hmcmt_map_default_options(&o);
    if (options) o = *options;
    if (const char* e = map_options_error(o)) { ctx->err = std::string(fn) + ": " + e; return HMCMT_EINVAL; }
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(m_start[i])) { ctx->err = std::string(fn) + ": non-finite start model"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& P = ctx->map;
    // a begin over a run keeps that run's buffers where the history fits them (the other sizes belong to the context)
    const bool reuse = P.h_rec != nullptr && P.cap >= o.history;
    if (!reuse) map_release(ctx);
    P.active = false;
    hipStream_t st = ctx->stream;
    auto build = [&]() -> int {
        int r;
        if (!reuse) {
            const size_t H = (size_t)o.history;
            const std::pair<double**, size_t> bufs[] = {
                {&P.d_m[0], (size_t)n}, {&P.d_m[1], (size_t)n}, {&P.d_g[0], (size_t)n}, {&P.d_g[1], (size_t)n}, {&P.d_pred[0], (size_t)2 * nData},
                {&P.d_pred[1], (size_t)2 * nData}, {&P.d_gd, (size_t)n}, {&P.d_pg, (size_t)n}, {&P.d_d, (size_t)n}, {&P.d_ring, 2 * H * (size_t)n},
                {&P.d_part, (size_t)MAP_PART_ROWS * LFNB}, {&P.d_SY, H * H}, {&P.d_YY, H * H}, {&P.d_cs, (size_t)(MAP_COEF + MAP_SCAL)}};
            for (const auto& b : bufs)
                if ((r = chain_acc_zeroed(ctx, fn, P.allocs, (void**)b.first, std::max<size_t>(b.second, 1) * sizeof(double)))) return r;
            if (hipHostMalloc((void**)&P.h_rec, sizeof(double) * (MAP_COEF + MAP_SCAL), hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                P.h_rec = nullptr;
                ctx->err = std::string(fn) + ": pinned allocation failed";
                return HMCMT_ENOMEM;
            }
            P.cap = o.history;
        } else {
            HIPCHK(hipMemsetAsync(P.d_cs, 0, sizeof(double) * (MAP_COEF + MAP_SCAL), st));
        }
        P.opt = o; P.regParam = regParam; P.lo = lnSigMin; P.hi = lnSigMax;
        P.cur = 0; P.head = P.count = 0; P.iter = 0;
        for (int i = 0; i < n; ++i) ctx->h_stage[i] = m_start[i] < lnSigMin ? lnSigMin : (m_start[i] > lnSigMax ? lnSigMax : m_start[i]);
        HIPCHK(hipMemcpyAsync(P.d_m[0], ctx->h_stage, sizeof(double) * n, hipMemcpyHostToDevice, st));
        return map_evaluate(ctx, 0, true);
    };
    if ((rc = build())) {
        const std::string e = ctx->err;
        map_release(ctx);
        ctx->err = e;
        return rc;
    }
    const double* s = P.h_rec + MAP_COEF;
    P.D = s[MS_D]; P.M = s[MS_M]; P.phi = P.D + P.M;
    P.pg2 = s[MS_PG2]; P.pginf = P.pginf0 = s[MS_PGINF]; P.nbound = (int)s[MS_NB];
    if (!std::isfinite(P.phi) || !std::isfinite(P.pg2)) {
        map_release(ctx);
        ctx->err = std::string(fn) + ": non-finite objective or gradient at the start model";
        return HMCMT_EBREAKDOWN;
    }
    P.status = P.pginf <= o.gtol * std::max(1.0, P.pginf0) ? HMCMT_MAP_CONVERGED : HMCMT_MAP_RUNNING;
    P.active = true;
    if (rec0) { map_blank_record(rec0); map_fill_record(P, rec0); rec0->nfevals = 1; }
    return 0;
}

// One round: the direction of the state and its line search.  *accepted: a trial passed (its scalars are in h_rec, the trial in buffer
// cur ^ 1); *fellBack: the device set the pairs aside (not a descent direction).  A failed evaluation has gone through map_fail.
static int map_round(hmcmt_ctx* ctx, hmcmt_map_record* rec, bool* accepted, bool* fellBack) {
    auto& P = ctx->map;
    const int n = ctx->v.nAC, t = P.cur ^ 1;
    hipStream_t st = ctx->stream;
    MapDir D{map_ring(P, n), P.d_m[P.cur], P.d_g[P.cur], P.lo, P.hi, P.d_pg, P.d_d, P.d_m[t], P.d_part, P.d_SY, P.d_YY, P.d_cs};
    hipLaunchKernelGGL(k_map_project, dim3(LFNB), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_map_coef, dim3(1), dim3(64), 0, st, D, (double*)nullptr);
    double alpha = 1.0;
    hipLaunchKernelGGL(k_map_expand, dim3(LFNB), dim3(256), 0, st, D, alpha);
    *accepted = *fellBack = false;
    for (double& v : rec->phi_trial) v = std::nan("");
    for (int k = 0; k <= P.opt.max_backtracks; ++k) {
        if (k > 0) {
            alpha *= P.opt.shrink;
            hipLaunchKernelGGL(k_map_clip, dim3((n + 255) / 256), dim3(256), 0, st, (long long)n, P.d_m[P.cur], P.d_d, alpha, P.lo, P.hi, P.d_m[t]);
        }
        const int rc = map_evaluate(ctx, t, false);
        if (rc) return rc;
        ++rec->nfevals;
        const double* c = P.h_rec;
        const double* s = P.h_rec + MAP_COEF;
        const double phiT = s[MS_D] + s[MS_M];
        rec->phi_trial[k] = phiT;
        rec->backtracks = k; rec->alpha = alpha; rec->gamma = c[MC_GAMMA]; rec->gTd = c[MC_GTD];
        *fellBack = c[MC_FLAG] != 0.0;
        if (std::isfinite(phiT) && std::isfinite(s[MS_PG2]) && phiT <= P.phi + P.opt.c1 * s[MS_GTS]) { *accepted = true; return 0; }
    }
    return 0;
}

int hmcmt_map_step(hmcmt_ctx* ctx, hmcmt_map_record* rec) {
    const char* fn = "hmcmt_map_step";
    if (!ctx) return HMCMT_EINVAL;
    if (!rec) { ctx->err = std::string(fn) + ": rec is NULL"; return HMCMT_EINVAL; }
    int rc = map_ready(ctx, fn, true);
    if (rc) return rc;
    auto& P = ctx->map;
    if (P.status != HMCMT_MAP_RUNNING) {
        ctx->err = std::string(fn) + ": the run has " + (P.status == HMCMT_MAP_CONVERGED ? "converged" : "stalled") + " (hmcmt_map_begin starts another)";
        return HMCMT_EINVAL;
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    const int head0 = P.head, count0 = P.count;
    map_blank_record(rec);
    bool accepted = false;
    for (;;) {
        const bool hadPairs = P.count > 0;
        bool fellBack = false;
        if ((rc = map_round(ctx, rec, &accepted, &fellBack))) { P.head = head0; P.count = count0; return rc; }
        bool pairsUsed = hadPairs;
        if (hadPairs && fellBack) { ++rec->resets; P.head = P.count = 0; pairsUsed = false; }     // (the round ran without them)
        if (accepted || !pairsUsed) break;
        ++rec->resets; P.head = P.count = 0;                   // every trial failed with pairs: once more without
    }
    if (!accepted) {
        P.status = HMCMT_MAP_STALLED;
        rec->alpha = 0.0;
        map_fill_record(P, rec);
        return 0;
    }
    const double* s = P.h_rec + MAP_COEF;
    const int t = P.cur ^ 1, H = P.opt.history;
    rec->sTy = s[MS_STY];
    if (s[MS_STY] > P.opt.curv_eps * std::sqrt(s[MS_STS]) * std::sqrt(s[MS_YTY])) {
        // the pairs that stay: all of them, or all but the oldest where the ring is full (the new pair takes its slot)
        if (P.count == H) { P.head = (P.head + 1) % H; --P.count; }
        const int slot = (P.head + P.count) % H;
        MapPair Q{map_ring(P, n), P.d_ring, slot, P.d_m[P.cur], P.d_g[P.cur], P.d_m[t], P.d_g[t], P.d_part, P.d_SY, P.d_YY, P.d_cs + MAP_COEF};
        hipLaunchKernelGGL(k_map_pair, dim3(LFNB), dim3(256), 0, st, Q);
        hipLaunchKernelGGL(k_map_pair_final, dim3(1), dim3(64), 0, st, Q);
        ++P.count;
        rec->pair_stored = 1;
    }
    P.cur = t;
    P.D = s[MS_D]; P.M = s[MS_M]; P.phi = P.D + P.M;
    P.pg2 = s[MS_PG2]; P.pginf = s[MS_PGINF]; P.nbound = (int)s[MS_NB];
    ++P.iter;
    if (P.pginf <= P.opt.gtol * std::max(1.0, P.pginf0)) P.status = HMCMT_MAP_CONVERGED;
    map_fill_record(P, rec);
    HIPCHK(hipGetLastError());
    return 0;
}

int hmcmt_map_run(hmcmt_ctx* ctx, int32_t maxiter, hmcmt_map_record* recs, int32_t* ndone) {
    const char* fn = "hmcmt_map_run";
    if (!ctx) return HMCMT_EINVAL;
    if (ndone) *ndone = 0;
    if (maxiter < 0) { ctx->err = std::string(fn) + ": need maxiter >= 0"; return HMCMT_EINVAL; }
    int rc = map_ready(ctx, fn, true);
    if (rc) return rc;
    if (ctx->map.status != HMCMT_MAP_RUNNING && maxiter > 0) {
        ctx->err = std::string(fn) + ": the run has ended (hmcmt_map_begin starts another)";
        return HMCMT_EINVAL;
    }
    for (int32_t k = 0; k < maxiter && ctx->map.status == HMCMT_MAP_RUNNING; ++k) {
        hmcmt_map_record r;
        if ((rc = hmcmt_map_step(ctx, &r))) return rc;
        if (recs) recs[k] = r;
        if (ndone) *ndone = k + 1;
    }
    return 0;
}

int hmcmt_map_state(hmcmt_ctx* ctx, double* m, double* grad, double* pred, int32_t on_device) {
    const char* fn = "hmcmt_map_state";
    if (!ctx) return HMCMT_EINVAL;
    const int rc = map_ready(ctx, fn, true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& P = ctx->map;
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    hipStream_t st = ctx->stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (m) HIPCHK(hipMemcpyAsync(m, P.d_m[P.cur], sizeof(double) * n, kind, st));
    if (grad) HIPCHK(hipMemcpyAsync(grad, P.d_g[P.cur], sizeof(double) * n, kind, st));
    if (pred) HIPCHK(hipMemcpyAsync(pred, P.d_pred[P.cur], sizeof(double) * 2 * nData, kind, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int hmcmt_map_end(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    if (ctx->statsPending) { ctx->err = "hmcmt_map_end: an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    map_release(ctx);
    return 0;
}

// ---- test hooks (hmcmt_debug.h) ---------------------------------------------------------------------------------------------------
int hmcmt_debug_map_direction(hmcmt_ctx* ctx, const hmcmt_debug_map_args* a) {
    const char* fn = "hmcmt_debug_map_direction";
    if (!ctx) return HMCMT_EINVAL;
    static_assert(HMCMT_MAP_SUMS == MAP_COEF + MAP_ROWS_MAX, "the hook's header mirrors hmcmt_items.h");
    const bool ok = a && a->n >= 1 && a->n <= (int64_t)HMCMT_MAP_HOOK_NMAX && a->history >= 1 && a->history <= MAP_HISTORY_MAX && a->count >= 0 &&
                    a->count <= a->history && a->head >= 0 && a->head < a->history && a->m && a->g && (a->count == 0 || (a->rows && a->sy && a->yy)) &&
                    std::isfinite(a->lo) && std::isfinite(a->hi) && a->hi > a->lo && std::isfinite(a->alpha);
    if (!ok) { ctx->err = std::string(fn) + ": need args, 1 <= n <= HMCMT_MAP_HOOK_NMAX, a ring within 1 <= history <= HMCMT_MAP_HISTORY_MAX, m, g, finite lo < hi and alpha"; return HMCMT_EINVAL; }
    const int rdy = map_ready(ctx, fn, false);
    if (rdy) return rdy;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)a->n, H = (size_t)a->history, vb = n * sizeof(double);
    ChainReadout R(ctx, fn, false);
    double* d_rows = (double*)R.scratch(2 * H * vb);
    double* d_sy = (double*)R.scratch(H * H * sizeof(double));
    double* d_yy = (double*)R.scratch(H * H * sizeof(double));
    double* d_m = (double*)R.scratch(vb);
    double* d_g = (double*)R.scratch(vb);
    double* d_part = (double*)R.scratch(sizeof(double) * MAP_PART_ROWS * LFNB);
    double* d_sums = (double*)R.scratch(sizeof(double) * HMCMT_MAP_SUMS);
    double* d_pg = (double*)R.scratch(vb);
    double* d_d = (double*)R.scratch(vb);
    double* d_mt = (double*)R.scratch(vb);
    if (R.rc) return R.rc;
    if (a->count > 0) {
        HIPCHK(hipMemcpyAsync(d_rows, a->rows, 2 * H * vb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_sy, a->sy, H * H * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_yy, a->yy, H * H * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(d_m, a->m, vb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_g, a->g, vb, hipMemcpyHostToDevice, st));
    MapDir D{MapRing{d_rows, (long long)a->n, a->history, a->head, a->count}, d_m, d_g, a->lo, a->hi, d_pg, d_d, d_mt, d_part, d_sy, d_yy, d_sums};
    hipLaunchKernelGGL(k_map_project, dim3(LFNB), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_map_coef, dim3(1), dim3(64), 0, st, D, d_sums + MAP_COEF);
    hipLaunchKernelGGL(k_map_expand, dim3(LFNB), dim3(256), 0, st, D, a->alpha);
    HIPCHK(hipGetLastError());
    if (a->pg) HIPCHK(hipMemcpyAsync(a->pg, d_pg, vb, hipMemcpyDeviceToHost, st));
    if (a->d) HIPCHK(hipMemcpyAsync(a->d, d_d, vb, hipMemcpyDeviceToHost, st));
    if (a->mt) HIPCHK(hipMemcpyAsync(a->mt, d_mt, vb, hipMemcpyDeviceToHost, st));
    if (a->sums) HIPCHK(hipMemcpyAsync(a->sums, d_sums, sizeof(double) * HMCMT_MAP_SUMS, hipMemcpyDeviceToHost, st));
    return R.finish();
}

int hmcmt_debug_map_rows(hmcmt_ctx* ctx, int32_t* info, double* rows, double* sy, double* yy) {
    const char* fn = "hmcmt_debug_map_rows";
    if (!ctx) return HMCMT_EINVAL;
    const int rc = map_ready(ctx, fn, true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& P = ctx->map;
    const size_t n = (size_t)ctx->v.nAC, H = (size_t)P.opt.history;
    hipStream_t st = ctx->stream;
    if (info) { info[0] = P.opt.history; info[1] = P.head; info[2] = P.count; info[3] = (int32_t)P.iter; }
    if (rows) HIPCHK(hipMemcpyAsync(rows, P.d_ring, 2 * H * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (sy) HIPCHK(hipMemcpyAsync(sy, P.d_SY, H * H * sizeof(double), hipMemcpyDeviceToHost, st));
    if (yy) HIPCHK(hipMemcpyAsync(yy, P.d_YY, H * H * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
