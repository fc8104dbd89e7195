// host_chain.h -- the device-resident HMC chain behind hmcmt_chain_* (include/hmcmt.h): host code of hmcmt_hip.hip's translation
// unit, included at the end of its extern "C" block (behind leapfrog_core and mass_apply_dev); kernels in kernels_chain.h.
//
// One sample = hmcmt_chain_momentum + hmcmt_chain_step.  What crosses PCIe per sample: nAC normals up, LFNB partial sums and
// CHAIN_REC scalars down; with outputs, nAC + 2 nData doubles more.  Launches per sample beyond leapfrog_core's (diagonal mass):
// k_chain_momentum, k_chain_kinetic, k_chain_final, k_chain_welford; with the optional accumulators of the commit on,
// k_chain_hist, a second k_chain_welford (the predicted data), k_chain_acov (lagged autocovariances) and k_chain_cov_commit (cross
// moments; every `batch` commits k_chain_cov_flush) behind them.

// measurement only (hmcmt_debug_chain_acov_time): the event pairs round the k_chain_acov launches
static void chain_acov_time_collect(hmcmt_ctx* ctx) {
    auto& A = ctx->chain.acov;
    if (A.pending.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (size_t i = 0; i < A.pending.size(); ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, A.ev[2 * i], A.ev[2 * i + 1]) == hipSuccess) { A.ms[A.pending[i]] += ms; A.launches[A.pending[i]] += 1; }
    }
    A.pending.clear();
}
static void chain_acov_time_free(hmcmt_ctx* ctx) {
    auto& A = ctx->chain.acov;
    if (A.ev.empty()) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : A.ev) hipEventDestroy(e);
    A.ev.clear(); A.pending.clear();
    A.timing = false;
}

// measurement only (hmcmt_debug_chain_cov_time): the event pairs round the k_chain_cov_commit and k_chain_cov_flush launches
static void chain_cov_time_collect(hmcmt_ctx* ctx) {
    auto& V = ctx->chain.cov;
    if (V.pending.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (size_t i = 0; i < V.pending.size(); ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, V.ev[2 * i], V.ev[2 * i + 1]) == hipSuccess) { V.ms[V.pending[i]] += ms; V.launches[V.pending[i]] += 1; }
    }
    V.pending.clear();
}
static void chain_cov_time_free(hmcmt_ctx* ctx) {
    auto& V = ctx->chain.cov;
    if (V.ev.empty()) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : V.ev) hipEventDestroy(e);
    V.ev.clear(); V.pending.clear();
    V.timing = false;
}
// the first event of the next pair of the pool, recorded (false: not timing, or no event to be had); chain_cov_time_stop closes it
static bool chain_cov_time_start(hmcmt_ctx* ctx) {
    auto& V = ctx->chain.cov;
    if (!V.timing) return false;
    if (V.pending.size() >= 1024) chain_cov_time_collect(ctx);
    const size_t i = V.pending.size();
    while (V.ev.size() < 2 * i + 2) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return false; } V.ev.push_back(e); }
    hipEventRecord(V.ev[2 * i], ctx->stream);
    return true;
}
static void chain_cov_time_stop(hmcmt_ctx* ctx, int cls) {
    auto& V = ctx->chain.cov;
    hipEventRecord(V.ev[2 * V.pending.size() + 1], ctx->stream);
    V.pending.push_back(cls);
}

// folds the parked commits into S (enqueued): the commit calls it when the batch is full, a read-out when any is parked
static void chain_cov_flush(hmcmt_ctx* ctx) {
    auto& V = ctx->chain.cov;
    if (V.npend == 0) return;
    const bool timed = chain_cov_time_start(ctx);
    const long long n = ctx->v.nAC, tiles = (V.nrow + CHAIN_COV_TILE_ROWS - 1) / CHAIN_COV_TILE_ROWS;
    const dim3 grid((unsigned)((n + CHAIN_COV_TILE_COLS - 1) / CHAIN_COV_TILE_COLS), (unsigned)std::min<long long>(tiles, 32768));
    static_assert(CHAIN_COV_BATCH_MAX == 16, "one instantiation of k_chain_cov_flush per batch length below");
    switch (V.npend) {
#define HMCMT_COV_FLUSH(NB) \
    case NB: hipLaunchKernelGGL(k_chain_cov_flush<NB>, grid, dim3(CHAIN_COV_TILE_COLS), 0, ctx->stream, n, V.nrow, V.d_row, V.d_pend, V.d_S); break;
        HMCMT_COV_FLUSH(1) HMCMT_COV_FLUSH(2) HMCMT_COV_FLUSH(3) HMCMT_COV_FLUSH(4) HMCMT_COV_FLUSH(5) HMCMT_COV_FLUSH(6)
        HMCMT_COV_FLUSH(7) HMCMT_COV_FLUSH(8) HMCMT_COV_FLUSH(9) HMCMT_COV_FLUSH(10) HMCMT_COV_FLUSH(11) HMCMT_COV_FLUSH(12)
        HMCMT_COV_FLUSH(13) HMCMT_COV_FLUSH(14) HMCMT_COV_FLUSH(15) HMCMT_COV_FLUSH(16)
#undef HMCMT_COV_FLUSH
    }
    if (timed) chain_cov_time_stop(ctx, 1);
    V.npend = 0;
}

// ends the commit's optional accumulators (histogram, data moments, autocovariances, cross moments) and frees their buffers
static void chain_acc_release(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
    void* bufs[] = {C.hist.d_target, C.hist.d_counts, C.dmom.d_mean, C.dmom.d_m2, C.acov.d_target, C.acov.d_x0, C.acov.d_tot,
                    C.acov.d_S, C.acov.d_H, C.acov.d_ring, C.cov.d_row, C.cov.d_x0, C.cov.d_tot, C.cov.d_q, C.cov.d_pend, C.cov.d_S};
    chain_acov_time_free(ctx);
    chain_cov_time_free(ctx);
    bool any = false;
    for (void* p : bufs) any = any || p;
    if (any) {
        hipSetDevice(ctx->device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);      // (a commit may still be counting)
        for (void* p : bufs) if (p) hipFree(p);
    }
    C.hist = hmcmt_ctx::Chain::Hist{};
    C.dmom = hmcmt_ctx::Chain::DataMoments{};
    C.acov = hmcmt_ctx::Chain::Acov{};
    C.cov = hmcmt_ctx::Chain::Cov{};
}

static void chain_release(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
    chain_acc_release(ctx);
    if (!C.allocs.empty() || C.h_rec) {
        hipSetDevice(ctx->device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);      // (a commit may still be running on the buffers)
        for (void* p : C.allocs) hipFree(p);
        if (C.h_rec) hipHostFree(C.h_rec);
    }
    C = hmcmt_ctx::Chain{};
}

static int chain_alloc(hmcmt_ctx* ctx, double** p, size_t n) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(double);
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = std::string("hmcmt_chain_begin: device allocation failed: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? HMCMT_ENOMEM : HMCMT_EHIP;
    }
    ctx->chain.allocs.push_back(q);
    HIPCHK(hipMemsetAsync(q, 0, bytes, ctx->stream));
    *p = (double*)q;
    return 0;
}

// what every chain call checks first
static int chain_ready(hmcmt_ctx* ctx, const char* fn, bool needChain) {
    if (ctx->statsPending) { ctx->err = std::string(fn) + ": an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    if (needChain && !ctx->chain.active) {
        ctx->err = std::string(fn) + ": no chain (hmcmt_chain_begin first; hmcmt_set_prior and hmcmt_set_mass end a chain)";
        return HMCMT_EINVAL;
    }
    return 0;
}

// a step that failed: everything in flight is drained, the chain's state stays, the next step evaluates its start gradient
static int chain_fail(hmcmt_ctx* ctx, int rc) {
    const std::string e = ctx->err;
    (void)collect_pending(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    (void)leapfrog_flag(ctx);
    prof_collect(ctx);
    ctx->err = e;
    ctx->lfHaveGrad = false;
    ctx->chain.nextStart = 0;
    return rc;
}

int hmcmt_chain_begin(hmcmt_ctx* ctx, const double* m_start, double dt, double regParam, double lnSigMin, double lnSigMax,
                      int64_t burnin, double* D0, double* M0) {
    if (!ctx) return HMCMT_EINVAL;
    if (!m_start) { ctx->err = "hmcmt_chain_begin: m_start is NULL"; return HMCMT_EINVAL; }
    int rc = chain_ready(ctx, "hmcmt_chain_begin", false);
    if (rc) return rc;
    if (!ctx->havePrior) { ctx->err = "hmcmt_chain_begin: hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (!(dt > 0) || !std::isfinite(dt) || !std::isfinite(regParam) || !std::isfinite(lnSigMin) || !std::isfinite(lnSigMax) ||
        !(lnSigMax > lnSigMin) || burnin < 0) {
        ctx->err = "hmcmt_chain_begin: need finite dt > 0, regParam, lnSigMax > lnSigMin and burnin >= 0";
        return HMCMT_EINVAL;
    }
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(m_start[i])) { ctx->err = "hmcmt_chain_begin: non-finite start model"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    auto& C = ctx->chain;
    // a begin on a context that holds a chain keeps that chain's buffers (their sizes belong to the context) and zeroes them
    const bool reuse = C.h_rec != nullptr;
    if (reuse) { C.active = C.haveMomentum = false; chain_acc_release(ctx); }
    else chain_release(ctx);
    hipStream_t st = ctx->stream;
    auto build = [&]() -> int {
        int r;
        const std::pair<double**, size_t> bufs[] = {
            {&C.d_m[0], (size_t)n}, {&C.d_m[1], (size_t)n}, {&C.d_p, (size_t)n}, {&C.d_z, (size_t)n}, {&C.d_mean, (size_t)n}, {&C.d_m2, (size_t)n},
            {&C.d_pred[0], (size_t)2 * nData}, {&C.d_pred[1], (size_t)2 * nData}, {&C.d_part, (size_t)2 * LFNB}, {&C.d_scal, (size_t)CHAIN_SCAL}};
        for (const auto& b : bufs) {
            if (!reuse) { if ((r = chain_alloc(ctx, b.first, b.second))) return r; }
            else HIPCHK(hipMemsetAsync(*b.first, 0, std::max<size_t>(b.second, 1) * sizeof(double), st));
        }
        if (!reuse && hipHostMalloc((void**)&C.h_rec, sizeof(double) * (CHAIN_REC + LFNB), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            C.h_rec = nullptr;
            ctx->err = "hmcmt_chain_begin: pinned allocation failed";
            return HMCMT_ENOMEM;
        }
        std::memcpy(ctx->h_stage, m_start, sizeof(double) * n);
        HIPCHK(hipMemcpyAsync(C.d_m[0], ctx->h_stage, sizeof(double) * n, hipMemcpyHostToDevice, st));
        // the Hamiltonian terms at the start model (getHamiltonian, HMCSampler.jl:358-397): one forward evaluation, then the prior term
        if ((r = evaluate(ctx, C.d_m[0], false, C.d_pred[0], C.d_scal + CH_D1, nullptr))) return r;
        if ((r = collect_stats(ctx, false))) return r;
        prof_collect(ctx);
        if ((r = finish_status(ctx))) return r;
        LfView lf{n, ctx->d_mref, ctx->d_invM, ctx->d_wmVal, ctx->d_wmRow, ctx->d_wmCol, C.d_m[0], C.d_p, ctx->d_g,
                  ctx->d_lfPart, ctx->d_lfScal, ctx->d_lfFlag, ctx->v.ticks};
        hipLaunchKernelGGL(k_lf_mnorm, dim3(LFNB), dim3(256), 0, st, lf, regParam);
        hipLaunchKernelGGL(k_lf_mnorm_final, dim3(1), dim3(1), 0, st, lf, regParam);
        HIPCHK(hipMemcpyAsync(C.h_rec, C.d_scal + CH_D1, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(C.h_rec + 1, ctx->d_lfScal, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        return 0;
    };
    if ((rc = build())) {
        const std::string e = ctx->err;
        chain_release(ctx);
        ctx->err = e;
        return rc;
    }
    C.D = C.h_rec[0]; C.M = C.h_rec[1];
    C.dt = dt; C.regParam = regParam; C.lo = lnSigMin; C.hi = lnSigMax;
    C.burnin = burnin; C.nsamples = C.nmoments = 0;
    C.cur = 0; C.nextStart = 0; C.haveMomentum = false;
    C.gen = ctx->stateGen;
    C.active = true;
    if (D0) *D0 = C.D;
    if (M0) *M0 = C.M;
    return 0;
}

int hmcmt_chain_momentum(hmcmt_ctx* ctx, const double* z, double* K) {
    if (!ctx) return HMCMT_EINVAL;
    if (!z) { ctx->err = "hmcmt_chain_momentum: z is NULL"; return HMCMT_EINVAL; }
    int rc = chain_ready(ctx, "hmcmt_chain_momentum", true);
    if (rc) return rc;
    auto& C = ctx->chain;
    const int n = ctx->v.nAC;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(z[i])) { ctx->err = "hmcmt_chain_momentum: non-finite normal"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    C.haveMomentum = false;
    std::memcpy(ctx->h_stage, z, sizeof(double) * n);
    HIPCHK(hipMemcpyAsync(C.d_z, ctx->h_stage, sizeof(double) * n, hipMemcpyHostToDevice, st));
    if (ctx->mass.kind == HMCMT_MASS_WM) {
        // p = L clip(z), x = Wm^-1 p, K = 0.5 p'x
        hipLaunchKernelGGL(k_chain_clip, dim3((n + 255) / 256), dim3(256), 0, st, n, C.d_z, C.d_p);
        if ((rc = mass_apply_dev(ctx, HMCMT_MASS_OP_SQRT, C.d_p, C.d_p))) return rc;
        if ((rc = mass_apply_dev(ctx, HMCMT_MASS_OP_INV, C.d_p, ctx->mass.d_x))) return rc;
        hipLaunchKernelGGL(k_chain_kinetic, dim3(LFNB), dim3(256), 0, st, n, C.d_p, ctx->mass.d_x, ctx->d_invM, C.d_part);
    } else {
        hipLaunchKernelGGL(k_chain_momentum, dim3(LFNB), dim3(256), 0, st, n, C.d_z, ctx->d_invM, C.d_p, C.d_part);
    }
    // (the partial sums come over and are added here in k_chain_final's order: the same bits as the record's K0, one launch less)
    HIPCHK(hipMemcpyAsync(C.h_rec + CHAIN_REC, C.d_part, sizeof(double) * LFNB, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    C.K0 = 0.5 * item_chain_total(C.h_rec + CHAIN_REC);
    if (!std::isfinite(C.K0)) { ctx->err = "hmcmt_chain_momentum: non-finite kinetic energy (the diagonal of M^-1 must be positive)"; return HMCMT_EBREAKDOWN; }
    C.haveMomentum = true;
    if (K) *K = C.K0;
    return 0;
}

int hmcmt_chain_step(hmcmt_ctx* ctx, int32_t L, double u, hmcmt_chain_record* rec, double* m_out, double* pred_out) {
    if (!ctx) return HMCMT_EINVAL;
    if (!rec) { ctx->err = "hmcmt_chain_step: rec is NULL"; return HMCMT_EINVAL; }
    int rc = chain_ready(ctx, "hmcmt_chain_step", true);
    if (rc) return rc;
    auto& C = ctx->chain;
    if (!C.haveMomentum) { ctx->err = "hmcmt_chain_step: no momentum since the last step (hmcmt_chain_momentum first)"; return HMCMT_EINVAL; }
    if (L < 1 || !std::isfinite(u)) { ctx->err = "hmcmt_chain_step: need L >= 1 and a finite u"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    hipStream_t st = ctx->stream;
    const int cur = C.cur, prop = cur ^ 1;
    C.haveMomentum = false;                                  // consumed, whatever happens
    // the gradient the last decision left on the device is the start gradient only if nothing has evaluated on the context since
    const int startGrad = (C.gen == ctx->stateGen && ctx->lfHaveGrad) ? C.nextStart : 0;
    C.nextStart = 0;
    HIPCHK(hipMemcpyAsync(C.d_m[prop], C.d_m[cur], sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    ctx->lfHaveGrad = false;
    int evals = 0;
    rc = leapfrog_core(ctx, C.d_m[prop], C.d_p, C.dt, L, C.regParam, C.lo, C.hi, startGrad, C.d_pred[prop], C.d_scal + CH_D1, &evals);
    if (rc) return chain_fail(ctx, rc);
    const bool wm = ctx->mass.kind == HMCMT_MASS_WM;
    if (wm && (rc = mass_apply_dev(ctx, HMCMT_MASS_OP_INV, C.d_p, ctx->mass.d_x))) return chain_fail(ctx, rc);
    hipLaunchKernelGGL(k_chain_kinetic, dim3(LFNB), dim3(256), 0, st, n, C.d_p, wm ? ctx->mass.d_x : nullptr, ctx->d_invM, C.d_part + LFNB);
    hipLaunchKernelGGL(k_chain_final, dim3(1), dim3(1), 0, st, C.d_part, C.d_part + LFNB, ctx->d_lfScal, ctx->d_lfFlag, C.d_scal);
    HIPCHK(hipMemcpyAsync(C.h_rec, C.d_scal, sizeof(double) * CHAIN_REC, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                        // the step's one wait
    HIPCHK(hipGetLastError());
    prof_collect(ctx);
    if ((rc = leapfrog_flag(ctx))) return chain_fail(ctx, rc);
    const double K0 = C.h_rec[CH_K0], K1 = C.h_rec[CH_K1], D1 = C.h_rec[CH_D1], M1 = C.h_rec[CH_M1];
    if (C.h_rec[CH_FLAG] != 0.0 || !std::isfinite(K1) || !std::isfinite(D1) || !std::isfinite(M1)) {
        ctx->err = "non-finite model value or Hamiltonian term at the proposal";
        return chain_fail(ctx, HMCMT_EBREAKDOWN);
    }
    ctx->lfHaveGrad = true;
    const double hdif = (C.D + C.M + K0) - (D1 + K1 + M1);
    const bool accepted = hdif > 0 || u < std::exp(hdif);
    if (accepted) { C.cur = prop; C.D = D1; C.M = M1; }
    C.nextStart = accepted ? 1 : 2;
    // the commit: enqueued, not waited for
    ++C.nsamples;
    if (C.nsamples > C.burnin) {
        ++C.nmoments;
        hipLaunchKernelGGL(k_chain_welford, dim3((n + 255) / 256), dim3(256), 0, st, n, C.d_m[C.cur], C.d_mean, C.d_m2, (double)C.nmoments);
        if (C.hist.on) {
            ++C.hist.count;
            hipLaunchKernelGGL(k_chain_hist, dim3((unsigned)((C.hist.ntarget + 255) / 256)), dim3(256), 0, st, C.hist.ntarget, C.hist.nbins,
                               C.hist.lo, C.hist.scale, C.d_m[C.cur], C.hist.d_target, C.hist.d_counts);
        }
        if (C.dmom.on && nData > 0) {
            ++C.dmom.count;
            hipLaunchKernelGGL(k_chain_welford, dim3((2 * nData + 255) / 256), dim3(256), 0, st, 2 * nData, C.d_pred[C.cur], C.dmom.d_mean,
                               C.dmom.d_m2, (double)C.dmom.count);
        }
        if (C.acov.on) {
            auto& A = C.acov;                                // (the commit's number t is the count before it: t = 0 sets the pivot)
            bool timed = false;
            if (A.timing) {                                  // (measurement only: the next pair of the pool, grown as needed)
                if (A.pending.size() >= 1024) chain_acov_time_collect(ctx);
                const size_t i = A.pending.size();
                while (A.ev.size() < 2 * i + 2) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); break; } A.ev.push_back(e); }
                timed = A.ev.size() >= 2 * i + 2;
                if (timed) hipEventRecord(A.ev[2 * i], st);
            }
            hipLaunchKernelGGL(k_chain_acov, dim3((unsigned)((A.ntarget + 255) / 256), (unsigned)(A.K / CHAIN_ACOV_RUN + 1)), dim3(256), 0, st,
                               A.ntarget, A.K, A.count, C.d_m[C.cur], A.d_target, A.d_x0, A.d_tot, A.d_S, A.d_H, A.d_ring);
            if (timed) { hipEventRecord(A.ev[2 * A.pending.size() + 1], st); A.pending.push_back(A.count >= A.K ? 1 : 0); }
            ++A.count;
        }
        if (C.cov.on) {
            auto& V = C.cov;                                 // (t = the count before this commit; the slot = the commits parked so far)
            const bool timed = chain_cov_time_start(ctx);
            hipLaunchKernelGGL(k_chain_cov_commit, dim3((n + 255) / 256), dim3(256), 0, st, (long long)n, V.count, V.npend, C.d_m[C.cur],
                               V.d_x0, V.d_tot, V.d_q, V.d_pend);
            if (timed) chain_cov_time_stop(ctx, 0);
            ++V.count;
            if (++V.npend == V.B) chain_cov_flush(ctx);
        }
    }
    C.gen = ctx->stateGen;
    rec->accepted = accepted ? 1 : 0;
    rec->nfevals = evals - (startGrad != 0 ? 1 : 0);
    rec->K0 = K0; rec->K1 = K1; rec->D1 = D1; rec->M1 = M1;
    rec->D = C.D; rec->M = C.M; rec->hdif = hdif;
    rec->nsamples = C.nsamples; rec->nmoments = C.nmoments;
    if (m_out || pred_out) {
        if (m_out) HIPCHK(hipMemcpyAsync(m_out, C.d_m[C.cur], sizeof(double) * n, hipMemcpyDeviceToHost, st));
        if (pred_out) HIPCHK(hipMemcpyAsync(pred_out, C.d_pred[C.cur], sizeof(double) * 2 * nData, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int hmcmt_chain_set_energy(hmcmt_ctx* ctx, double D, double M) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_chain_set_energy", true);
    if (rc) return rc;
    if (!std::isfinite(D) || !std::isfinite(M)) { ctx->err = "hmcmt_chain_set_energy: non-finite value"; return HMCMT_EINVAL; }
    ctx->chain.D = D;
    ctx->chain.M = M;
    return 0;
}

int hmcmt_chain_state(hmcmt_ctx* ctx, double* m_cur, double* p_cur, double* pred_cur) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_chain_state", true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    auto& C = ctx->chain;
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    hipStream_t st = ctx->stream;
    if (m_cur) HIPCHK(hipMemcpyAsync(m_cur, C.d_m[C.cur], sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (p_cur) HIPCHK(hipMemcpyAsync(p_cur, C.d_p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (pred_cur) HIPCHK(hipMemcpyAsync(pred_cur, C.d_pred[C.cur], sizeof(double) * 2 * nData, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int hmcmt_chain_moments(hmcmt_ctx* ctx, int64_t* count, double* mean, double* m2, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_chain_moments", true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    auto& C = ctx->chain;
    const size_t bytes = sizeof(double) * ctx->v.nAC;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (mean) HIPCHK(hipMemcpyAsync(mean, C.d_mean, bytes, kind, ctx->stream));
    if (m2) HIPCHK(hipMemcpyAsync(m2, C.d_m2, bytes, kind, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (count) *count = C.nmoments;
    return 0;
}

// ---- the commit's optional accumulators: histograms of the model, moments of the predicted data ------------------------------------
static int chain_acc_alloc(hmcmt_ctx* ctx, const char* fn, void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        ctx->err = std::string(fn) + ": device allocation failed: " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? HMCMT_ENOMEM : HMCMT_EHIP;
    }
    return 0;
}

int hmcmt_chain_hist_begin(hmcmt_ctx* ctx, int64_t ntarget, const int64_t* target, int32_t nbins, double lo, double hi) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_hist_begin", true);
    if (rc) return rc;
    if (!target || ntarget < 1 || nbins < 1 || nbins > CHAIN_HIST_MAXBINS || !std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo) ||
        !std::isfinite(hi - lo)) {
        ctx->err = "hmcmt_chain_hist_begin: need target, ntarget >= 1, 1 <= nbins <= 4096 and finite lo < hi";
        return HMCMT_EINVAL;
    }
    const int n = ctx->v.nAC;
    for (int64_t i = 0; i < ntarget; ++i)
        if (target[i] < 0 || target[i] >= n) {
            ctx->err = "hmcmt_chain_hist_begin: target " + std::to_string(i) + " = " + std::to_string(target[i]) + " is no active cell (0.." +
                       std::to_string(n - 1) + ")";
            return HMCMT_EINVAL;
        }
    HIPCHK(hipSetDevice(ctx->device));
    auto& C = ctx->chain;
    auto& H = C.hist;
    hipStream_t st = ctx->stream;
    HIPCHK(hipStreamSynchronize(st));                        // (a commit may still be counting into the histogram this one replaces)
    for (void* p : {(void*)H.d_target, (void*)H.d_counts}) if (p) hipFree(p);
    H = hmcmt_ctx::Chain::Hist{};
    const size_t nb = (size_t)ntarget * sizeof(long long), cb = (size_t)ntarget * (size_t)nbins * sizeof(unsigned int);
    auto build = [&]() -> int {
        int r;
        if ((r = chain_acc_alloc(ctx, "hmcmt_chain_hist_begin", (void**)&H.d_target, nb))) return r;
        if ((r = chain_acc_alloc(ctx, "hmcmt_chain_hist_begin", (void**)&H.d_counts, cb))) return r;
        static_assert(sizeof(long long) == sizeof(int64_t), "the target list is uploaded as it is");
        HIPCHK(hipMemcpyAsync(H.d_target, target, nb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(H.d_counts, 0, cb, st));
        HIPCHK(hipStreamSynchronize(st));                    // (the caller's list is free again on return)
        return 0;
    };
    if ((rc = build())) {
        for (void* p : {(void*)H.d_target, (void*)H.d_counts}) if (p) hipFree(p);
        H = hmcmt_ctx::Chain::Hist{};
        return rc;
    }
    H.ntarget = ntarget; H.nbins = nbins; H.lo = lo; H.hi = hi;
    H.scale = (double)nbins / (hi - lo);
    H.w = (hi - lo) / (double)nbins;
    H.count = 0;
    H.on = true;
    return 0;
}

int hmcmt_chain_hist(hmcmt_ctx* ctx, int64_t* count, uint32_t* counts, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_chain_hist", true);
    if (rc) return rc;
    auto& H = ctx->chain.hist;
    if (!H.on) { ctx->err = "hmcmt_chain_hist: no histogram (hmcmt_chain_hist_begin first)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long long total = H.ntarget * H.nbins;
    if (counts && on_device) {
        hipLaunchKernelGGL(k_chain_hist_out, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, H.ntarget, H.nbins, H.d_counts, counts);
        HIPCHK(hipGetLastError());
    } else if (counts) {
        // bin-major on the device, target-major for the caller: turned here, no second device array
        std::vector<unsigned int> tmp;
        try { tmp.resize((size_t)total); } catch (const std::bad_alloc&) { ctx->err = "hmcmt_chain_hist: host allocation failed"; return HMCMT_ENOMEM; }
        HIPCHK(hipMemcpyAsync(tmp.data(), H.d_counts, sizeof(unsigned int) * (size_t)total, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (long long r0 = 0; r0 < H.ntarget; r0 += 256) {   // (in blocks of rows: the strided side stays in cache)
            const long long r1 = std::min(r0 + 256, H.ntarget);
            for (int b = 0; b < H.nbins; ++b) {
                const unsigned int* src = tmp.data() + (size_t)b * H.ntarget;
                for (long long r = r0; r < r1; ++r) counts[(size_t)r * H.nbins + b] = src[r];
            }
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    if (count) *count = H.count;
    return 0;
}

int hmcmt_chain_hist_quantiles(hmcmt_ctx* ctx, int32_t nq, const double* q, double* out, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_hist_quantiles", true);
    if (rc) return rc;
    auto& H = ctx->chain.hist;
    if (!H.on) { ctx->err = "hmcmt_chain_hist_quantiles: no histogram (hmcmt_chain_hist_begin first)"; return HMCMT_EINVAL; }
    if (!q || !out || nq < 1) { ctx->err = "hmcmt_chain_hist_quantiles: need q, out and nq >= 1"; return HMCMT_EINVAL; }
    for (int i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) { ctx->err = "hmcmt_chain_hist_quantiles: every q must lie in [0, 1]"; return HMCMT_EINVAL; }
    if (H.count == 0) { ctx->err = "hmcmt_chain_hist_quantiles: the histogram is empty (no commit behind the burn-in yet)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<double> x((size_t)nq);
    for (int i = 0; i < nq; ++i) x[i] = q[i] * (double)H.count;       // (one product: what a host restatement forms)
    double *d_x = nullptr, *d_out = nullptr;
    const size_t ob = sizeof(double) * (size_t)nq * (size_t)H.ntarget;
    auto run = [&]() -> int {
        int r;
        if ((r = chain_acc_alloc(ctx, "hmcmt_chain_hist_quantiles", (void**)&d_x, sizeof(double) * nq))) return r;
        if (!on_device && (r = chain_acc_alloc(ctx, "hmcmt_chain_hist_quantiles", (void**)&d_out, ob))) return r;
        double* dst = on_device ? out : d_out;
        HIPCHK(hipMemcpyAsync(d_x, x.data(), sizeof(double) * nq, hipMemcpyHostToDevice, st));
        for (int q0 = 0; q0 < nq; q0 += 32768) {             // (a grid's y extent)
            const int nc = std::min(nq - q0, 32768);
            hipLaunchKernelGGL(k_chain_quantiles, dim3((unsigned)((H.ntarget + 255) / 256), (unsigned)nc), dim3(256), 0, st, H.ntarget, H.nbins,
                               nc, H.lo, H.w, d_x + q0, H.d_counts, dst + (size_t)q0 * H.ntarget);
        }
        HIPCHK(hipGetLastError());
        if (!on_device) HIPCHK(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    if (d_x) hipFree(d_x);
    if (d_out) hipFree(d_out);
    return rc;
}

int hmcmt_chain_data_moments_begin(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_data_moments_begin", true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    auto& M = ctx->chain.dmom;
    hipStream_t st = ctx->stream;
    const size_t bytes = sizeof(double) * std::max<size_t>((size_t)2 * ctx->v.nData, 1);
    M.on = false;
    if (!M.d_mean && (rc = chain_acc_alloc(ctx, "hmcmt_chain_data_moments_begin", (void**)&M.d_mean, bytes))) return rc;
    if (!M.d_m2 && (rc = chain_acc_alloc(ctx, "hmcmt_chain_data_moments_begin", (void**)&M.d_m2, bytes))) return rc;
    HIPCHK(hipMemsetAsync(M.d_mean, 0, bytes, st));          // (behind a commit that may still be running on them)
    HIPCHK(hipMemsetAsync(M.d_m2, 0, bytes, st));
    M.count = 0;
    M.on = true;
    return 0;
}

int hmcmt_chain_data_moments(hmcmt_ctx* ctx, int64_t* count, double* mean, double* m2, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_chain_data_moments", true);
    if (rc) return rc;
    auto& M = ctx->chain.dmom;
    if (!M.on) { ctx->err = "hmcmt_chain_data_moments: no data moments (hmcmt_chain_data_moments_begin first)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * 2 * ctx->v.nData;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (mean) HIPCHK(hipMemcpyAsync(mean, M.d_mean, bytes, kind, ctx->stream));
    if (m2) HIPCHK(hipMemcpyAsync(m2, M.d_m2, bytes, kind, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (count) *count = M.count;
    return 0;
}

// ---- lagged autocovariances and the effective sample size (k_chain_acov, k_chain_acov_out, k_chain_ess) ----------------------------
static void chain_acov_free(hmcmt_ctx* ctx) {
    auto& A = ctx->chain.acov;
    chain_acov_time_free(ctx);
    for (void* p : {(void*)A.d_target, (void*)A.d_x0, (void*)A.d_tot, (void*)A.d_S, (void*)A.d_H, (void*)A.d_ring}) if (p) hipFree(p);
    A = hmcmt_ctx::Chain::Acov{};
}

int hmcmt_chain_acov_begin(hmcmt_ctx* ctx, int64_t ntarget, const int64_t* target, int32_t maxlag) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_acov_begin", true);
    if (rc) return rc;
    const int n = ctx->v.nAC;
    const bool all = !target && ntarget == 0;
    if ((!all && (!target || ntarget < 1)) || maxlag < 1 || maxlag > CHAIN_ACOV_MAXLAG) {
        ctx->err = "hmcmt_chain_acov_begin: need target and ntarget >= 1 (or NULL and 0: every active cell) and 1 <= maxlag <= 1023";
        return HMCMT_EINVAL;
    }
    for (int64_t i = 0; i < ntarget; ++i)
        if (target[i] < 0 || target[i] >= n) {
            ctx->err = "hmcmt_chain_acov_begin: target " + std::to_string(i) + " = " + std::to_string(target[i]) + " is no active cell (0.." +
                       std::to_string(n - 1) + ")";
            return HMCMT_EINVAL;
        }
    HIPCHK(hipSetDevice(ctx->device));
    auto& A = ctx->chain.acov;
    hipStream_t st = ctx->stream;
    HIPCHK(hipStreamSynchronize(st));                        // (a commit may still be adding to the accumulator this one replaces)
    chain_acov_free(ctx);
    const long long nt = all ? n : ntarget;
    const size_t tb = (size_t)nt * sizeof(long long), vb = (size_t)nt * sizeof(double), lb = vb * (size_t)(maxlag + 1);
    auto build = [&]() -> int {
        int r;
        if (!all && (r = chain_acc_alloc(ctx, "hmcmt_chain_acov_begin", (void**)&A.d_target, tb))) return r;
        const std::pair<double**, size_t> bufs[] = {{&A.d_x0, vb}, {&A.d_tot, vb}, {&A.d_S, lb}, {&A.d_H, lb}, {&A.d_ring, lb}};
        for (const auto& b : bufs) {
            if ((r = chain_acc_alloc(ctx, "hmcmt_chain_acov_begin", (void**)b.first, b.second))) return r;
            HIPCHK(hipMemsetAsync(*b.first, 0, b.second, st));
        }
        if (!all) HIPCHK(hipMemcpyAsync(A.d_target, target, tb, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));                    // (the caller's list is free again on return)
        return 0;
    };
    if ((rc = build())) {
        (void)hipStreamSynchronize(st);
        chain_acov_free(ctx);
        return rc;
    }
    A.ntarget = nt; A.K = maxlag; A.count = 0;
    A.on = true;
    return 0;
}

// mean and acov into device pointers (each may be nullptr), enqueued
static void chain_acov_launch(hmcmt_ctx* ctx, double* d_mean, double* d_acov) {
    auto& A = ctx->chain.acov;
    hipLaunchKernelGGL(k_chain_acov_out, dim3((unsigned)((A.ntarget + 255) / 256)), dim3(256), 0, ctx->stream,
                       A.ntarget, A.K, A.count, A.d_x0, A.d_tot, A.d_S, A.d_H, A.d_ring, d_mean, d_acov);
}

int hmcmt_chain_acov(hmcmt_ctx* ctx, int64_t* count, double* mean, double* acov, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_acov", true);
    if (rc) return rc;
    auto& A = ctx->chain.acov;
    if (!A.on) { ctx->err = "hmcmt_chain_acov: no autocovariances (hmcmt_chain_acov_begin first)"; return HMCMT_EINVAL; }
    if ((mean || acov) && A.count == 0) { ctx->err = "hmcmt_chain_acov: the accumulator is empty (no commit behind the burn-in yet)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t mb = sizeof(double) * (size_t)A.ntarget, ab = mb * (size_t)(A.K + 1);
    double *d_mean = nullptr, *d_acov = nullptr;
    auto run = [&]() -> int {
        int r;
        if (!mean && !acov) return 0;
        if (on_device) { d_mean = mean; d_acov = acov; }
        else {
            if (mean && (r = chain_acc_alloc(ctx, "hmcmt_chain_acov", (void**)&d_mean, mb))) return r;
            if (acov && (r = chain_acc_alloc(ctx, "hmcmt_chain_acov", (void**)&d_acov, ab))) return r;
        }
        chain_acov_launch(ctx, d_mean, d_acov);
        HIPCHK(hipGetLastError());
        if (!on_device) {
            if (mean) HIPCHK(hipMemcpyAsync(mean, d_mean, mb, hipMemcpyDeviceToHost, st));
            if (acov) HIPCHK(hipMemcpyAsync(acov, d_acov, ab, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    if (!on_device) { if (d_mean) hipFree(d_mean); if (d_acov) hipFree(d_acov); }
    if (!rc && count) *count = A.count;
    return rc;
}

int hmcmt_chain_ess(hmcmt_ctx* ctx, double* tau, double* ess, int32_t* window, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_ess", true);
    if (rc) return rc;
    auto& A = ctx->chain.acov;
    if (!A.on) { ctx->err = "hmcmt_chain_ess: no autocovariances (hmcmt_chain_acov_begin first)"; return HMCMT_EINVAL; }
    if (A.count == 0) { ctx->err = "hmcmt_chain_ess: the accumulator is empty (no commit behind the burn-in yet)"; return HMCMT_EINVAL; }
    if (!tau && !ess && !window) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t mb = sizeof(double) * (size_t)A.ntarget, ab = mb * (size_t)(A.K + 1), wb = sizeof(int) * (size_t)A.ntarget;
    const double lg = std::max(1.0, std::log10((double)A.count));
    double *d_acov = nullptr, *d_tau = nullptr, *d_ess = nullptr;
    int* d_win = nullptr;
    static_assert(sizeof(int) == sizeof(int32_t), "window is written as int");
    auto run = [&]() -> int {
        int r;
        if ((r = chain_acc_alloc(ctx, "hmcmt_chain_ess", (void**)&d_acov, ab))) return r;
        if (on_device) { d_tau = tau; d_ess = ess; d_win = (int*)window; }
        else {
            if (tau && (r = chain_acc_alloc(ctx, "hmcmt_chain_ess", (void**)&d_tau, mb))) return r;
            if (ess && (r = chain_acc_alloc(ctx, "hmcmt_chain_ess", (void**)&d_ess, mb))) return r;
            if (window && (r = chain_acc_alloc(ctx, "hmcmt_chain_ess", (void**)&d_win, wb))) return r;
        }
        chain_acov_launch(ctx, nullptr, d_acov);
        hipLaunchKernelGGL(k_chain_ess, dim3((unsigned)((A.ntarget + 255) / 256)), dim3(256), 0, st, A.ntarget, A.K, A.count,
                           (double)A.count * lg, 1.0 / lg, d_acov, d_tau, d_ess, d_win);
        HIPCHK(hipGetLastError());
        if (!on_device) {
            if (tau) HIPCHK(hipMemcpyAsync(tau, d_tau, mb, hipMemcpyDeviceToHost, st));
            if (ess) HIPCHK(hipMemcpyAsync(ess, d_ess, mb, hipMemcpyDeviceToHost, st));
            if (window) HIPCHK(hipMemcpyAsync(window, d_win, wb, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    if (d_acov) hipFree(d_acov);
    if (!on_device) { if (d_tau) hipFree(d_tau); if (d_ess) hipFree(d_ess); if (d_win) hipFree(d_win); }
    return rc;
}

// measurement only (include/hmcmt_debug.h)
int hmcmt_debug_chain_acov_time(hmcmt_ctx* ctx, int32_t enable, double* ms, int64_t* launches) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_debug_chain_acov_time", true);
    if (rc) return rc;
    auto& A = ctx->chain.acov;
    if (!A.on) { ctx->err = "hmcmt_debug_chain_acov_time: no autocovariances (hmcmt_chain_acov_begin first)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    chain_acov_time_collect(ctx);
    for (int i = 0; i < 2; ++i) {
        if (ms) ms[i] = A.ms[i];
        if (launches) launches[i] = A.launches[i];
    }
    if (enable >= 0) {                                       // (the sums up to here went out; a switch starts new ones)
        A.timing = enable != 0;
        for (int i = 0; i < 2; ++i) { A.ms[i] = 0; A.launches[i] = 0; }
    }
    return 0;
}

// ---- posterior covariance and correlation (k_chain_cov_commit, k_chain_cov_flush, k_chain_cov_out, k_chain_corr) --------------------
static void chain_cov_free(hmcmt_ctx* ctx) {
    auto& V = ctx->chain.cov;
    chain_cov_time_free(ctx);
    for (void* p : {(void*)V.d_row, (void*)V.d_x0, (void*)V.d_tot, (void*)V.d_q, (void*)V.d_pend, (void*)V.d_S}) if (p) hipFree(p);
    V = hmcmt_ctx::Chain::Cov{};
}

int hmcmt_chain_cov_begin(hmcmt_ctx* ctx, int64_t nrow, const int64_t* row, int32_t batch) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_cov_begin", true);
    if (rc) return rc;
    static_assert(CHAIN_COV_BATCH_MAX == HMCMT_COV_BATCH_MAX, "the header's bound is the kernels'");
    const int n = ctx->v.nAC;
    const bool all = !row && nrow == 0;
    if ((!all && (!row || nrow < 1)) || batch < 0 || batch > CHAIN_COV_BATCH_MAX) {
        ctx->err = "hmcmt_chain_cov_begin: need row and nrow >= 1 (or NULL and 0: every active cell) and 1 <= batch <= 16 (0: the default, 8)";
        return HMCMT_EINVAL;
    }
    for (int64_t i = 0; i < nrow; ++i)
        if (row[i] < 0 || row[i] >= n) {
            ctx->err = "hmcmt_chain_cov_begin: row " + std::to_string(i) + " = " + std::to_string(row[i]) + " is no active cell (0.." +
                       std::to_string(n - 1) + ")";
            return HMCMT_EINVAL;
        }
    HIPCHK(hipSetDevice(ctx->device));
    auto& V = ctx->chain.cov;
    hipStream_t st = ctx->stream;
    HIPCHK(hipStreamSynchronize(st));                        // (a commit may still be adding to the accumulator this one replaces)
    chain_cov_free(ctx);
    const long long nr = all ? n : nrow;
    const int B = batch == 0 ? CHAIN_COV_BATCH_DEFAULT : batch;
    const size_t rb = (size_t)nr * sizeof(long long), vb = (size_t)n * sizeof(double);
    auto build = [&]() -> int {
        int r;
        if (!all && (r = chain_acc_alloc(ctx, "hmcmt_chain_cov_begin", (void**)&V.d_row, rb))) return r;
        const std::pair<double**, size_t> bufs[] = {{&V.d_x0, vb}, {&V.d_tot, vb}, {&V.d_q, vb}, {&V.d_pend, vb * (size_t)B}, {&V.d_S, vb * (size_t)nr}};
        for (const auto& b : bufs) {
            if ((r = chain_acc_alloc(ctx, "hmcmt_chain_cov_begin", (void**)b.first, b.second))) return r;
            HIPCHK(hipMemsetAsync(*b.first, 0, b.second, st));
        }
        static_assert(sizeof(long long) == sizeof(int64_t), "the row list is uploaded as it is");
        if (!all) HIPCHK(hipMemcpyAsync(V.d_row, row, rb, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));                    // (the caller's list is free again on return)
        return 0;
    };
    if ((rc = build())) {
        (void)hipStreamSynchronize(st);
        chain_cov_free(ctx);
        return rc;
    }
    V.nrow = nr; V.B = B; V.npend = 0; V.count = 0;
    V.on = true;
    return 0;
}

static dim3 chain_cov_grid(hmcmt_ctx* ctx, long long nrow) {
    return dim3((unsigned)((ctx->v.nAC + 255) / 256), (unsigned)std::min<long long>(nrow, 32768));
}

int hmcmt_chain_cov(hmcmt_ctx* ctx, int64_t* count, double* mean, double* var, double* cov, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_cov", true);
    if (rc) return rc;
    auto& V = ctx->chain.cov;
    if (!V.on) { ctx->err = "hmcmt_chain_cov: no covariance (hmcmt_chain_cov_begin first)"; return HMCMT_EINVAL; }
    if ((mean || var || cov) && V.count == 0) { ctx->err = "hmcmt_chain_cov: the accumulator is empty (no commit behind the burn-in yet)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long long n = ctx->v.nAC;
    const size_t mb = sizeof(double) * (size_t)n, cb = mb * (size_t)V.nrow;
    double *d_mean = nullptr, *d_var = nullptr, *d_cov = nullptr;
    auto run = [&]() -> int {
        int r;
        if (!mean && !var && !cov) return 0;
        if (on_device) { d_mean = mean; d_var = var; d_cov = cov; }
        else {
            if (mean && (r = chain_acc_alloc(ctx, "hmcmt_chain_cov", (void**)&d_mean, mb))) return r;
            if (var && (r = chain_acc_alloc(ctx, "hmcmt_chain_cov", (void**)&d_var, mb))) return r;
            if (cov && (r = chain_acc_alloc(ctx, "hmcmt_chain_cov", (void**)&d_cov, cb))) return r;
        }
        if (cov) chain_cov_flush(ctx);                       // (the parked commits first: the later bits stay what they would have been)
        const long long rows = cov ? V.nrow : 1;             // (row 0's owners write mean and var)
        hipLaunchKernelGGL(k_chain_cov_out, chain_cov_grid(ctx, rows), dim3(256), 0, st, n, rows, (double)V.count, V.d_x0, V.d_tot, V.d_q,
                           V.d_S, V.d_row, d_mean, d_var, d_cov);
        HIPCHK(hipGetLastError());
        if (!on_device) {
            if (mean) HIPCHK(hipMemcpyAsync(mean, d_mean, mb, hipMemcpyDeviceToHost, st));
            if (var) HIPCHK(hipMemcpyAsync(var, d_var, mb, hipMemcpyDeviceToHost, st));
            if (cov) HIPCHK(hipMemcpyAsync(cov, d_cov, cb, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    if (!on_device) { if (d_mean) hipFree(d_mean); if (d_var) hipFree(d_var); if (d_cov) hipFree(d_cov); }
    if (!rc && count) *count = V.count;
    return rc;
}

int hmcmt_chain_corr(hmcmt_ctx* ctx, double* corr, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, "hmcmt_chain_corr", true);
    if (rc) return rc;
    auto& V = ctx->chain.cov;
    if (!V.on) { ctx->err = "hmcmt_chain_corr: no covariance (hmcmt_chain_cov_begin first)"; return HMCMT_EINVAL; }
    if (V.count == 0) { ctx->err = "hmcmt_chain_corr: the accumulator is empty (no commit behind the burn-in yet)"; return HMCMT_EINVAL; }
    if (!corr) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const long long n = ctx->v.nAC;
    const size_t cb = sizeof(double) * (size_t)n * (size_t)V.nrow;
    double* d_corr = nullptr;
    auto run = [&]() -> int {
        int r;
        if (on_device) d_corr = corr;
        else if ((r = chain_acc_alloc(ctx, "hmcmt_chain_corr", (void**)&d_corr, cb))) return r;
        chain_cov_flush(ctx);
        hipLaunchKernelGGL(k_chain_corr, chain_cov_grid(ctx, V.nrow), dim3(256), 0, st, n, V.nrow, (double)V.count, V.d_tot, V.d_q, V.d_S,
                           V.d_row, d_corr);
        HIPCHK(hipGetLastError());
        if (!on_device) HIPCHK(hipMemcpyAsync(corr, d_corr, cb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    if (!on_device && d_corr) hipFree(d_corr);
    return rc;
}

// measurement only (include/hmcmt_debug.h)
int hmcmt_debug_chain_cov_time(hmcmt_ctx* ctx, int32_t enable, double* ms, int64_t* launches) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_debug_chain_cov_time", true);
    if (rc) return rc;
    auto& V = ctx->chain.cov;
    if (!V.on) { ctx->err = "hmcmt_debug_chain_cov_time: no covariance (hmcmt_chain_cov_begin first)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->device));
    chain_cov_time_collect(ctx);
    for (int i = 0; i < 2; ++i) {
        if (ms) ms[i] = V.ms[i];
        if (launches) launches[i] = V.launches[i];
    }
    if (enable >= 0) {                                       // (the sums up to here went out; a switch starts new ones)
        V.timing = enable != 0;
        for (int i = 0; i < 2; ++i) { V.ms[i] = 0; V.launches[i] = 0; }
    }
    return 0;
}

int hmcmt_chain_end(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    if (ctx->statsPending) { ctx->err = "hmcmt_chain_end: an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    chain_release(ctx);
    return 0;
}
