// host_chain.h -- the device-resident HMC chain behind hmcmt_chain_* (include/hmcmt.h): host code of hmcmt_hip.hip's translation
// unit, included at the end of its extern "C" block (behind leapfrog_core and mass_apply_dev); kernels in kernels_chain.h.
//
// One sample = hmcmt_chain_momentum + hmcmt_chain_step.  What crosses PCIe per sample: nAC normals up, LFNB partial sums and
// CHAIN_REC scalars down; with outputs, nAC + 2 nData doubles more.  Launches per sample beyond leapfrog_core's (diagonal mass):
// k_chain_momentum, k_chain_kinetic, k_chain_final, k_chain_welford.

static void chain_release(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
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
    if (reuse) C.active = C.haveMomentum = false;
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

int hmcmt_chain_end(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    if (ctx->statsPending) { ctx->err = "hmcmt_chain_end: an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    chain_release(ctx);
    return 0;
}
