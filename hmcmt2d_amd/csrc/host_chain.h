// host_chain.h -- the device-resident HMC chain behind hmcmt_chain_* (include/hmcmt.h): host code of hmcmt_hip.hip's translation
// unit, included at the end of its extern "C" block (behind leapfrog_core and mass_apply_dev); kernels in kernels_chain.h.
//
// One sample = hmcmt_chain_momentum + hmcmt_chain_step.  What crosses PCIe per sample: nAC normals up, LFNB partial sums and
// CHAIN_REC scalars down; with outputs, nAC + 2 nData doubles more.  A seeded chain (hmcmt_chain_seed) draws its numbers itself:
// one sample = hmcmt_chain_sample, k_chain_draw_momentum in k_chain_momentum's place, nothing up, CHAIN_REC scalars down, one wait.  Launches per sample beyond leapfrog_core's (diagonal mass):
// k_chain_momentum, k_chain_kinetic, k_chain_final, k_chain_welford; with the optional accumulators of the commit on,
// k_chain_hist, a second k_chain_welford (the predicted data), k_chain_acov (lagged autocovariances) and k_chain_cov_commit (cross
// moments; every `batch` commits k_chain_cov_flush) and k_chain_sketch_commit (the row sketch; every ell commits k_chain_sketch_gram,
// a wait for its 2 ell x 2 ell result and k_chain_sketch_shrink) behind them.  During a warm-up (hmcmt_chain_adapt_*) a k_chain_welford on the
// window's buffers inside a window and k_chain_adapt_mass at a window's end follow the commit.  A NUTS sample (hmcmt_chain_nuts_sample,
// kernels_nuts.h) chooses its trajectory length: per leaf leapfrog_core(L = 1) with its wait for the solver records, k_nuts_leaf, k_nuts_final,
// NUTS_SCAL scalars down and one wait more; it ends in the same commit.
//
// The accumulators share their host scaffolding, which stands in front of them: ChainTimer (the event pairs of the measurement
// hooks), chain_acc_alloc / chain_acc_free (each accumulator's struct owns its buffers through `allocs`), chain_acc_ready (the
// guards of an entry point), chain_cell_list / chain_cell_upload (a begin's list of active cells) and ChainReadout (the outputs of
// one read-out: the caller's device pointers, or temporaries copied back).  A further accumulator is its kernels, its struct in
// hmcmt_ctx::Chain, its launch in hmcmt_chain_step's commit, a line in chain_acc_release, and a begin and a read-out written with these.

// what every chain call checks first
static int chain_ready(hmcmt_ctx* ctx, const char* fn, bool needChain) {
    if (ctx->statsPending) { ctx->err = std::string(fn) + ": an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    if (needChain && !ctx->chain.active) {
        ctx->err = std::string(fn) + ": no chain (hmcmt_chain_begin first; hmcmt_set_prior and hmcmt_set_mass end a chain)";
        return HMCMT_EINVAL;
    }
    return 0;
}

// ---- what the accumulators share: the timer, the owner of their buffers, the guards of their entry points, the read-out ------------
// the first event of the next pair of the pool, recorded (false: not timing, or no event to be had); stop closes the pair
bool ChainTimer::start(hipStream_t st) {
    if (!timing) return false;
    if (pending.size() >= 1024) collect(st);
    const size_t i = pending.size();
    while (ev.size() < 2 * i + 2) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return false; } ev.push_back(e); }
    hipEventRecord(ev[2 * i], st);
    return true;
}
void ChainTimer::stop(hipStream_t st, int cls) {
    hipEventRecord(ev[2 * pending.size() + 1], st);
    pending.push_back(cls);
}
void ChainTimer::collect(hipStream_t st) {
    if (pending.empty()) return;
    (void)hipStreamSynchronize(st);
    for (size_t i = 0; i < pending.size(); ++i) {
        float t = 0;
        if (hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) == hipSuccess) { ms[pending[i]] += t; launches[pending[i]] += 1; }
    }
    pending.clear();
}
void ChainTimer::free(int device, hipStream_t st) {
    if (ev.empty()) return;
    hipSetDevice(device);
    if (st) (void)hipStreamSynchronize(st);
    for (hipEvent_t e : ev) hipEventDestroy(e);
    ev.clear(); pending.clear();
    timing = false;
}
// the sums since the last switch go out; enable = 1 / 0 switches and starts new ones, -1 only reads
void ChainTimer::report(hipStream_t st, int enable, double* msOut, int64_t* launchesOut) {
    collect(st);
    for (int i = 0; i < 2; ++i) {
        if (msOut) msOut[i] = ms[i];
        if (launchesOut) launchesOut[i] = launches[i];
    }
    if (enable >= 0) {
        timing = enable != 0;
        for (int i = 0; i < 2; ++i) { ms[i] = 0; launches[i] = 0; }
    }
}

// a device buffer that `owner` (an accumulator's allocs, a read-out's) frees
static int chain_acc_alloc(hmcmt_ctx* ctx, const char* fn, std::vector<void*>& owner, void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        ctx->err = std::string(fn) + ": device allocation failed: " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? HMCMT_ENOMEM : HMCMT_EHIP;
    }
    owner.push_back(*p);
    return 0;
}
// ... zeroed (enqueued)
static int chain_acc_zeroed(hmcmt_ctx* ctx, const char* fn, std::vector<void*>& owner, void** p, size_t bytes) {
    const int rc = chain_acc_alloc(ctx, fn, owner, p, bytes);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(*p, 0, bytes, ctx->stream));
    return 0;
}
// frees an accumulator's buffers (the caller resets it: X = {}); the caller has made sure that no commit still runs on them
static void chain_acc_free(std::vector<void*>& allocs) {
    for (void* p : allocs) hipFree(p);
    allocs.clear();
}

// what the messages call an accumulator
struct ChainAccName { const char *noun, *begin, *empty; };
static const ChainAccName CHAIN_HIST = {"histogram", "hmcmt_chain_hist_begin", "the histogram"},
                          CHAIN_DMOM = {"data moments", "hmcmt_chain_data_moments_begin", "the accumulator"},
                          CHAIN_ACOV = {"autocovariances", "hmcmt_chain_acov_begin", "the accumulator"},
                          CHAIN_COV = {"covariance", "hmcmt_chain_cov_begin", "the accumulator"};
// what a call on a running accumulator checks first: chain_ready, that it runs, and (needCommits) that it has counted a commit
static int chain_acc_ready(hmcmt_ctx* ctx, const char* fn, bool on, long long count, bool needCommits, const ChainAccName& name) {
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    if (!on) { ctx->err = std::string(fn) + ": no " + name.noun + " (" + name.begin + " first)"; return HMCMT_EINVAL; }
    if (needCommits && count == 0) { ctx->err = std::string(fn) + ": " + name.empty + " is empty (no commit behind the burn-in yet)"; return HMCMT_EINVAL; }
    return 0;
}

// the "list of active cells" argument of a begin (`what`: "target" / "row"): *count = the list's length, or with allowAll the number
// of active cells for NULL and 0.  `need`, the call's requirement sentence, is the error where the list's shape or the call's other
// arguments (restOk) miss it.
static int chain_cell_list(hmcmt_ctx* ctx, const char* fn, const char* what, int64_t n, const int64_t* list, bool allowAll, bool restOk,
                           const char* need, long long* count) {
    const int nAC = ctx->v.nAC;
    const bool all = allowAll && !list && n == 0;
    if ((!all && (!list || n < 1)) || !restOk) { ctx->err = std::string(fn) + ": need " + need; return HMCMT_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        if (list[i] < 0 || list[i] >= nAC) {
            ctx->err = std::string(fn) + ": " + what + " " + std::to_string(i) + " = " + std::to_string(list[i]) + " is no active cell (0.." +
                       std::to_string(nAC - 1) + ")";
            return HMCMT_EINVAL;
        }
    *count = all ? nAC : n;
    return 0;
}
// the list's device copy, owned by `owner` (enqueued: the caller waits before it returns); NULL, every cell, has none
static int chain_cell_upload(hmcmt_ctx* ctx, const char* fn, std::vector<void*>& owner, long long** d_list, const int64_t* list, long long n) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the list is uploaded as it is");
    if (!list) return 0;
    const int rc = chain_acc_alloc(ctx, fn, owner, (void**)d_list, (size_t)n * sizeof(long long));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(*d_list, list, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

// One read-out's outputs.  out(): the device pointer to launch into for an output of the caller's -- the caller's own with on_device
// (nullptr where it passed none), else a temporary that finish() copies back; scratch(): a device-only temporary.  A failed
// allocation leaves rc (and nullptr, as every later call does).  finish(): the launches' status, the copies back, one wait.  Left
// without a finish() that succeeded, it waits for the stream first; it frees what it allocated, never a pointer of the caller's.
struct ChainReadout {
    hmcmt_ctx* ctx;
    const char* fn;
    bool onDevice, done = false;
    int rc = 0, nback = 0;
    std::vector<void*> allocs;
    struct { void *host, *dev; size_t bytes; } back[3];
    ChainReadout(hmcmt_ctx* c, const char* f, bool dev) : ctx(c), fn(f), onDevice(dev) {}
    ChainReadout(const ChainReadout&) = delete;
    void* scratch(size_t bytes) {
        void* p = nullptr;
        if (!rc) rc = chain_acc_alloc(ctx, fn, allocs, &p, bytes);
        return p;
    }
    void* out(void* caller, size_t bytes) {
        if (onDevice || !caller) return caller;
        void* p = scratch(bytes);
        if (p) back[nback++] = {caller, p, bytes};
        return p;
    }
    int finish() {
        HIPCHK(hipGetLastError());
        for (int i = 0; i < nback; ++i) HIPCHK(hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        done = true;
        return 0;
    }
    ~ChainReadout() {
        if (!done) (void)hipStreamSynchronize(ctx->stream);
        for (void* p : allocs) hipFree(p);
    }
};

// the Welford read-out of hmcmt_chain_moments and hmcmt_chain_data_moments: two copies, one wait
static int chain_welford_out(hmcmt_ctx* ctx, size_t bytes, const double* d_mean, const double* d_m2, double* mean, double* m2, int32_t on_device) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (mean) HIPCHK(hipMemcpyAsync(mean, d_mean, bytes, kind, ctx->stream));
    if (m2) HIPCHK(hipMemcpyAsync(m2, d_m2, bytes, kind, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// folds the parked commits into S (enqueued): the commit calls it when the batch is full, a read-out when any is parked
static void chain_cov_flush(hmcmt_ctx* ctx) {
    auto& V = ctx->chain.cov;
    if (V.npend == 0) return;
    const bool timed = V.timer.start(ctx->stream);
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
    if (timed) V.timer.stop(ctx->stream, 1);
    V.npend = 0;
}

// ---- the row sketch's buffers, commit and shrink (hmcmt_chain_sketch_*, hmcmt_debug_chain_sketch; the entry points stand behind
// hmcmt_chain_cov's).  They work on a Sketch of the caller's, so that the debug hook drives the chain's very launches without a chain.
using ChainSketch = hmcmt_ctx::Chain::Sketch;
static const ChainAccName CHAIN_SKETCH = {"sketch", "hmcmt_chain_sketch_begin", "the sketch"};

// ends a sketch and frees its buffers; `why` (may be empty) is what the read-outs say from then on
static void chain_sketch_end(hmcmt_ctx* ctx, ChainSketch& S, const std::string& why) {
    if (!S.allocs.empty() && ctx->stream) (void)hipStreamSynchronize(ctx->stream);    // (a commit may still be writing a row)
    S.timer.free(ctx->cfg.device, ctx->stream);
    chain_acc_free(S.allocs);
    S = {};
    S.ended = why;
}

// the zeroed buffers of hmcmt_chain_sketch_begin in S (which is empty); pivot: nAC host doubles or nullptr
static int chain_sketch_alloc(hmcmt_ctx* ctx, const char* fn, ChainSketch& S, int ell, const double* pivot) {
    const size_t n = (size_t)ctx->v.nAC, D = sizeof(double), rows = (size_t)2 * ell + 1;
    const size_t stage = std::max((size_t)ell * 2 * ell, rows * (size_t)HMCMT_MASS_RANK_MAX);
    const std::pair<double**, size_t> bufs[] = {{&S.d_B, rows * n * D}, {&S.d_x0, n * D}, {&S.d_tot, n * D}, {&S.d_q, n * D},
                                                {&S.d_K, rows * rows * D}, {&S.d_T, stage * D}};
    int rc;
    for (const auto& b : bufs)
        if ((rc = chain_acc_zeroed(ctx, fn, S.allocs, (void**)b.first, b.second))) return rc;
    if (pivot) HIPCHK(hipMemcpyAsync(S.d_x0, pivot, n * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));               // (the caller's pivot is free again on return)
    S.hK.assign(rows * rows, 0.0);
    S.ell = ell; S.fill = 0; S.count = 0; S.shrinks = 0; S.Delta = 0.0;
    S.pivotGiven = pivot != nullptr;
    return 0;
}

// K = W W' of rows 0 .. nrows - 1 of B (and the mean row behind them) into S.d_K, enqueued
static SketchRows chain_sketch_gram(hmcmt_ctx* ctx, const ChainSketch& S, int nrows, bool meanRow) {
    const int nAC = ctx->v.nAC;
    const SketchRows w{nAC, nrows, nrows + (meanRow ? 1 : 0), S.d_B, meanRow ? S.d_B + (size_t)2 * S.ell * nAC : nullptr};
    const int T = (w.nw + ADAPT_LR_TILE - 1) / ADAPT_LR_TILE;
    hipLaunchKernelGGL(k_chain_sketch_gram, dim3(T * (T + 1) / 2), dim3(256), 0, ctx->stream, w, S.d_K);
    return w;
}

// The shrink of a full buffer (fill == 2 ell): the Gram kernel, the shrink's ONE wait with K's download, the host's eigenproblem, T's
// upload, the shrink kernel (enqueued).  K_out [2 ell]^2 / T_out [ell][2 ell]: the debug hook's copies, or nullptr.  Returns 0;
// HMCMT_EHIP behind a HIP error and HMCMT_EBREAKDOWN where the eigensolver gave up -- both have ended the sketch.
static int chain_sketch_shrink(hmcmt_ctx* ctx, ChainSketch& S, double* K_out, double* T_out) {
    hipStream_t st = ctx->stream;
    const int ell = S.ell, n2 = 2 * ell;
    const size_t kb = sizeof(double) * (size_t)n2 * n2;
    auto failed = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return false;
        (void)hipGetLastError();
        ctx->err = std::string("the sketch's shrink: ") + what + ": " + hipGetErrorString(e) + " (the sketch is ended)";
        chain_sketch_end(ctx, S, std::string("a HIP error in a shrink (") + what + ") ended the sketch");
        return true;
    };
    bool timed = S.timer.start(st);
    (void)chain_sketch_gram(ctx, S, n2, false);
    if (timed) S.timer.stop(st, 1);
    if (failed(hipMemcpyAsync(S.hK.data(), S.d_K, kb, hipMemcpyDeviceToHost, st), "the download of K")) return HMCMT_EHIP;
    if (failed(hipStreamSynchronize(st), "the wait for K")) return HMCMT_EHIP;                  // the shrink's wait
    if (K_out) std::memcpy(K_out, S.hK.data(), kb);
    const auto h0 = std::chrono::steady_clock::now();
    std::vector<double>& T = S.hT;                          // (the sketch's: the upload below reads it until the next wait of this stream)
    double delta = 0.0;
    const bool ok = item_chain_sketch_shrink_T(ell, S.hK.data(), T, &delta);
    if (S.timer.timing) S.hostMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    if (!ok) {
        chain_sketch_end(ctx, S, "the eigensolver of a shrink did not converge within its sweeps, or its Gram matrix was not finite: the sketch was ended");
        return HMCMT_EBREAKDOWN;
    }
    if (T_out) std::memcpy(T_out, T.data(), sizeof(double) * T.size());
    if (failed(hipMemcpyAsync(S.d_T, T.data(), sizeof(double) * T.size(), hipMemcpyHostToDevice, st), "the upload of T")) return HMCMT_EHIP;
    const long long n = ctx->v.nAC;
    timed = S.timer.start(st);
    hipLaunchKernelGGL(k_chain_sketch_shrink, dim3((unsigned)((n + CHAIN_SKETCH_COLS - 1) / CHAIN_SKETCH_COLS)), dim3(CHAIN_SKETCH_COLS),
                       sizeof(double) * (size_t)n2 * CHAIN_SKETCH_COLS, st, n, ell, S.d_T, S.d_B);
    if (timed) S.timer.stop(st, 1);
    if (failed(hipGetLastError(), "a kernel launch")) return HMCMT_EHIP;
    S.Delta += delta;
    ++S.shrinks;
    S.fill = ell;
    return 0;
}

// one counted commit of the model d_m: the commit kernel (enqueued) and, when it fills the buffer, the shrink (its results above)
static int chain_sketch_commit(hmcmt_ctx* ctx, ChainSketch& S, const double* d_m, double* K_out, double* T_out) {
    hipStream_t st = ctx->stream;
    const long long n = ctx->v.nAC;
    const bool timed = S.timer.start(st);
    hipLaunchKernelGGL(k_chain_sketch_commit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, S.count, S.pivotGiven ? 1 : 0, d_m,
                       S.d_x0, S.d_tot, S.d_q, S.d_B + (size_t)S.fill * n);
    if (timed) S.timer.stop(st, 0);
    ++S.count;
    if (++S.fill == 2 * S.ell) return chain_sketch_shrink(ctx, S, K_out, T_out);
    return 0;
}

// ends the commit's optional accumulators (histogram, data moments, autocovariances, cross moments, sketch) and frees their buffers
static void chain_acc_release(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
    C.acov.timer.free(ctx->cfg.device, ctx->stream);
    C.cov.timer.free(ctx->cfg.device, ctx->stream);
    if (!C.sketch.allocs.empty()) hipSetDevice(ctx->cfg.device);
    chain_sketch_end(ctx, C.sketch, "");
    if (!C.hist.allocs.empty() || !C.dmom.allocs.empty() || !C.acov.allocs.empty() || !C.cov.allocs.empty() || !C.adapt.allocs.empty()) {
        hipSetDevice(ctx->cfg.device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);      // (a commit may still be counting)
    }
    chain_acc_free(C.hist.allocs); C.hist = {};
    chain_acc_free(C.dmom.allocs); C.dmom = {};
    chain_acc_free(C.acov.allocs); C.acov = {};
    chain_acc_free(C.cov.allocs); C.cov = {};
    chain_acc_free(C.adapt.allocs); C.adapt = {};
}

static void chain_release(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
    chain_acc_release(ctx);
    if (!C.allocs.empty() || C.h_rec || !C.nuts.allocs.empty() || C.nuts.h_scal) {
        hipSetDevice(ctx->cfg.device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);      // (a commit may still be running on the buffers)
        for (void* p : C.allocs) hipFree(p);
        if (C.h_rec) hipHostFree(C.h_rec);
        chain_acc_free(C.nuts.allocs);
        if (C.nuts.h_scal) hipHostFree(C.nuts.h_scal);
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

// ---- low-rank mass in the warm-up (hmcmt_chain_adapt_lowrank; hmcmt.h has the algorithm, kernels_chain.h the kernels) -------------
// a counted step inside a window, behind the Welford kernel: one launch where the step is due, no wait
static void chain_adapt_lr_store(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
    auto& L = C.adapt.lr;
    const int n = ctx->v.nAC;
    const long long i = C.adapt.c - L.winStart;
    if (i < 0 || !item_adapt_lr_due(i, L.stride) || L.stored >= L.opt.max_samples) return;
    // (NOT REACHED in this library: both callers set lfHaveGrad behind their decision, also where a foreign evaluation came between two
    // steps -- the step then evaluated its own start gradient.  Kept so that a future caller without a gradient skips and counts
    // instead of storing a stale one; `skipped` is 0 in every chain that can be run today)
    if (!ctx->lfHaveGrad) { ++L.skipped; return; }
    // the data gradient at the current model: what the next step's start_grad 1 (accepted; a NUTS sample's selection) or 2 (rejected) reuses
    const double* gdata = C.nextStart == 2 ? ctx->d_gStart : ctx->d_g;
    LfView lf{n, ctx->d_mref, ctx->d_invM, ctx->d_wmVal, ctx->d_wmRow, ctx->d_wmCol, C.d_m[C.cur], C.d_p, ctx->d_g,
              ctx->d_lfPart, ctx->d_lfScal, ctx->d_lfFlag, ctx->v.ticks};
    hipLaunchKernelGGL(k_adapt_lr_store, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, lf, gdata, C.regParam,
                       L.d_X + (size_t)L.stored * n, L.d_G + (size_t)L.stored * n);
    ++L.stored;
}

// K = W W' of n rows on the device into d_K (enqueued): the means and s = sqrt(invM), then the tiles of the upper block triangle
static AdaptLr chain_adapt_lr_gram(hipStream_t st, int nAC, int n, const double* d_X, const double* d_G, const double* d_invM, double* d_meanX,
                                   double* d_meanG, double* d_s, double* d_K) {
    const AdaptLr w{nAC, n, std::sqrt((double)(n - 1)), d_X, d_G, d_meanX, d_meanG, d_s};
    hipLaunchKernelGGL(k_adapt_lr_mean, dim3((nAC + 255) / 256), dim3(256), 0, st, nAC, n, d_X, d_G, d_invM, d_meanX, d_meanG, d_s);
    const int T = (2 * n + ADAPT_LR_TILE - 1) / ADAPT_LR_TILE;
    hipLaunchKernelGGL(k_adapt_lr_gram, dim3(T * (T + 1) / 2), dim3(256), 0, st, w, d_K);
    return w;
}
// U = B' W into d_U with the sign convention (enqueued; B is on the device)
static void chain_adapt_lr_lift(hipStream_t st, const AdaptLr& w, const double* d_B, int r, double* d_U) {
    hipLaunchKernelGGL(k_adapt_lr_lift, dim3((w.nAC + 255) / 256), dim3(256), 0, st, w, d_B, r, d_U);
    hipLaunchKernelGGL(k_adapt_lr_sign, dim3(r), dim3(256), 0, st, w.nAC, d_U);
}

// A window's end behind k_chain_adapt_mass (hmcmt.h: a. to e.).  It waits for K -- the adaptation's one added wait, once per window --
// and, where directions were kept, for the orthonormality check's partial sums.  A window that yields no estimate (fewer than four
// pairs, a non-finite value, an eigensolver that did not converge, defect above 1e-8) ends on the diagonal mass with fallback = 1 and
// returns 0; a HIP error ends there too but is NOT a fallback: ctx->err names it and HMCMT_EHIP goes back to the step.  Two event pairs
// time the kernels of every window end (hmcmt_debug_adapt_lowrank_time): four records per window, nothing per step.
static int chain_adapt_lr_window_end(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
    auto& L = C.adapt.lr;
    auto& M = ctx->mass;
    const int nAC = ctx->v.nAC, n = L.stored;
    hipStream_t st = ctx->stream;
    hmcmt_adapt_lowrank_info info{};
    info.windows = L.last.windows + 1;
    info.stored = n; info.skipped = L.skipped; info.stride = L.stride;
    info.fallback = 1;
    int r = 0, rc = 0;
    auto failed = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return false;
        (void)hipGetLastError();
        ctx->err = std::string("hmcmt_chain_adapt_lowrank, window end: ") + what + ": " + hipGetErrorString(e);
        rc = HMCMT_EHIP;
        return true;
    };
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};     // (made and destroyed here: once per window end)
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); e = nullptr; }
    const bool timed = ev[0] && ev[1] && ev[2] && ev[3];
    for (double& t : L.times) t = 0.0;
    bool lifted = false;
    [&]() {
        if (n < ADAPT_LR_NMIN) return;
        const auto w0 = std::chrono::steady_clock::now();
        if (timed) hipEventRecord(ev[0], st);
        const AdaptLr w = chain_adapt_lr_gram(st, nAC, n, L.d_X, L.d_G, ctx->d_invM, L.d_meanX, L.d_meanG, L.d_s, L.d_K);
        if (timed) hipEventRecord(ev[1], st);
        const size_t N2 = (size_t)2 * n;
        L.hK.resize(N2 * N2);
        if (failed(hipMemcpyAsync(L.hK.data(), L.d_K, sizeof(double) * N2 * N2, hipMemcpyDeviceToHost, st), "the download of K")) return;
        if (failed(hipStreamSynchronize(st), "the wait for K")) return;             // the window end's wait
        const auto t0 = std::chrono::steady_clock::now();
        L.times[2] = std::chrono::duration<double, std::milli>(t0 - w0).count();
        const AdaptLrEstimate E = item_adapt_lr_estimate(n, L.hK.data(), L.opt.rank, L.opt.cutoff, L.opt.gamma);
        const auto t1 = std::chrono::steady_clock::now();
        info.host_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        if (E.fallback) return;
        info.dims = E.m; info.theta_min = E.thetaMin; info.theta_max = E.thetaMax;
        if (E.r == 0) { info.fallback = 0; return; }
        if (E.r > M.lrCap) return;                           // (cannot happen: the estimate keeps at most opt.rank == lrCap; the buffers are sized by it)
        std::vector<double> c((size_t)2 * E.r);
        for (int k = 0; k < E.r; ++k) { c[k] = E.theta[k] - 1.0; c[E.r + k] = 1.0 / std::sqrt(E.theta[k]) - 1.0; }
        // (the stream is idle behind the wait: the two small uploads are complete when they return)
        if (failed(hipMemcpy(L.d_B, E.B.data(), sizeof(double) * N2 * E.r, hipMemcpyHostToDevice), "the upload of B")) return;
        if (failed(hipMemcpy(L.d_c, c.data(), sizeof(double) * 2 * E.r, hipMemcpyHostToDevice), "the upload of the coefficients")) return;
        if (timed) hipEventRecord(ev[2], st);
        chain_adapt_lr_lift(st, w, L.d_B, E.r, L.d_U);
        if (timed) hipEventRecord(ev[3], st);
        lifted = true;
        double defect = INFINITY;
        if (mass_lr_defect(ctx, E.r, L.d_s, L.d_U, L.d_c, L.d_part, &defect)) { rc = HMCMT_EHIP; return; }   // (ctx->err is set)
        L.times[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        info.defect = defect;
        if (!(defect <= 1e-8)) return;
        // filled and checked: now into the mass's own buffers, behind everything that still reads them
        if (failed(hipMemcpyAsync(M.d_lrS, L.d_s, sizeof(double) * nAC, hipMemcpyDeviceToDevice, st), "the copy of s") ||
            failed(hipMemcpyAsync(M.d_lrU, L.d_U, sizeof(double) * (size_t)E.r * nAC, hipMemcpyDeviceToDevice, st), "the copy of U") ||
            failed(hipMemcpyAsync(M.d_lrC, L.d_c, sizeof(double) * 2 * E.r, hipMemcpyDeviceToDevice, st), "the copy of the coefficients")) return;
        r = E.r;
        L.hTheta = E.theta;
        info.fallback = 0;
    }();
    if (!rc) {
        const hipError_t e = hipGetLastError();              // (a launch that failed: not a statistical fallback either)
        if (failed(e, "a kernel launch")) { r = 0; info.fallback = 1; }
    }
    if (timed && !rc && n >= ADAPT_LR_NMIN) {                // (both pairs are complete: the last wait came behind them)
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) L.times[0] = ms;
        if (lifted && hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) L.times[1] = ms;
        (void)hipGetLastError();
    }
    for (auto& e : ev)
        if (e) hipEventDestroy(e);
    info.rank = r;
    M.lrRank = r;
    if (r > 0) M.lrLambda.assign(L.hTheta.begin(), L.hTheta.begin() + r); else M.lrLambda.clear();
    M.kind = r > 0 ? HMCMT_MASS_LOWRANK : HMCMT_MASS_DIAGONAL;
    L.last = info;
    return rc;
}

// One counted step of the warm-up (hmcmt.h: 1. to 5.), behind the decision and the commit: launches on the context's stream and scalar
// host work, no wait -- but for the end of a window of an adaptation upgraded by hmcmt_chain_adapt_lowrank (above).  alpha: the step's
// acceptance probability min(1, exp(hdif)), a NUTS sample's mean over its leaves.  The mass kernel runs behind the commit, in front of
// the next k_chain_momentum.  Returns 0, or HMCMT_EHIP where a window end met a HIP error (the adaptation's bookkeeping is complete either way).
static int chain_adapt_step(hmcmt_ctx* ctx, double alpha) {
    auto& C = ctx->chain;
    auto& A = C.adapt;
    const hmcmt_adapt_options& o = A.opt;
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    int rc = 0;
    A.alphaLast = alpha;
    A.alphaSum += alpha;
    const bool inWindow = o.adapt_mass && A.c >= o.init_buffer && A.c < o.nwarmup - o.term_buffer;
    if (inWindow) {
        ++A.wcount;
        hipLaunchKernelGGL(k_chain_welford, dim3((n + 255) / 256), dim3(256), 0, st, n, C.d_m[C.cur], A.d_mean, A.d_m2, (double)A.wcount);
        if (A.lr.on) chain_adapt_lr_store(ctx);
    }
    C.dt = item_adapt_dt(item_adapt_update(A.da, alpha, o.delta, o.gamma, o.t0, o.kappa), o.dt_min, o.dt_max);
    if (inWindow && A.c == A.wnext) {
        if (A.wcount >= 2) {
            const double dn = (double)A.wcount, w = dn / (dn + 5.0), f = 1e-3 * 5.0 / (dn + 5.0);
            hipLaunchKernelGGL(k_chain_adapt_mass, dim3((n + 255) / 256), dim3(256), 0, st, n, A.d_m2, dn - 1.0, w, f, ctx->d_invM);
            if (A.lr.on) rc = chain_adapt_lr_window_end(ctx);
            ++A.windowsDone;
            item_adapt_restart(A.da, C.dt);
        }
        (void)hipMemsetAsync(A.d_mean, 0, sizeof(double) * n, st);
        (void)hipMemsetAsync(A.d_m2, 0, sizeof(double) * n, st);
        A.wcount = 0;
        A.wnext = item_adapt_next_window(A.c, &A.wsize, o.nwarmup, o.term_buffer);
        if (A.lr.on) {                                       // the stores rewind; the next window's length is known now
            A.lr.winStart = A.c + 1;
            A.lr.stride = A.wnext >= 0 ? item_adapt_lr_stride(A.wnext - A.c, A.lr.opt.max_samples) : 1;
            A.lr.closedStored = A.lr.stored;
            A.lr.stored = A.lr.skipped = 0;
        }
    }
    if (++A.c == o.nwarmup) {
        if (A.da.t > 0) C.dt = item_adapt_dt(A.da.x_bar, o.dt_min, o.dt_max);
        A.active = false;
    }
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
    HIPCHK(hipSetDevice(ctx->cfg.device));
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
    C.seeded = false; C.seed = C.t = 0; C.stream = 0;        // (a begin forgets the seed)
    C.active = true;
    if (D0) *D0 = C.D;
    if (M0) *M0 = C.M;
    return 0;
}

// ---- one sample in parts: hmcmt_chain_momentum + hmcmt_chain_step wait twice with the host's numbers, hmcmt_chain_sample once with
// the chain's own (Chain::seed, stream, t) -----------------------------------------------------------------------------------------
// The momentum's launches, enqueued: p = sqrtM clip(z) into d_p and the partial sums of p' M^-1 p into d_part[0 .. LFNB).  draw ==
// nullptr: z is what the caller left in d_z; else *draw is the index of the chain's own draw and nothing is read from d_z.
static int chain_momentum_enqueue(hmcmt_ctx* ctx, const uint64_t* draw) {
    auto& C = ctx->chain;
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    int rc;
    if (ctx->mass.kind != HMCMT_MASS_DIAGONAL) {
        // p = L clip(z), x = Wm^-1 p, K = 0.5 p'x (HMCMT_MASS_LOWRANK: p = F clip(z), x = M^-1 p)
        if (draw) hipLaunchKernelGGL(k_chain_draw_clip, dim3((n + 255) / 256), dim3(256), 0, st, n, C.seed, C.stream, *draw, C.d_p);
        else hipLaunchKernelGGL(k_chain_clip, dim3((n + 255) / 256), dim3(256), 0, st, n, C.d_z, C.d_p);
        if ((rc = mass_apply_dev(ctx, HMCMT_MASS_OP_SQRT, C.d_p, C.d_p))) return rc;
        if ((rc = mass_apply_dev(ctx, HMCMT_MASS_OP_INV, C.d_p, ctx->mass.d_x))) return rc;
        hipLaunchKernelGGL(k_chain_kinetic, dim3(LFNB), dim3(256), 0, st, n, C.d_p, ctx->mass.d_x, ctx->d_invM, C.d_part);
    } else if (draw) {
        hipLaunchKernelGGL(k_chain_draw_momentum, dim3(LFNB), dim3(256), 0, st, n, C.seed, C.stream, *draw, ctx->d_invM, C.d_p, C.d_part);
    } else {
        hipLaunchKernelGGL(k_chain_momentum, dim3(LFNB), dim3(256), 0, st, n, C.d_z, ctx->d_invM, C.d_p, C.d_part);
    }
    return 0;
}

// what a step carries from its enqueue part to its decide part
struct ChainStepState { int startGrad = 0, evals = 0; };

// The step's launches behind a momentum in d_p and its partial sums in d_part: the trajectory of L steps in the proposal buffer, K1,
// k_chain_final and the record's copy to h_rec -- enqueued, the caller waits.  A failure has gone through chain_fail.
static int chain_step_enqueue(hmcmt_ctx* ctx, int32_t L, ChainStepState* S) {
    auto& C = ctx->chain;
    const int n = ctx->v.nAC;
    hipStream_t st = ctx->stream;
    const int cur = C.cur, prop = cur ^ 1;
    C.haveMomentum = false;                                  // consumed, whatever happens
    // the gradient the last decision left on the device is the start gradient only if nothing has evaluated on the context since
    S->startGrad = (C.gen == ctx->stateGen && ctx->lfHaveGrad) ? C.nextStart : 0;
    C.nextStart = 0;
    HIPCHK(hipMemcpyAsync(C.d_m[prop], C.d_m[cur], sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    ctx->lfHaveGrad = false;
    int rc = leapfrog_core(ctx, C.d_m[prop], C.d_p, C.dt, L, C.regParam, C.lo, C.hi, S->startGrad, C.d_pred[prop], C.d_scal + CH_D1, &S->evals);
    if (rc) return chain_fail(ctx, rc);
    const bool wm = ctx->mass.kind != HMCMT_MASS_DIAGONAL;
    if (wm && (rc = mass_apply_dev(ctx, HMCMT_MASS_OP_INV, C.d_p, ctx->mass.d_x))) return chain_fail(ctx, rc);
    hipLaunchKernelGGL(k_chain_kinetic, dim3(LFNB), dim3(256), 0, st, n, C.d_p, wm ? ctx->mass.d_x : nullptr, ctx->d_invM, C.d_part + LFNB);
    hipLaunchKernelGGL(k_chain_final, dim3(1), dim3(1), 0, st, C.d_part, C.d_part + LFNB, ctx->d_lfScal, ctx->d_lfFlag, C.d_scal);
    HIPCHK(hipMemcpyAsync(C.h_rec, C.d_scal, sizeof(double) * CHAIN_REC, hipMemcpyDeviceToHost, st));
    return 0;
}
static int chain_step_decide(hmcmt_ctx* ctx, double u, const ChainStepState& S, hmcmt_chain_record* rec, double* m_out, double* pred_out);

int hmcmt_chain_momentum(hmcmt_ctx* ctx, const double* z, double* K) {
    if (!ctx) return HMCMT_EINVAL;
    if (!z) { ctx->err = "hmcmt_chain_momentum: z is NULL"; return HMCMT_EINVAL; }
    int rc = chain_ready(ctx, "hmcmt_chain_momentum", true);
    if (rc) return rc;
    auto& C = ctx->chain;
    const int n = ctx->v.nAC;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(z[i])) { ctx->err = "hmcmt_chain_momentum: non-finite normal"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    C.haveMomentum = false;
    std::memcpy(ctx->h_stage, z, sizeof(double) * n);
    HIPCHK(hipMemcpyAsync(C.d_z, ctx->h_stage, sizeof(double) * n, hipMemcpyHostToDevice, st));
    if ((rc = chain_momentum_enqueue(ctx, nullptr))) return rc;
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
    HIPCHK(hipSetDevice(ctx->cfg.device));
    ChainStepState S;
    if ((rc = chain_step_enqueue(ctx, L, &S))) return rc;
    return chain_step_decide(ctx, u, S, rec, m_out, pred_out);
}

// The commit of a sample behind its decision, shared by hmcmt_chain_step and the NUTS sample: the counters, the moments and the
// optional accumulators with the chain's current model -- enqueued, not waited for, but for the sketch's shrink once in ell counted
// commits.  Returns 0, or HMCMT_EHIP where that shrink met a HIP error (the sample stands, the sketch is ended).
static int chain_commit(hmcmt_ctx* ctx) {
    auto& C = ctx->chain;
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    hipStream_t st = ctx->stream;
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
            const bool timed = A.timer.start(st);
            hipLaunchKernelGGL(k_chain_acov, dim3((unsigned)((A.ntarget + 255) / 256), (unsigned)(A.K / CHAIN_ACOV_RUN + 1)), dim3(256), 0, st,
                               A.ntarget, A.K, A.count, C.d_m[C.cur], A.d_target, A.d_x0, A.d_tot, A.d_S, A.d_H, A.d_ring);
            if (timed) A.timer.stop(st, A.count >= A.K ? 1 : 0);
            ++A.count;
        }
        if (C.cov.on) {
            auto& V = C.cov;                                 // (t = the count before this commit; the slot = the commits parked so far)
            const bool timed = V.timer.start(st);
            hipLaunchKernelGGL(k_chain_cov_commit, dim3((n + 255) / 256), dim3(256), 0, st, (long long)n, V.count, V.npend, C.d_m[C.cur],
                               V.d_x0, V.d_tot, V.d_q, V.d_pend);
            if (timed) V.timer.stop(st, 0);
            ++V.count;
            if (++V.npend == V.B) chain_cov_flush(ctx);
        }
        if (C.sketch.on && chain_sketch_commit(ctx, C.sketch, C.d_m[C.cur], nullptr, nullptr) == HMCMT_EHIP) return HMCMT_EHIP;
    }
    return 0;
}

// The step behind its launches: the sample's one wait, the record's checks, the accept test with u, the commit (enqueued), the outputs.
// K0 is the record's: what hmcmt_chain_momentum returned, bit for bit, and the only place hmcmt_chain_sample reads it.
static int chain_step_decide(hmcmt_ctx* ctx, double u, const ChainStepState& S, hmcmt_chain_record* rec, double* m_out, double* pred_out) {
    auto& C = ctx->chain;
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    hipStream_t st = ctx->stream;
    const int prop = C.cur ^ 1, startGrad = S.startGrad, evals = S.evals;
    int rc;
    HIPCHK(hipStreamSynchronize(st));                        // the step's one wait
    HIPCHK(hipGetLastError());
    prof_collect(ctx);
    if ((rc = leapfrog_flag(ctx))) return chain_fail(ctx, rc);
    const double K0 = C.h_rec[CH_K0], K1 = C.h_rec[CH_K1], D1 = C.h_rec[CH_D1], M1 = C.h_rec[CH_M1];
    if (!std::isfinite(K0)) {                                // (a host-fed momentum has failed in hmcmt_chain_momentum already)
        ctx->err = "non-finite kinetic energy of the drawn momentum (the diagonal of M^-1 must be positive)";
        return chain_fail(ctx, HMCMT_EBREAKDOWN);
    }
    if (C.h_rec[CH_FLAG] != 0.0 || !std::isfinite(K1) || !std::isfinite(D1) || !std::isfinite(M1)) {
        ctx->err = "non-finite model value or Hamiltonian term at the proposal";
        return chain_fail(ctx, HMCMT_EBREAKDOWN);
    }
    ctx->lfHaveGrad = true;
    const double hdif = (C.D + C.M + K0) - (D1 + K1 + M1);
    const bool accepted = hdif > 0 || u < std::exp(hdif);
    if (accepted) { C.cur = prop; C.D = D1; C.M = M1; }
    C.nextStart = accepted ? 1 : 2;
    const int src = chain_commit(ctx);
    const int wrc = C.adapt.active ? chain_adapt_step(ctx, hdif > 0 ? 1.0 : std::exp(hdif)) : 0;
    const int arc = src ? src : wrc;
    C.gen = ctx->stateGen;
    if (arc) return chain_fail(ctx, arc);                    // (the sample stands; the call reports the HIP error of the sketch's shrink or the window end)
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
    HIPCHK(hipSetDevice(ctx->cfg.device));
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
    int rc = chain_ready(ctx, "hmcmt_chain_moments", true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& C = ctx->chain;
    if ((rc = chain_welford_out(ctx, sizeof(double) * ctx->v.nAC, C.d_mean, C.d_m2, mean, m2, on_device))) return rc;
    if (count) *count = C.nmoments;
    return 0;
}

// ---- the chain's own random numbers: Philox4x32-10 by counter (hmcmt_items.h: item_rng_*), one wait per sample -----------------------
// the two generator calls that need neither a context nor a device: the item functions on the host
int hmcmt_rng_draw(uint64_t seed, uint32_t stream, uint64_t t, int32_t Lmin, int32_t Lmax, int32_t* L, double* u) {
    if (Lmin < 1 || Lmax < Lmin) return HMCMT_EINVAL;
    int l = 0;
    double uu = 0.0;
    item_rng_scalars(seed, stream, t, Lmin, Lmax, &l, &uu);
    if (L) *L = l;
    if (u) *u = uu;
    return 0;
}
int hmcmt_rng_normals(uint64_t seed, uint32_t stream, uint64_t t, int64_t a0, int64_t n, double* z) {
    if (a0 < 0 || n < 0 || a0 > (int64_t)INT32_MAX || n > (int64_t)INT32_MAX + 1 - a0 || (n > 0 && !z)) return HMCMT_EINVAL;
    for (int64_t i = 0; i < n; ++i) z[i] = item_rng_normal(seed, stream, t, (int)(a0 + i));
    return 0;
}

// what the calls on a seeded chain check first
static int chain_rng_ready(hmcmt_ctx* ctx, const char* fn) {
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    if (!ctx->chain.seeded) { ctx->err = std::string(fn) + ": the chain has no seed (hmcmt_chain_seed first; hmcmt_chain_begin forgets it)"; return HMCMT_EINVAL; }
    return 0;
}

int hmcmt_chain_seed(hmcmt_ctx* ctx, uint64_t seed, uint32_t stream) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_chain_seed", true);
    if (rc) return rc;
    auto& C = ctx->chain;
    C.seed = seed; C.stream = stream; C.t = 0;
    C.seeded = true;
    return 0;
}

int hmcmt_chain_rng_state(hmcmt_ctx* ctx, uint64_t* seed, uint32_t* stream, uint64_t* t) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_rng_ready(ctx, "hmcmt_chain_rng_state");
    if (rc) return rc;
    const auto& C = ctx->chain;
    if (seed) *seed = C.seed;
    if (stream) *stream = C.stream;
    if (t) *t = C.t;
    return 0;
}

int hmcmt_chain_rng_seek(hmcmt_ctx* ctx, uint64_t t) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_rng_ready(ctx, "hmcmt_chain_rng_seek");
    if (rc) return rc;
    ctx->chain.t = t;
    return 0;
}

int hmcmt_chain_normals(hmcmt_ctx* ctx, uint64_t t, double* z, int32_t on_device) {
    const char* fn = "hmcmt_chain_normals";
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_rng_ready(ctx, fn);
    if (rc) return rc;
    if (!z) { ctx->err = std::string(fn) + ": z is NULL"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const auto& C = ctx->chain;
    const int n = ctx->v.nAC;
    ChainReadout R(ctx, fn, on_device);
    double* dst = (double*)R.out(z, sizeof(double) * (size_t)n);
    if (R.rc) return R.rc;
    hipLaunchKernelGGL(k_chain_draw_clip, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, C.seed, C.stream, t, dst);
    return R.finish();
}

// one sample with the chain's own numbers; fn: the entry point the messages name
static int chain_sample(hmcmt_ctx* ctx, const char* fn, int32_t Lmin, int32_t Lmax, hmcmt_chain_record* rec, double* m_out, double* pred_out) {
    auto& C = ctx->chain;
    int L = 0;
    double u = 0.0;
    item_rng_scalars(C.seed, C.stream, C.t, Lmin, Lmax, &L, &u);
    const uint64_t t = C.t++;                                // the draw is consumed, whatever happens
    C.haveMomentum = false;
    int rc = chain_momentum_enqueue(ctx, &t);
    if (rc) { ctx->err = std::string(fn) + ": " + ctx->err; return chain_fail(ctx, rc); }
    ChainStepState S;
    if ((rc = chain_step_enqueue(ctx, L, &S))) return rc;
    return chain_step_decide(ctx, u, S, rec, m_out, pred_out);
}

static int chain_sample_ready(hmcmt_ctx* ctx, const char* fn, int32_t Lmin, int32_t Lmax) {
    const int rc = chain_rng_ready(ctx, fn);
    if (rc) return rc;
    if (Lmin < 1 || Lmax < Lmin) { ctx->err = std::string(fn) + ": need 1 <= Lmin <= Lmax"; return HMCMT_EINVAL; }
    return 0;
}

int hmcmt_chain_sample(hmcmt_ctx* ctx, int32_t Lmin, int32_t Lmax, hmcmt_chain_record* rec, double* m_out, double* pred_out) {
    const char* fn = "hmcmt_chain_sample";
    if (!ctx) return HMCMT_EINVAL;
    if (!rec) { ctx->err = std::string(fn) + ": rec is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_sample_ready(ctx, fn, Lmin, Lmax);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    return chain_sample(ctx, fn, Lmin, Lmax, rec, m_out, pred_out);
}

int hmcmt_chain_run(hmcmt_ctx* ctx, int64_t nsamples, int32_t Lmin, int32_t Lmax, hmcmt_chain_record* recs, double* models, double* preds,
                    int64_t* done) {
    const char* fn = "hmcmt_chain_run";
    if (!ctx) return HMCMT_EINVAL;
    if (done) *done = 0;
    if (!recs || nsamples < 0) { ctx->err = std::string(fn) + ": need recs[nsamples] and nsamples >= 0"; return HMCMT_EINVAL; }
    int rc = chain_sample_ready(ctx, fn, Lmin, Lmax);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t)ctx->v.nAC, nd = (size_t)2 * ctx->v.nData;
    for (int64_t i = 0; i < nsamples; ++i) {
        if ((rc = chain_sample(ctx, fn, Lmin, Lmax, recs + i, models ? models + (size_t)i * n : nullptr, preds ? preds + (size_t)i * nd : nullptr)))
            return rc;
        if (done) *done = i + 1;
    }
    return 0;
}

// ---- the No-U-turn sampler (hmcmt.h has the algorithm; kernels_nuts.h; hmcmt_items.h: item_nuts_*) ---------------------------------------
// A sample = the momentum of draw t, then leaf by leaf: leapfrog_core(L = 1) on the moving end's own (m, p) with the gradient kept in
// ctx->d_g (it ends in collect_pending's wait for the evaluation's solver records, as every trajectory does -- once per leaf here, once
// per L steps there), the mass application, k_nuts_leaf, k_nuts_final, one copy of NUTS_SCAL scalars, the leaf's own wait, and the host's decision
// (item_nuts_leaf / item_nuts_merge).  Captures (model, predicted data, gradient) are enqueued behind the decision, in front of the next
// leaf.  The sample ends in chain_commit.
int hmcmt_rng_nuts(uint64_t seed, uint32_t stream, uint64_t t, int32_t kind, uint32_t index, int32_t* forward, double* u) {
    if ((kind != 0 && kind != 1) || (kind == 0 && index >= 32u) || (kind == 1 && index >= 0x40000000u)) return HMCMT_EINVAL;
    int f = 0;
    double uu = 0.0;
    item_rng_nuts(seed, stream, t, kind, index, &f, &uu);
    if (forward) *forward = f;
    if (u) *u = uu;
    return 0;
}

// the tree's buffers, through the chain's allocator; a failure frees what it got and leaves the chain as it was
static int chain_nuts_alloc(hmcmt_ctx* ctx, const char* fn) {
    auto& N = ctx->chain.nuts;
    if (N.ready) return 0;
    const size_t vb = sizeof(double) * std::max<size_t>((size_t)ctx->v.nAC, 1), pb = sizeof(double) * std::max<size_t>((size_t)2 * ctx->v.nData, 1);
    std::vector<std::pair<double**, size_t>> bufs = {{&N.d_g0, vb}, {&N.d_rhoS, vb}, {&N.d_pred, pb},
                                                     {&N.d_part, sizeof(double) * NUTS_NQ * LFNB}, {&N.d_scal, sizeof(double) * NUTS_SCAL}};
    for (int e = 0; e < 2; ++e) {
        for (double** q : {&N.d_m[e], &N.d_p[e], &N.d_x[e], &N.d_g[e], &N.d_rho[e], &N.d_selM[e], &N.d_selG[e]}) bufs.push_back({q, vb});
        bufs.push_back({&N.d_selPred[e], pb});
    }
    for (int k = 0; k < NUTS_CK_MAX; ++k)
        for (int v = 0; v < 3; ++v) bufs.push_back({&N.d_ck[k][v], vb});
    int rc = 0;
    for (const auto& b : bufs)
        if ((rc = chain_acc_zeroed(ctx, fn, N.allocs, (void**)b.first, b.second))) break;
    if (!rc && hipHostMalloc((void**)&N.h_scal, sizeof(double) * NUTS_SCAL, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        N.h_scal = nullptr;
        ctx->err = std::string(fn) + ": pinned allocation failed";
        rc = HMCMT_ENOMEM;
    }
    if (rc) {
        const std::string e = ctx->err;
        (void)hipStreamSynchronize(ctx->stream);
        chain_acc_free(N.allocs);
        N = {};
        ctx->err = e;
        return rc;
    }
    N.ready = true;
    return 0;
}

// the launches of one leaf's sums behind its step: the passes of k_nuts_leaf (NUTS_GROUP due checkpoints each), k_nuts_final
static void nuts_leaf_launch(hipStream_t st, NutsLeaf L, int ndue, const double* const (*due)[3], const double* partK0, const double* misfit,
                             const double* mnorm, const int* flag, double* scal) {
    for (int c0 = 0; c0 == 0 || c0 < ndue; c0 += NUTS_GROUP) {
        const int nc = std::max(0, std::min(NUTS_GROUP, ndue - c0));
        L.ndue = nc;
        L.q0 = c0;
        for (int c = 0; c < NUTS_GROUP; ++c) {
            L.dueP[c] = c < nc ? due[c0 + c][0] : nullptr;
            L.dueX[c] = c < nc ? due[c0 + c][1] : nullptr;
            L.dueR[c] = c < nc ? due[c0 + c][2] : nullptr;
        }
        static_assert(NUTS_GROUP == 4, "one instantiation of k_nuts_leaf per number of checkpoints in a pass below");
        switch (nc + (c0 == 0 ? 0 : 8)) {
#define HMCMT_NUTS_LEAF(NC, FIRST, CASE) \
    case CASE: hipLaunchKernelGGL((k_nuts_leaf<NC, FIRST>), dim3(LFNB), dim3(256), 0, st, L); break;
            HMCMT_NUTS_LEAF(0, true, 0) HMCMT_NUTS_LEAF(1, true, 1) HMCMT_NUTS_LEAF(2, true, 2) HMCMT_NUTS_LEAF(3, true, 3) HMCMT_NUTS_LEAF(4, true, 4)
            HMCMT_NUTS_LEAF(1, false, 9) HMCMT_NUTS_LEAF(2, false, 10) HMCMT_NUTS_LEAF(3, false, 11) HMCMT_NUTS_LEAF(4, false, 12)
#undef HMCMT_NUTS_LEAF
        }
    }
    hipLaunchKernelGGL(k_nuts_final, dim3(1), dim3(64), 0, st, 3 + 2 * ndue, L.part, partK0, misfit, mnorm, flag, scal);
}

// one NUTS sample with the chain's own numbers; fn: the entry point the messages name
static int chain_nuts_sample(hmcmt_ctx* ctx, const char* fn, int32_t maxDepth, hmcmt_nuts_record* rec, double* m_out, double* pred_out) {
    auto& C = ctx->chain;
    auto& N = C.nuts;
    const int n = ctx->v.nAC, nData = ctx->v.nData;
    hipStream_t st = ctx->stream;
    const size_t vb = sizeof(double) * (size_t)n, pb = sizeof(double) * 2 * (size_t)nData;
    const uint64_t t = C.t++;                                // the draw is consumed, whatever happens
    C.haveMomentum = false;
    int rc = chain_nuts_alloc(ctx, fn);
    if (rc) return rc;                                       // (nothing is in flight: the chain stays usable)
    if ((rc = chain_momentum_enqueue(ctx, &t))) { ctx->err = std::string(fn) + ": " + ctx->err; return chain_fail(ctx, rc); }
    // the start gradient into ctx->d_g: what the last decision left on the device, or one evaluation
    const int startGrad = (C.gen == ctx->stateGen && ctx->lfHaveGrad) ? C.nextStart : 0;
    C.nextStart = 0;
    ctx->lfHaveGrad = false;
    int evals = 0;
    if (startGrad == 0) {
        if ((rc = evaluate(ctx, C.d_m[C.cur], true, nullptr, nullptr, ctx->d_g)) || (rc = collect_stats(ctx, true)) || (rc = finish_status(ctx)))
            return chain_fail(ctx, rc);
        ++evals;
    } else if (startGrad == 2) {
        HIPCHK(hipMemcpyAsync(ctx->d_g, ctx->d_gStart, vb, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(N.d_g0, ctx->d_g, vb, hipMemcpyDeviceToDevice, st));
    const bool diag = ctx->mass.kind == HMCMT_MASS_DIAGONAL;
    hipLaunchKernelGGL(k_nuts_begin, dim3((n + 255) / 256), dim3(256), 0, st, n, C.d_m[C.cur], C.d_p, diag ? nullptr : ctx->mass.d_x, N.d_m[0], N.d_m[1],
                       N.d_p[0], N.d_p[1], N.d_x[0], N.d_x[1], N.d_rho[0]);
    int rho = 0;                                             // d_rho[rho]: the tree's momentum sum
    int selTree = 0;                                         // d_sel*[selTree]: the tree's selection once it has left the start, [selTree ^ 1]: the subtree's
    int gOwner = -1;                                         // the end whose gradient ctx->d_g holds (-1: the start's, both ends')
    bool moved[2] = {false, false};                          // the end has left the start: its gradient is in d_g or saved in N.d_g[end]
    NutsTree T;
    item_nuts_begin(T, maxDepth, 0.0);                       // (H0 follows with the first leaf's scalars, which bring K0)
    double K0 = 0, selS[3] = {0, 0, 0}, sel[3] = {0, 0, 0};  // K, D, M at the subtree's / the tree's selection
    uint32_t leaf = 0;
    int unused = 0;                                          // (a leaf's draw has no direction)
    bool first = true;
    while (true) {
        int forward = 0;
        double uj = 0, ul = 0;
        item_rng_nuts(C.seed, C.stream, t, 0, (uint32_t)T.depth, &forward, &uj);
        item_nuts_doubling(T, forward);
        const int d = forward, nl = 1 << T.depth;
        int status = 0;
        for (int i = 0; i < nl; ++i) {
            const int changed = gOwner >= 0 && gOwner != d;
            if (gOwner != d) {                               // the gradient's hand-over where the direction changes
                if (gOwner >= 0) HIPCHK(hipMemcpyAsync(N.d_g[gOwner], ctx->d_g, vb, hipMemcpyDeviceToDevice, st));
                if (gOwner >= 0) HIPCHK(hipMemcpyAsync(ctx->d_g, moved[d] ? N.d_g[d] : N.d_g0, vb, hipMemcpyDeviceToDevice, st));
                gOwner = d;
            }
            int le = 0;
            if ((rc = leapfrog_core(ctx, N.d_m[d], N.d_p[d], C.dt, 1, C.regParam, C.lo, C.hi, 1, N.d_pred, C.d_scal + CH_D1, &le))) return chain_fail(ctx, rc);
            moved[d] = true;
            ++evals;                                         // (le counts the kept start gradient too)
            N.its[changed] += (long long)ctx->stats.iters_fwd_sum + ctx->stats.iters_adj_sum;
            N.solves[changed] += 2LL * ctx->stats.nsystems;
            if (!diag && (rc = mass_apply_dev(ctx, HMCMT_MASS_OP_INV, N.d_p[d], N.d_x[d]))) return chain_fail(ctx, rc);
            int slot = 0, ndue = 0;
            item_nuts_checkpoints(i, &slot, &ndue);
            NutsLeaf L{};
            L.n = n; L.first = i == 0; L.merged = i == nl - 1;
            L.sign = d ? 1.0 : -1.0; L.signOther = d ? -1.0 : 1.0;
            L.p = N.d_p[d]; L.x = diag ? nullptr : N.d_x[d]; L.invM = ctx->d_invM;
            L.rhoS = N.d_rhoS;
            const double* due[NUTS_CK_MAX][3] = {};
            if (i & 1) {
                for (int c = 0; c < ndue; ++c)
                    for (int v = 0; v < 3; ++v) due[c][v] = N.d_ck[slot - c][v];
            } else {
                L.ckP = N.d_ck[slot][0]; L.ckX = N.d_ck[slot][1]; L.ckR = N.d_ck[slot][2];
                ndue = 0;
            }
            L.rho = N.d_rho[rho]; L.rhoNext = N.d_rho[rho ^ 1];
            L.pOther = N.d_p[d ^ 1]; L.xOther = diag ? nullptr : N.d_x[d ^ 1];
            L.part = N.d_part;
            nuts_leaf_launch(st, L, ndue, due, C.d_part, C.d_scal + CH_D1, ctx->d_lfScal, ctx->d_lfFlag, N.d_scal);
            HIPCHK(hipMemcpyAsync(N.h_scal, N.d_scal, sizeof(double) * NUTS_SCAL, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));                // the leaf's one wait
            HIPCHK(hipGetLastError());
            prof_collect(ctx);
            if ((rc = leapfrog_flag(ctx))) return chain_fail(ctx, rc);
            const double* h = N.h_scal;
            if (first) {
                K0 = h[NS_K0];
                if (!std::isfinite(K0)) {
                    ctx->err = "non-finite kinetic energy of the drawn momentum (the diagonal of M^-1 must be positive)";
                    return chain_fail(ctx, HMCMT_EBREAKDOWN);
                }
                T.H0 = C.D + C.M + K0;
                first = false;
            }
            const double K1 = 0.5 * h[NS_SUM], D1 = h[NS_D1], M1 = h[NS_M1];
            const double H = h[NS_FLAG] != 0.0 ? NAN : D1 + K1 + M1;
            item_rng_nuts(C.seed, C.stream, t, 1, leaf++, &unused, &ul);
            bool take = false;
            status = item_nuts_leaf(T, H, ul, h + NS_SUM, &take);
            if (status < 0) break;
            if (take) {                                      // the capture: the leaf is the subtree's selection
                const int s = selTree ^ 1;
                HIPCHK(hipMemcpyAsync(N.d_selM[s], N.d_m[d], vb, hipMemcpyDeviceToDevice, st));
                HIPCHK(hipMemcpyAsync(N.d_selPred[s], N.d_pred, pb, hipMemcpyDeviceToDevice, st));
                HIPCHK(hipMemcpyAsync(N.d_selG[s], ctx->d_g, vb, hipMemcpyDeviceToDevice, st));
                selS[0] = K1; selS[1] = D1; selS[2] = M1;
            }
        }
        if (status < 0) break;
        bool take = false;
        status = item_nuts_merge(T, uj, N.h_scal + NS_SUM, &take);
        if (take) { selTree ^= 1; sel[0] = selS[0]; sel[1] = selS[1]; sel[2] = selS[2]; }
        rho ^= 1;
        if (status < 0) break;
    }
    // the decision: the selected state becomes the chain's, and its gradient the next sample's start gradient
    const bool movedOn = T.selected != 0;
    const int prop = C.cur ^ 1;
    if (movedOn) {
        HIPCHK(hipMemcpyAsync(C.d_m[prop], N.d_selM[selTree], vb, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(C.d_pred[prop], N.d_selPred[selTree], pb, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->d_g, N.d_selG[selTree], vb, hipMemcpyDeviceToDevice, st));
    } else {
        HIPCHK(hipMemcpyAsync(ctx->d_g, N.d_g0, vb, hipMemcpyDeviceToDevice, st));
    }
    ctx->lfHaveGrad = true;
    C.nextStart = 1;
    const double D0 = C.D, M0 = C.M;
    if (movedOn) { C.cur = prop; C.D = sel[1]; C.M = sel[2]; }
    const double alpha = T.alphaSum / (double)T.nleaves;
    const int src = chain_commit(ctx);
    const int wrc = C.adapt.active ? chain_adapt_step(ctx, alpha) : 0;
    const int arc = src ? src : wrc;
    C.gen = ctx->stateGen;
    if (arc) return chain_fail(ctx, arc);                    // (the sample stands; the call reports the HIP error of the sketch's shrink or the window end)
    std::memset(rec, 0, sizeof *rec);
    rec->rec.accepted = movedOn ? 1 : 0;
    rec->rec.nfevals = evals;
    rec->rec.K0 = K0;
    rec->rec.K1 = movedOn ? sel[0] : K0; rec->rec.D1 = movedOn ? sel[1] : D0; rec->rec.M1 = movedOn ? sel[2] : M0;
    rec->rec.D = C.D; rec->rec.M = C.M;
    rec->rec.hdif = movedOn ? (D0 + M0 + K0) - (sel[1] + sel[0] + sel[2]) : 0.0;
    rec->rec.nsamples = C.nsamples; rec->rec.nmoments = C.nmoments;
    rec->depth = T.depth; rec->nleaves = T.nleaves; rec->stop = T.stop; rec->dirs = T.dirs;
    rec->selected = T.selected; rec->alpha = alpha;
    if (m_out || pred_out) {
        if (m_out) HIPCHK(hipMemcpyAsync(m_out, C.d_m[C.cur], vb, hipMemcpyDeviceToHost, st));
        if (pred_out) HIPCHK(hipMemcpyAsync(pred_out, C.d_pred[C.cur], pb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int chain_nuts_ready(hmcmt_ctx* ctx, const char* fn, int32_t maxDepth) {
    const int rc = chain_rng_ready(ctx, fn);
    if (rc) return rc;
    if (maxDepth < 1 || maxDepth > HMCMT_NUTS_DEPTH_MAX) {
        ctx->err = std::string(fn) + ": need 1 <= max_depth <= HMCMT_NUTS_DEPTH_MAX = " + std::to_string(HMCMT_NUTS_DEPTH_MAX);
        return HMCMT_EINVAL;
    }
    if (ctx->mass.kind == HMCMT_MASS_WM) {
        ctx->err = std::string(fn) + ": HMCMT_MASS_WM is not supported (its mass solve synchronises); use the diagonal or the low-rank mass";
        return HMCMT_EINVAL;
    }
    return 0;
}

int hmcmt_chain_nuts_sample(hmcmt_ctx* ctx, int32_t max_depth, hmcmt_nuts_record* rec, double* m_out, double* pred_out) {
    const char* fn = "hmcmt_chain_nuts_sample";
    if (!ctx) return HMCMT_EINVAL;
    if (!rec) { ctx->err = std::string(fn) + ": rec is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_nuts_ready(ctx, fn, max_depth);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    return chain_nuts_sample(ctx, fn, max_depth, rec, m_out, pred_out);
}

int hmcmt_chain_nuts_run(hmcmt_ctx* ctx, int64_t nsamples, int32_t max_depth, hmcmt_nuts_record* recs, double* models, double* preds,
                         int64_t* done) {
    const char* fn = "hmcmt_chain_nuts_run";
    if (!ctx) return HMCMT_EINVAL;
    if (done) *done = 0;
    if (!recs || nsamples < 0) { ctx->err = std::string(fn) + ": need recs[nsamples] and nsamples >= 0"; return HMCMT_EINVAL; }
    int rc = chain_nuts_ready(ctx, fn, max_depth);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t)ctx->v.nAC, nd = (size_t)2 * ctx->v.nData;
    for (int64_t i = 0; i < nsamples; ++i) {
        if ((rc = chain_nuts_sample(ctx, fn, max_depth, recs + i, models ? models + i * n : nullptr, preds ? preds + i * nd : nullptr))) return rc;
        if (done) *done = i + 1;
    }
    return 0;
}

// measurement: the solver's work per leaf by whether the leaf follows a change of direction (hmcmt_debug.h)
int hmcmt_debug_nuts_iters(hmcmt_ctx* ctx, int64_t* out, int32_t reset) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, "hmcmt_debug_nuts_iters", true);
    if (rc) return rc;
    auto& N = ctx->chain.nuts;
    if (out) { out[0] = N.its[1]; out[1] = N.solves[1]; out[2] = N.its[0]; out[3] = N.solves[0]; }
    if (reset) N.its[0] = N.its[1] = N.solves[0] = N.solves[1] = 0;
    return 0;
}

// the two kernels on the caller's device vectors (hmcmt_debug.h)
int hmcmt_debug_nuts_leaf(hmcmt_ctx* ctx, const hmcmt_debug_nuts_args* a, double* sums) {
    const char* fn = "hmcmt_debug_nuts_leaf";
    if (!ctx) return HMCMT_EINVAL;
    static_assert(HMCMT_NUTS_CK_MAX == NUTS_CK_MAX && HMCMT_NUTS_SUMS == NUTS_NQ, "the hook's header mirrors hmcmt_items.h");
    const bool ok = a && sums && a->n >= 1 && a->n <= (int64_t)HMCMT_NUTS_HOOK_NMAX && a->ndue >= 0 && a->ndue <= NUTS_CK_MAX && a->p && a->rho_s &&
                    (a->x || a->inv_m) && (!a->merged || (a->rho && a->rho_next && a->p_other && (a->x_other || a->inv_m)));
    if (!ok) { ctx->err = std::string(fn) + ": need args, sums, 1 <= n <= HMCMT_NUTS_HOOK_NMAX, 0 <= ndue <= HMCMT_NUTS_CK_MAX and the vectors the leaf reads"; return HMCMT_EINVAL; }
    for (int c = 0; c < a->ndue; ++c)
        if (!a->ck_due[c][0] || !a->ck_due[c][1] || !a->ck_due[c][2]) { ctx->err = std::string(fn) + ": a due checkpoint is NULL"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    ChainReadout R(ctx, fn, false);
    double* part = (double*)R.scratch(sizeof(double) * NUTS_NQ * LFNB);
    double* aux = (double*)R.scratch(sizeof(double) * (LFNB + 4));       // zeros: the K0 partial sums, misfit, mnorm, flag
    double scal[NUTS_SCAL];
    double* d_scal = (double*)R.out(scal, sizeof scal);
    if (R.rc) return R.rc;
    HIPCHK(hipMemsetAsync(part, 0, sizeof(double) * NUTS_NQ * LFNB, st));
    HIPCHK(hipMemsetAsync(aux, 0, sizeof(double) * (LFNB + 4), st));
    HIPCHK(hipMemsetAsync(d_scal, 0, sizeof scal, st));
    NutsLeaf L{};
    L.n = (int)a->n; L.first = a->first != 0; L.merged = a->merged != 0;
    L.sign = a->backward ? -1.0 : 1.0; L.signOther = a->other_backward ? -1.0 : 1.0;
    L.p = a->p; L.x = a->x; L.invM = a->inv_m; L.rhoS = a->rho_s;
    L.ckP = a->ck_write[0]; L.ckX = a->ck_write[1]; L.ckR = a->ck_write[2];
    if (!L.ckP || !L.ckX || !L.ckR) L.ckP = L.ckX = L.ckR = nullptr;
    L.rho = a->rho; L.rhoNext = a->rho_next; L.pOther = a->p_other; L.xOther = a->x_other;
    L.part = part;
    nuts_leaf_launch(st, L, a->ndue, a->ck_due, aux, aux + LFNB, aux + LFNB + 1, (const int*)(aux + LFNB + 2), d_scal);
    const int rc = R.finish();
    if (rc) return rc;
    for (int q = 0; q < NUTS_NQ; ++q) sums[q] = q < 3 + 2 * a->ndue ? scal[NS_SUM + q] : 0.0;
    return 0;
}

// ---- the commit's optional accumulators: histograms of the model, moments of the predicted data ------------------------------------
int hmcmt_chain_hist_begin(hmcmt_ctx* ctx, int64_t ntarget, const int64_t* target, int32_t nbins, double lo, double hi) {
    const char* fn = "hmcmt_chain_hist_begin";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    const bool restOk = nbins >= 1 && nbins <= CHAIN_HIST_MAXBINS && std::isfinite(lo) && std::isfinite(hi) && hi > lo && std::isfinite(hi - lo);
    long long nt = 0;
    if ((rc = chain_cell_list(ctx, fn, "target", ntarget, target, false, restOk, "target, ntarget >= 1, 1 <= nbins <= 4096 and finite lo < hi", &nt)))
        return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& H = ctx->chain.hist;
    hipStream_t st = ctx->stream;
    HIPCHK(hipStreamSynchronize(st));                        // (a commit may still be counting into the histogram this one replaces)
    chain_acc_free(H.allocs); H = {};
    auto build = [&]() -> int {
        int r;
        if ((r = chain_cell_upload(ctx, fn, H.allocs, &H.d_target, target, nt))) return r;
        if ((r = chain_acc_zeroed(ctx, fn, H.allocs, (void**)&H.d_counts, (size_t)nt * (size_t)nbins * sizeof(unsigned int)))) return r;
        HIPCHK(hipStreamSynchronize(st));                    // (the caller's list is free again on return)
        return 0;
    };
    if ((rc = build())) {
        (void)hipStreamSynchronize(st);
        chain_acc_free(H.allocs); H = {};
        return rc;
    }
    H.ntarget = nt; H.nbins = nbins; H.lo = lo; H.hi = hi;
    H.scale = (double)nbins / (hi - lo);
    H.w = (hi - lo) / (double)nbins;
    H.count = 0;
    H.on = true;
    return 0;
}

int hmcmt_chain_hist(hmcmt_ctx* ctx, int64_t* count, uint32_t* counts, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    auto& H = ctx->chain.hist;
    const int rc = chain_acc_ready(ctx, "hmcmt_chain_hist", H.on, H.count, false, CHAIN_HIST);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
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
    const char* fn = "hmcmt_chain_hist_quantiles";
    if (!ctx) return HMCMT_EINVAL;
    auto& H = ctx->chain.hist;
    int rc = chain_acc_ready(ctx, fn, H.on, H.count, false, CHAIN_HIST);
    if (rc) return rc;
    if (!q || !out || nq < 1) { ctx->err = "hmcmt_chain_hist_quantiles: need q, out and nq >= 1"; return HMCMT_EINVAL; }
    for (int i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) { ctx->err = "hmcmt_chain_hist_quantiles: every q must lie in [0, 1]"; return HMCMT_EINVAL; }
    if ((rc = chain_acc_ready(ctx, fn, H.on, H.count, true, CHAIN_HIST))) return rc;      // (empty: reported behind the arguments)
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    std::vector<double> x((size_t)nq);
    for (int i = 0; i < nq; ++i) x[i] = q[i] * (double)H.count;       // (one product: what a host restatement forms)
    ChainReadout R(ctx, fn, on_device);
    double* d_x = (double*)R.scratch(sizeof(double) * nq);
    double* dst = (double*)R.out(out, sizeof(double) * (size_t)nq * (size_t)H.ntarget);
    if (R.rc) return R.rc;
    HIPCHK(hipMemcpyAsync(d_x, x.data(), sizeof(double) * nq, hipMemcpyHostToDevice, st));
    for (int q0 = 0; q0 < nq; q0 += 32768) {                 // (a grid's y extent)
        const int nc = std::min(nq - q0, 32768);
        hipLaunchKernelGGL(k_chain_quantiles, dim3((unsigned)((H.ntarget + 255) / 256), (unsigned)nc), dim3(256), 0, st, H.ntarget, H.nbins,
                           nc, H.lo, H.w, d_x + q0, H.d_counts, dst + (size_t)q0 * H.ntarget);
    }
    return R.finish();
}

int hmcmt_chain_data_moments_begin(hmcmt_ctx* ctx) {
    const char* fn = "hmcmt_chain_data_moments_begin";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& M = ctx->chain.dmom;
    hipStream_t st = ctx->stream;
    const size_t bytes = sizeof(double) * std::max<size_t>((size_t)2 * ctx->v.nData, 1);
    M.on = false;
    // (a running accumulator's buffers are kept and zeroed behind a commit that may still be running on them: no wait)
    if (!M.d_mean && (rc = chain_acc_alloc(ctx, fn, M.allocs, (void**)&M.d_mean, bytes))) return rc;
    if (!M.d_m2 && (rc = chain_acc_alloc(ctx, fn, M.allocs, (void**)&M.d_m2, bytes))) return rc;
    HIPCHK(hipMemsetAsync(M.d_mean, 0, bytes, st));
    HIPCHK(hipMemsetAsync(M.d_m2, 0, bytes, st));
    M.count = 0;
    M.on = true;
    return 0;
}

int hmcmt_chain_data_moments(hmcmt_ctx* ctx, int64_t* count, double* mean, double* m2, int32_t on_device) {
    if (!ctx) return HMCMT_EINVAL;
    auto& M = ctx->chain.dmom;
    int rc = chain_acc_ready(ctx, "hmcmt_chain_data_moments", M.on, M.count, false, CHAIN_DMOM);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if ((rc = chain_welford_out(ctx, sizeof(double) * 2 * ctx->v.nData, M.d_mean, M.d_m2, mean, m2, on_device))) return rc;
    if (count) *count = M.count;
    return 0;
}

// ---- lagged autocovariances and the effective sample size (k_chain_acov, k_chain_acov_out, k_chain_ess) ----------------------------
int hmcmt_chain_acov_begin(hmcmt_ctx* ctx, int64_t ntarget, const int64_t* target, int32_t maxlag) {
    const char* fn = "hmcmt_chain_acov_begin";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    long long nt = 0;
    if ((rc = chain_cell_list(ctx, fn, "target", ntarget, target, true, maxlag >= 1 && maxlag <= CHAIN_ACOV_MAXLAG,
                              "target and ntarget >= 1 (or NULL and 0: every active cell) and 1 <= maxlag <= 1023", &nt)))
        return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& A = ctx->chain.acov;
    hipStream_t st = ctx->stream;
    HIPCHK(hipStreamSynchronize(st));                        // (a commit may still be adding to the accumulator this one replaces)
    A.timer.free(ctx->cfg.device, st);
    chain_acc_free(A.allocs); A = {};
    const size_t vb = (size_t)nt * sizeof(double), lb = vb * (size_t)(maxlag + 1);
    auto build = [&]() -> int {
        int r;
        if ((r = chain_cell_upload(ctx, fn, A.allocs, &A.d_target, target, nt))) return r;
        const std::pair<double**, size_t> bufs[] = {{&A.d_x0, vb}, {&A.d_tot, vb}, {&A.d_S, lb}, {&A.d_H, lb}, {&A.d_ring, lb}};
        for (const auto& b : bufs)
            if ((r = chain_acc_zeroed(ctx, fn, A.allocs, (void**)b.first, b.second))) return r;
        HIPCHK(hipStreamSynchronize(st));                    // (the caller's list is free again on return)
        return 0;
    };
    if ((rc = build())) {
        (void)hipStreamSynchronize(st);
        chain_acc_free(A.allocs); A = {};
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
    const char* fn = "hmcmt_chain_acov";
    if (!ctx) return HMCMT_EINVAL;
    auto& A = ctx->chain.acov;
    int rc = chain_acc_ready(ctx, fn, A.on, A.count, mean || acov, CHAIN_ACOV);
    if (rc) return rc;
    if (mean || acov) {
        HIPCHK(hipSetDevice(ctx->cfg.device));
        const size_t mb = sizeof(double) * (size_t)A.ntarget;
        ChainReadout R(ctx, fn, on_device);
        double *d_mean = (double*)R.out(mean, mb), *d_acov = (double*)R.out(acov, mb * (size_t)(A.K + 1));
        if (R.rc) return R.rc;
        chain_acov_launch(ctx, d_mean, d_acov);
        if ((rc = R.finish())) return rc;
    }
    if (count) *count = A.count;
    return 0;
}

int hmcmt_chain_ess(hmcmt_ctx* ctx, double* tau, double* ess, int32_t* window, int32_t on_device) {
    const char* fn = "hmcmt_chain_ess";
    if (!ctx) return HMCMT_EINVAL;
    auto& A = ctx->chain.acov;
    const int rc = chain_acc_ready(ctx, fn, A.on, A.count, true, CHAIN_ACOV);
    if (rc) return rc;
    if (!tau && !ess && !window) return 0;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t mb = sizeof(double) * (size_t)A.ntarget;
    const double lg = std::max(1.0, std::log10((double)A.count));
    static_assert(sizeof(int) == sizeof(int32_t), "window is written as int");
    ChainReadout R(ctx, fn, on_device);
    double* d_acov = (double*)R.scratch(mb * (size_t)(A.K + 1));
    double *d_tau = (double*)R.out(tau, mb), *d_ess = (double*)R.out(ess, mb);
    int* d_win = (int*)R.out(window, sizeof(int) * (size_t)A.ntarget);
    if (R.rc) return R.rc;
    chain_acov_launch(ctx, nullptr, d_acov);
    hipLaunchKernelGGL(k_chain_ess, dim3((unsigned)((A.ntarget + 255) / 256)), dim3(256), 0, ctx->stream, A.ntarget, A.K, A.count,
                       (double)A.count * lg, 1.0 / lg, d_acov, d_tau, d_ess, d_win);
    return R.finish();
}

// measurement only (include/hmcmt_debug.h): the two timing entry points behind their guards
static int chain_timer_report(hmcmt_ctx* ctx, const char* fn, bool on, const ChainAccName& name, ChainTimer& T, int32_t enable, double* ms,
                              int64_t* launches) {
    const int rc = chain_acc_ready(ctx, fn, on, 0, false, name);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    T.report(ctx->stream, enable, ms, launches);
    return 0;
}
int hmcmt_debug_chain_acov_time(hmcmt_ctx* ctx, int32_t enable, double* ms, int64_t* launches) {
    if (!ctx) return HMCMT_EINVAL;
    return chain_timer_report(ctx, "hmcmt_debug_chain_acov_time", ctx->chain.acov.on, CHAIN_ACOV, ctx->chain.acov.timer, enable, ms, launches);
}

// ---- posterior covariance and correlation (k_chain_cov_commit, k_chain_cov_flush, k_chain_cov_out, k_chain_corr) --------------------
int hmcmt_chain_cov_begin(hmcmt_ctx* ctx, int64_t nrow, const int64_t* row, int32_t batch) {
    const char* fn = "hmcmt_chain_cov_begin";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    static_assert(CHAIN_COV_BATCH_MAX == HMCMT_COV_BATCH_MAX, "the header's bound is the kernels'");
    long long nr = 0;
    if ((rc = chain_cell_list(ctx, fn, "row", nrow, row, true, batch >= 0 && batch <= CHAIN_COV_BATCH_MAX,
                              "row and nrow >= 1 (or NULL and 0: every active cell) and 1 <= batch <= 16 (0: the default, 8)", &nr)))
        return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& V = ctx->chain.cov;
    hipStream_t st = ctx->stream;
    HIPCHK(hipStreamSynchronize(st));                        // (a commit may still be adding to the accumulator this one replaces)
    V.timer.free(ctx->cfg.device, st);
    chain_acc_free(V.allocs); V = {};
    const int B = batch == 0 ? CHAIN_COV_BATCH_DEFAULT : batch;
    const size_t vb = (size_t)ctx->v.nAC * sizeof(double);
    auto build = [&]() -> int {
        int r;
        if ((r = chain_cell_upload(ctx, fn, V.allocs, &V.d_row, row, nr))) return r;
        const std::pair<double**, size_t> bufs[] = {{&V.d_x0, vb}, {&V.d_tot, vb}, {&V.d_q, vb}, {&V.d_pend, vb * (size_t)B}, {&V.d_S, vb * (size_t)nr}};
        for (const auto& b : bufs)
            if ((r = chain_acc_zeroed(ctx, fn, V.allocs, (void**)b.first, b.second))) return r;
        HIPCHK(hipStreamSynchronize(st));                    // (the caller's list is free again on return)
        return 0;
    };
    if ((rc = build())) {
        (void)hipStreamSynchronize(st);
        chain_acc_free(V.allocs); V = {};
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
    const char* fn = "hmcmt_chain_cov";
    if (!ctx) return HMCMT_EINVAL;
    auto& V = ctx->chain.cov;
    int rc = chain_acc_ready(ctx, fn, V.on, V.count, mean || var || cov, CHAIN_COV);
    if (rc) return rc;
    if (mean || var || cov) {
        HIPCHK(hipSetDevice(ctx->cfg.device));
        const long long n = ctx->v.nAC;
        const size_t mb = sizeof(double) * (size_t)n;
        ChainReadout R(ctx, fn, on_device);
        double *d_mean = (double*)R.out(mean, mb), *d_var = (double*)R.out(var, mb), *d_cov = (double*)R.out(cov, mb * (size_t)V.nrow);
        if (R.rc) return R.rc;
        if (cov) chain_cov_flush(ctx);                       // (the parked commits first: the later bits stay what they would have been)
        const long long rows = cov ? V.nrow : 1;             // (row 0's owners write mean and var)
        hipLaunchKernelGGL(k_chain_cov_out, chain_cov_grid(ctx, rows), dim3(256), 0, ctx->stream, n, rows, (double)V.count, V.d_x0, V.d_tot,
                           V.d_q, V.d_S, V.d_row, d_mean, d_var, d_cov);
        if ((rc = R.finish())) return rc;
    }
    if (count) *count = V.count;
    return 0;
}

int hmcmt_chain_corr(hmcmt_ctx* ctx, double* corr, int32_t on_device) {
    const char* fn = "hmcmt_chain_corr";
    if (!ctx) return HMCMT_EINVAL;
    auto& V = ctx->chain.cov;
    const int rc = chain_acc_ready(ctx, fn, V.on, V.count, true, CHAIN_COV);
    if (rc) return rc;
    if (!corr) return 0;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const long long n = ctx->v.nAC;
    ChainReadout R(ctx, fn, on_device);
    double* d_corr = (double*)R.out(corr, sizeof(double) * (size_t)n * (size_t)V.nrow);
    if (R.rc) return R.rc;
    chain_cov_flush(ctx);
    hipLaunchKernelGGL(k_chain_corr, chain_cov_grid(ctx, V.nrow), dim3(256), 0, ctx->stream, n, V.nrow, (double)V.count, V.d_tot, V.d_q, V.d_S,
                       V.d_row, d_corr);
    return R.finish();
}

int hmcmt_debug_chain_cov_time(hmcmt_ctx* ctx, int32_t enable, double* ms, int64_t* launches) {
    if (!ctx) return HMCMT_EINVAL;
    return chain_timer_report(ctx, "hmcmt_debug_chain_cov_time", ctx->chain.cov.on, CHAIN_COV, ctx->chain.cov.timer, enable, ms, launches);
}

// ---- posterior principal components by a row sketch (k_chain_sketch_*; the commit and the shrink stand in front of chain_acc_release) ----
int hmcmt_chain_sketch_begin(hmcmt_ctx* ctx, int32_t ell, const double* pivot) {
    const char* fn = "hmcmt_chain_sketch_begin";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    static_assert(CHAIN_SKETCH_ELL_MAX == HMCMT_SKETCH_ELL_MAX, "the header's bound is the kernels'");
    if (ell < CHAIN_SKETCH_ELL_MIN || ell > CHAIN_SKETCH_ELL_MAX) { ctx->err = std::string(fn) + ": need 2 <= ell <= 64"; return HMCMT_EINVAL; }
    if (pivot)
        for (int a = 0; a < ctx->v.nAC; ++a)
            if (!std::isfinite(pivot[a])) { ctx->err = std::string(fn) + ": non-finite pivot"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& S = ctx->chain.sketch;
    HIPCHK(hipStreamSynchronize(ctx->stream));               // (a commit may still be adding to the sketch this one replaces)
    chain_sketch_end(ctx, S, "");
    if ((rc = chain_sketch_alloc(ctx, fn, S, ell, pivot))) {
        const std::string e = ctx->err;
        (void)hipGetLastError();
        chain_sketch_end(ctx, S, "");
        ctx->err = e;
        return rc;
    }
    S.on = true;
    return 0;
}

// the guards of the sketch's read-outs: chain_acc_ready, with the reason where a shrink ended the sketch
static int chain_sketch_ready(hmcmt_ctx* ctx, const char* fn, bool needCommits) {
    const auto& S = ctx->chain.sketch;
    if (!S.on && !S.ended.empty()) {
        const int rc = chain_ready(ctx, fn, true);
        if (rc) return rc;
        ctx->err = std::string(fn) + ": " + S.ended;
        return HMCMT_EINVAL;
    }
    return chain_acc_ready(ctx, fn, S.on, S.count, needCommits, CHAIN_SKETCH);
}

static void chain_sketch_info(const ChainSketch& S, hmcmt_sketch_info* info) {
    *info = hmcmt_sketch_info{};
    info->count = S.count; info->ell = S.ell; info->fill = S.fill; info->shrinks = S.shrinks; info->Delta = S.Delta;
    info->pivot_given = S.pivotGiven ? 1 : 0;
}

int hmcmt_chain_sketch(hmcmt_ctx* ctx, hmcmt_sketch_info* info, double* mean, double* var, double* rows, int32_t on_device) {
    const char* fn = "hmcmt_chain_sketch";
    if (!ctx) return HMCMT_EINVAL;
    auto& S = ctx->chain.sketch;
    int rc = chain_sketch_ready(ctx, fn, mean || var || rows);
    if (rc) return rc;
    if (mean || var || rows) {
        HIPCHK(hipSetDevice(ctx->cfg.device));
        const long long n = ctx->v.nAC;
        const size_t mb = sizeof(double) * (size_t)n;
        if (mean || var) {
            ChainReadout R(ctx, fn, on_device);
            double *d_mean = (double*)R.out(mean, mb), *d_var = (double*)R.out(var, mb);
            if (R.rc) return R.rc;
            hipLaunchKernelGGL(k_chain_cov_out, chain_cov_grid(ctx, 1), dim3(256), 0, ctx->stream, n, 1LL, (double)S.count, S.d_x0, S.d_tot,
                               S.d_q, (const double*)nullptr, (const long long*)nullptr, d_mean, d_var, (double*)nullptr);
            if ((rc = R.finish())) return rc;
        }
        if (rows) {
            HIPCHK(hipMemcpyAsync(rows, S.d_B, mb * (size_t)S.fill, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
    }
    if (info) chain_sketch_info(S, info);
    return 0;
}

int hmcmt_chain_pca(hmcmt_ctx* ctx, int32_t rank, int32_t* kept, double* lambda, double* U, double* err, int32_t on_device) {
    const char* fn = "hmcmt_chain_pca";
    if (!ctx) return HMCMT_EINVAL;
    auto& S = ctx->chain.sketch;
    int rc = chain_sketch_ready(ctx, fn, true);
    if (rc) return rc;
    if (!kept || rank < 1 || rank > HMCMT_MASS_RANK_MAX) { ctx->err = std::string(fn) + ": need kept and 1 <= rank <= HMCMT_MASS_RANK_MAX"; return HMCMT_EINVAL; }
    if (S.count < 2) { ctx->err = std::string(fn) + ": the sketch holds " + std::to_string(S.count) + " commit (two at least make a covariance)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    const long long n = ctx->v.nAC;
    const int nw = S.fill + 1;
    const double dN = (double)S.count;
    hipLaunchKernelGGL(k_chain_sketch_mean, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, dN, std::sqrt(dN), S.d_tot, S.d_B + (size_t)2 * S.ell * n);
    const SketchRows w = chain_sketch_gram(ctx, S, S.fill, true);
    HIPCHK(hipMemcpyAsync(S.hK.data(), S.d_K, sizeof(double) * (size_t)nw * nw, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                        // the read-out's wait for G
    HIPCHK(hipGetLastError());
    std::vector<double> theta;
    std::vector<double>& coef = S.hT;                       // (the sketch's: the upload below reads it until the next wait of this stream)
    const int r = item_chain_sketch_pca(nw, S.hK.data(), rank, theta, coef);
    if (r < 0) { ctx->err = std::string(fn) + ": the Gram matrix is not finite, or an eigensolver did not converge within its sweeps"; return HMCMT_EBREAKDOWN; }
    if (r > 0) {
        HIPCHK(hipMemcpyAsync(S.d_T, coef.data(), sizeof(double) * (size_t)nw * r, hipMemcpyHostToDevice, st));
        ChainReadout R(ctx, fn, on_device);
        double* d_U = U ? (double*)R.out(U, sizeof(double) * (size_t)r * n) : (double*)R.scratch(sizeof(double) * (size_t)r * n);
        double* d_part = (double*)R.scratch(sizeof(double) * (size_t)r * LFNB);
        if (R.rc) return R.rc;
        hipLaunchKernelGGL(k_chain_sketch_lift, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, S.d_T, r, d_U);
        hipLaunchKernelGGL(k_adapt_lr_sign, dim3(r), dim3(256), 0, st, (int)n, d_U);
        double defect = 0.0;
        if ((rc = mass_lr_defect(ctx, r, nullptr, d_U, nullptr, d_part, &defect))) return rc;
        if (!(defect <= 1e-8)) {
            ctx->err = std::string(fn) + ": the components are not orthonormal (max |U U' - I| = " + std::to_string(defect) + ")";
            return HMCMT_EBREAKDOWN;
        }
        if ((rc = R.finish())) return rc;
        if (lambda) {
            for (double& t : theta) t = t / dN;
            if (on_device) HIPCHK(hipMemcpy(lambda, theta.data(), sizeof(double) * r, hipMemcpyHostToDevice));
            else std::copy(theta.begin(), theta.end(), lambda);
        }
    }
    *kept = r;
    if (err) *err = S.Delta / dN;
    return 0;
}

int hmcmt_debug_chain_sketch(hmcmt_ctx* ctx, int32_t ell, int64_t n, const double* rows, const double* pivot, hmcmt_sketch_info* info,
                             double* x0, double* tot, double* q, double* B_out, int32_t max_shrinks, double* K_out, double* T_out) {
    const char* fn = "hmcmt_debug_chain_sketch";
    if (!ctx) return HMCMT_EINVAL;
    if (!ctx->havePrior) { ctx->err = std::string(fn) + ": hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    int rc = chain_ready(ctx, fn, false);
    if (rc) return rc;
    if (!rows || !info || n < 1 || n > 65536 || ell < CHAIN_SKETCH_ELL_MIN || ell > CHAIN_SKETCH_ELL_MAX || max_shrinks < 0 ||
        (max_shrinks > 0 && (!K_out || !T_out))) {
        ctx->err = std::string(fn) + ": need rows, info, 1 <= n <= 65536, 2 <= ell <= 64, and K_out and T_out with max_shrinks > 0";
        return HMCMT_EINVAL;
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    const size_t nAC = (size_t)ctx->v.nAC, vb = nAC * sizeof(double), n2 = (size_t)2 * ell;
    ChainSketch S;
    std::vector<void*> own;
    double* d_rows = nullptr;
    auto run = [&]() -> int {
        int r;
        if ((r = chain_acc_alloc(ctx, fn, own, (void**)&d_rows, (size_t)n * vb))) return r;
        if ((r = chain_sketch_alloc(ctx, fn, S, ell, pivot))) return r;
        HIPCHK(hipMemcpy(d_rows, rows, (size_t)n * vb, hipMemcpyHostToDevice));
        for (int64_t t = 0; t < n; ++t) {
            const bool keep = S.shrinks < max_shrinks;
            r = chain_sketch_commit(ctx, S, d_rows + (size_t)t * nAC, keep ? K_out + (size_t)S.shrinks * n2 * n2 : nullptr,
                                    keep ? T_out + (size_t)S.shrinks * ell * n2 : nullptr);
            if (r == HMCMT_EBREAKDOWN) ctx->err = std::string(fn) + ": " + S.ended;
            if (r) return r;
        }
        if (x0) HIPCHK(hipMemcpyAsync(x0, S.d_x0, vb, hipMemcpyDeviceToHost, st));
        if (tot) HIPCHK(hipMemcpyAsync(tot, S.d_tot, vb, hipMemcpyDeviceToHost, st));
        if (q) HIPCHK(hipMemcpyAsync(q, S.d_q, vb, hipMemcpyDeviceToHost, st));
        if (B_out) HIPCHK(hipMemcpyAsync(B_out, S.d_B, vb * (size_t)S.fill, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        chain_sketch_info(S, info);
        return 0;
    };
    rc = run();
    const std::string e = ctx->err;
    (void)hipStreamSynchronize(st);
    chain_sketch_end(ctx, S, "");
    chain_acc_free(own);
    ctx->err = e;
    return rc;
}

int hmcmt_debug_chain_sketch_sums(hmcmt_ctx* ctx, double* x0, double* tot, double* q, int32_t on_device) {
    const char* fn = "hmcmt_debug_chain_sketch_sums";
    if (!ctx) return HMCMT_EINVAL;
    const auto& S = ctx->chain.sketch;
    const int rc = chain_sketch_ready(ctx, fn, false);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t vb = sizeof(double) * (size_t)ctx->v.nAC;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (x0) HIPCHK(hipMemcpyAsync(x0, S.d_x0, vb, kind, ctx->stream));
    if (tot) HIPCHK(hipMemcpyAsync(tot, S.d_tot, vb, kind, ctx->stream));
    if (q) HIPCHK(hipMemcpyAsync(q, S.d_q, vb, kind, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int hmcmt_debug_chain_sketch_time(hmcmt_ctx* ctx, int32_t enable, double* ms, int64_t* launches, double* host_ms) {
    if (!ctx) return HMCMT_EINVAL;
    auto& S = ctx->chain.sketch;
    const int rc = chain_timer_report(ctx, "hmcmt_debug_chain_sketch_time", S.on, CHAIN_SKETCH, S.timer, enable, ms, launches);
    if (rc) return rc;
    if (host_ms) *host_ms = S.hostMs;
    if (enable >= 0) S.hostMs = 0.0;
    return 0;
}

// ---- the chain's step size and diagonal mass between two steps, and their warm-up adaptation (chain_adapt_step, k_chain_adapt_mass) ----
int hmcmt_chain_set_dt(hmcmt_ctx* ctx, double dt) {
    const char* fn = "hmcmt_chain_set_dt";
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    if (!(dt > 0) || !std::isfinite(dt)) { ctx->err = std::string(fn) + ": need a finite dt > 0"; return HMCMT_EINVAL; }
    if (ctx->chain.adapt.active) { ctx->err = std::string(fn) + ": an adaptation is active (hmcmt_chain_adapt_end first)"; return HMCMT_EINVAL; }
    ctx->chain.dt = dt;
    return 0;
}

int hmcmt_chain_set_mass_diag(hmcmt_ctx* ctx, const double* invM) {
    const char* fn = "hmcmt_chain_set_mass_diag";
    if (!ctx) return HMCMT_EINVAL;
    if (!invM) { ctx->err = std::string(fn) + ": invM is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    auto& C = ctx->chain;
    if (ctx->mass.kind != HMCMT_MASS_DIAGONAL) { 
        ctx->err = std::string(fn) + ": the mass is " + (ctx->mass.kind == HMCMT_MASS_WM ? "HMCMT_MASS_WM" : "HMCMT_MASS_LOWRANK") + ", which has no diagonal to set";
        return HMCMT_EINVAL;
    }
    if (C.adapt.active && C.adapt.opt.adapt_mass) {
        ctx->err = std::string(fn) + ": an adaptation of the mass is active (hmcmt_chain_adapt_end first)";
        return HMCMT_EINVAL;
    }
    const int n = ctx->v.nAC;
    for (int i = 0; i < n; ++i)
        if (!(invM[i] > 0) || !std::isfinite(invM[i])) { ctx->err = std::string(fn) + ": every entry must be finite and > 0"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    C.haveMomentum = false;                                  // (its K0 belongs to the old mass)
    std::memcpy(ctx->h_stage, invM, sizeof(double) * n);
    HIPCHK(hipMemcpyAsync(ctx->d_invM, ctx->h_stage, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));               // (the staging buffer is free again on return)
    return 0;
}

int hmcmt_chain_mass_diag(hmcmt_ctx* ctx, double* invM, int32_t on_device) {
    const char* fn = "hmcmt_chain_mass_diag";
    if (!ctx) return HMCMT_EINVAL;
    if (!invM) { ctx->err = std::string(fn) + ": invM is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipMemcpyAsync(invM, ctx->d_invM, sizeof(double) * ctx->v.nAC, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

void hmcmt_default_adapt_options(hmcmt_adapt_options* o) {
    if (!o) return;
    *o = hmcmt_adapt_options{};
    o->adapt_mass = 1;
    o->init_buffer = 75; o->term_buffer = 50; o->base_window = 25;
    o->delta = 0.8; o->gamma = 0.05; o->t0 = 10.0; o->kappa = 0.75;
}

int hmcmt_chain_adapt_begin(hmcmt_ctx* ctx, const hmcmt_adapt_options* o) {
    const char* fn = "hmcmt_chain_adapt_begin";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    if (!o) { ctx->err = std::string(fn) + ": options is NULL (the defaults leave nwarmup open)"; return HMCMT_EINVAL; }
    const bool finite = std::isfinite(o->delta) && std::isfinite(o->gamma) && std::isfinite(o->t0) && std::isfinite(o->kappa) &&
                        std::isfinite(o->dt_min) && std::isfinite(o->dt_max);
    if (!finite || o->nwarmup < 1 || !(o->delta > 0 && o->delta < 1) || !(o->gamma > 0) || !(o->t0 > 0) || !(o->kappa > 0.5 && o->kappa <= 1) ||
        o->dt_min < 0 || o->dt_max < 0 || (o->dt_min > 0 && o->dt_max > 0 && o->dt_min > o->dt_max)) {
        ctx->err = std::string(fn) + ": need nwarmup >= 1, 0 < delta < 1, gamma > 0, t0 > 0, 0.5 < kappa <= 1 and finite 0 <= dt_min <= dt_max (0: no bound)";
        return HMCMT_EINVAL;
    }
    if (o->adapt_mass) {
        if (ctx->mass.kind != HMCMT_MASS_DIAGONAL) { ctx->err = std::string(fn) + ": adapt_mass needs HMCMT_MASS_DIAGONAL"; return HMCMT_EINVAL; }
        if (o->init_buffer < 0 || o->term_buffer < 0 || o->base_window < 1 ||
            (int64_t)o->init_buffer + o->base_window + o->term_buffer > o->nwarmup) {
            ctx->err = std::string(fn) + ": adapt_mass needs init_buffer, term_buffer >= 0, base_window >= 1 and init_buffer + base_window + term_buffer <= nwarmup";
            return HMCMT_EINVAL;
        }
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    auto& C = ctx->chain;
    auto& A = C.adapt;
    hipStream_t st = ctx->stream;
    if (!A.allocs.empty()) HIPCHK(hipStreamSynchronize(st));    // (a step may still be adding to the window this one replaces)
    chain_acc_free(A.allocs); A = {};
    if (o->adapt_mass) {
        const size_t vb = sizeof(double) * (size_t)ctx->v.nAC;
        if ((rc = chain_acc_zeroed(ctx, fn, A.allocs, (void**)&A.d_mean, vb)) || (rc = chain_acc_zeroed(ctx, fn, A.allocs, (void**)&A.d_m2, vb))) {
            (void)hipStreamSynchronize(st);
            chain_acc_free(A.allocs); A = {};
            return rc;
        }
    }
    A.opt = *o;
    A.opt.adapt_mass = o->adapt_mass ? 1 : 0;
    item_adapt_restart(A.da, C.dt);
    A.wsize = o->base_window;
    A.wnext = o->adapt_mass ? (long long)o->init_buffer + o->base_window - 1 : -1;
    A.begun = A.active = true;
    return 0;
}

// what the info and end calls check first
static int chain_adapt_ready(hmcmt_ctx* ctx, const char* fn) {
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    if (!ctx->chain.adapt.begun) { ctx->err = std::string(fn) + ": no adaptation in this chain (hmcmt_chain_adapt_begin first)"; return HMCMT_EINVAL; }
    return 0;
}

int hmcmt_chain_adapt_info(hmcmt_ctx* ctx, hmcmt_adapt_info* info) {
    const char* fn = "hmcmt_chain_adapt_info";
    if (!ctx) return HMCMT_EINVAL;
    if (!info) { ctx->err = std::string(fn) + ": info is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_adapt_ready(ctx, fn);
    if (rc) return rc;
    const auto& C = ctx->chain;
    const auto& A = C.adapt;
    std::memset(info, 0, sizeof *info);                      // (the padding too: two infos of one state compare equal as bytes)
    info->step = A.c; info->nwarmup = A.opt.nwarmup; info->window_count = A.wcount; info->next_window_end = A.wnext;
    info->active = A.active ? 1 : 0; info->windows_done = A.windowsDone;
    info->dt = C.dt;
    info->dt_bar = A.da.t > 0 ? item_adapt_dt(A.da.x_bar, A.opt.dt_min, A.opt.dt_max) : C.dt;
    info->mu = A.da.mu; info->s_bar = A.da.s_bar; info->alpha_last = A.alphaLast; info->alpha_sum = A.alphaSum;
    return 0;
}

int hmcmt_chain_adapt_end(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    const int rc = chain_adapt_ready(ctx, "hmcmt_chain_adapt_end");
    if (rc) return rc;
    auto& C = ctx->chain;
    auto& A = C.adapt;
    if (A.active) {
        if (A.da.t > 0) C.dt = item_adapt_dt(A.da.x_bar, A.opt.dt_min, A.opt.dt_max);
        A.active = false;                                    // (the window's buffers go with the chain, or with the next begin call)
    }
    return 0;
}

// ---- the low-rank mass of a live chain: the warm-up's upgrade, its info, the between-steps setter and the read-out ----------------
void hmcmt_default_adapt_lowrank_options(hmcmt_adapt_lowrank_options* o) {
    if (!o) return;
    *o = hmcmt_adapt_lowrank_options{};
    o->rank = 8; o->max_samples = 64; o->cutoff = 2.0; o->gamma = 1e-5;
}

int hmcmt_chain_adapt_lowrank(hmcmt_ctx* ctx, const hmcmt_adapt_lowrank_options* o) {
    const char* fn = "hmcmt_chain_adapt_lowrank";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_adapt_ready(ctx, fn);
    if (rc) return rc;
    if (!o) { ctx->err = std::string(fn) + ": options is NULL"; return HMCMT_EINVAL; }
    auto& A = ctx->chain.adapt;
    auto& M = ctx->mass;
    if (!A.active || !A.opt.adapt_mass) { ctx->err = std::string(fn) + ": needs a running adaptation begun with adapt_mass = 1"; return HMCMT_EINVAL; }
    if (A.c != 0) { ctx->err = std::string(fn) + ": the adaptation has counted a step (call it right behind hmcmt_chain_adapt_begin)"; return HMCMT_EINVAL; }
    if (A.lr.on) { ctx->err = std::string(fn) + ": the adaptation is upgraded already"; return HMCMT_EINVAL; }
    if (o->rank < 1 || o->rank > HMCMT_MASS_RANK_MAX || o->max_samples < ADAPT_LR_NMIN || o->max_samples > ADAPT_LR_NMAX ||
        !std::isfinite(o->cutoff) || !(o->cutoff > 1.0) || !std::isfinite(o->gamma) || !(o->gamma > 0.0)) {
        ctx->err = std::string(fn) + ": need 1 <= rank <= HMCMT_MASS_RANK_MAX, 4 <= max_samples <= 128, a finite cutoff > 1 and a finite gamma > 0";
        return HMCMT_EINVAL;
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t nAC = (size_t)ctx->v.nAC, ms = (size_t)o->max_samples, rk = (size_t)o->rank, D = sizeof(double);
    decltype(A.lr) L{};
    std::vector<void*> own;                                  // handed to the adaptation's allocs only when everything is there
    const std::vector<std::pair<double**, size_t>> bufs = {
        {&L.d_X, ms * nAC * D}, {&L.d_G, ms * nAC * D}, {&L.d_K, 4 * ms * ms * D}, {&L.d_B, 2 * ms * rk * D}, {&L.d_meanX, nAC * D},
        {&L.d_meanG, nAC * D}, {&L.d_s, nAC * D}, {&L.d_U, rk * nAC * D}, {&L.d_c, 2 * rk * D}, {&L.d_part, rk * LFNB * D}};
    for (const auto& b : bufs)
        if ((rc = chain_acc_zeroed(ctx, fn, own, (void**)b.first, b.second))) break;
    // the mass's own buffers for `rank` directions (the kind is HMCMT_MASS_DIAGONAL here: adapt_mass = 1 was accepted, so none are held)
    double *d_s = nullptr, *d_U = nullptr, *d_c = nullptr, *d_part = nullptr;
    if (!rc && (rc = mass_lr_alloc(ctx, o->rank, &d_s, &d_U, &d_c, &d_part))) {
        (void)hipGetLastError();
        mass_lr_free(ctx, {d_s, d_U, d_c, d_part});
        ctx->err = std::string(fn) + ": device allocation failed";
        rc = HMCMT_ENOMEM;
    }
    if (rc) {                                                // (the diagonal adaptation goes on as it was)
        const std::string e = ctx->err;
        (void)hipStreamSynchronize(ctx->stream);
        chain_acc_free(own);
        ctx->err = e;
        return rc;
    }
    mass_lr_release(ctx);
    M.d_lrS = d_s; M.d_lrU = d_U; M.d_lrC = d_c; M.d_lrPart = d_part;
    M.lrRank = 0; M.lrCap = o->rank;
    A.allocs.insert(A.allocs.end(), own.begin(), own.end());
    L.on = true;
    L.opt = *o;
    L.winStart = A.opt.init_buffer;
    L.stride = item_adapt_lr_stride(A.wnext - A.opt.init_buffer + 1, o->max_samples);
    A.lr = std::move(L);
    return 0;
}

int hmcmt_chain_adapt_lowrank_info(hmcmt_ctx* ctx, hmcmt_adapt_lowrank_info* info) {
    const char* fn = "hmcmt_chain_adapt_lowrank_info";
    if (!ctx) return HMCMT_EINVAL;
    if (!info) { ctx->err = std::string(fn) + ": info is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_adapt_ready(ctx, fn);
    if (rc) return rc;
    if (!ctx->chain.adapt.lr.on) { ctx->err = std::string(fn) + ": the adaptation was not upgraded (hmcmt_chain_adapt_lowrank)"; return HMCMT_EINVAL; }
    std::memset(info, 0, sizeof *info);
    const hmcmt_adapt_lowrank_info& s = ctx->chain.adapt.lr.last;
    info->windows = s.windows; info->stored = s.stored; info->skipped = s.skipped; info->dims = s.dims; info->rank = s.rank;
    info->fallback = s.fallback; info->stride = s.stride;
    info->theta_min = s.theta_min; info->theta_max = s.theta_max; info->defect = s.defect; info->host_ms = s.host_ms;
    return 0;
}

int hmcmt_chain_set_mass_lowrank(hmcmt_ctx* ctx, const double* invM, int32_t rank, const double* U, const double* lambda) {
    const char* fn = "hmcmt_chain_set_mass_lowrank";
    if (!ctx) return HMCMT_EINVAL;
    int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    auto& C = ctx->chain;
    auto& M = ctx->mass;
    if (M.kind == HMCMT_MASS_WM) { ctx->err = std::string(fn) + ": the mass is HMCMT_MASS_WM (hmcmt_set_mass first; it ends the chain)"; return HMCMT_EINVAL; }
    if (C.adapt.active && C.adapt.opt.adapt_mass) {
        ctx->err = std::string(fn) + ": an adaptation of the mass is active (hmcmt_chain_adapt_end first)";
        return HMCMT_EINVAL;
    }
    if (rank < 0 || rank > HMCMT_MASS_RANK_MAX) {
        ctx->err = std::string(fn) + ": rank " + std::to_string(rank) + " is outside 0 .. HMCMT_MASS_RANK_MAX = " + std::to_string(HMCMT_MASS_RANK_MAX);
        return HMCMT_EINVAL;
    }
    if (rank == 0 && !invM) { ctx->err = std::string(fn) + ": rank 0 needs invM"; return HMCMT_EINVAL; }
    if (rank > 0 && (!U || !lambda)) { ctx->err = std::string(fn) + (!U ? ": U is NULL" : ": lambda is NULL"); return HMCMT_EINVAL; }
    const int n = ctx->v.nAC;
    std::vector<double> s((size_t)n), c((size_t)2 * rank);
    for (int k = 0; k < rank; ++k) {
        if (!std::isfinite(lambda[k]) || !(lambda[k] > 0.0)) { ctx->err = std::string(fn) + ": lambda[" + std::to_string(k) + "] is not finite and positive"; return HMCMT_EINVAL; }
        c[k] = lambda[k] - 1.0;
        c[rank + k] = 1.0 / std::sqrt(lambda[k]) - 1.0;
    }
    for (size_t i = 0; i < (size_t)rank * n; ++i)
        if (!std::isfinite(U[i])) { ctx->err = std::string(fn) + ": U[" + std::to_string(i / n) + "][" + std::to_string(i % n) + "] is not finite"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));               // (a commit may still be reading the mass buffers)
    if (invM) std::copy(invM, invM + n, s.begin());
    else if (M.kind == HMCMT_MASS_LOWRANK && !M.lrInvM.empty()) s = M.lrInvM;     // (the scales hmcmt_set_mass_lowrank was given: in force, not in d_invM)
    else HIPCHK(hipMemcpy(s.data(), ctx->d_invM, sizeof(double) * n, hipMemcpyDeviceToHost));   // (the diagonal in force)
    for (int a = 0; a < n; ++a)
        if (!std::isfinite(s[a]) || !(s[a] > 0.0)) { ctx->err = std::string(fn) + ": invM[" + std::to_string(a) + "] is not finite and positive"; return HMCMT_EINVAL; }
    if (rank == 0) {
        HIPCHK(hipMemcpy(ctx->d_invM, s.data(), sizeof(double) * n, hipMemcpyHostToDevice));
        mass_lr_release(ctx);
        M.kind = HMCMT_MASS_DIAGONAL;
        C.haveMomentum = false;
        return 0;
    }
    const std::vector<double> diag = s;
    for (int a = 0; a < n; ++a) s[a] = std::sqrt(s[a]);
    double *d_s = nullptr, *d_U = nullptr, *d_c = nullptr, *d_part = nullptr, defect = 0.0;
    rc = mass_lr_build(ctx, rank, s, U, c, &d_s, &d_U, &d_c, &d_part, &defect);
    if (rc || !(defect <= 1e-8)) {                           // (nothing has changed: the mass and the chain stay)
        const std::string e = ctx->err;
        mass_lr_free(ctx, {d_s, d_U, d_c, d_part});
        if (rc) { ctx->err = e; return rc; }
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.3e", defect);
        ctx->err = std::string(fn) + ": the rows of U are not orthonormal (max |U'U - I| = " + buf + " > 1e-8)";
        return HMCMT_EINVAL;
    }
    HIPCHK(hipMemcpy(ctx->d_invM, diag.data(), sizeof(double) * n, hipMemcpyHostToDevice));   // (hmcmt_chain_mass_diag stays truthful)
    mass_lr_release(ctx);
    M.d_lrS = d_s; M.d_lrU = d_U; M.d_lrC = d_c; M.d_lrPart = d_part;
    M.lrRank = M.lrCap = rank;
    M.lrLambda.assign(lambda, lambda + rank);
    M.kind = HMCMT_MASS_LOWRANK;
    C.haveMomentum = false;                                  // (its K0 belongs to the old mass)
    return 0;
}

int hmcmt_chain_mass_lowrank(hmcmt_ctx* ctx, int32_t* rank, double* invM, double* U, double* lambda, int32_t on_device) {
    const char* fn = "hmcmt_chain_mass_lowrank";
    if (!ctx) return HMCMT_EINVAL;
    if (!rank) { ctx->err = std::string(fn) + ": rank is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    auto& M = ctx->mass;
    if (M.kind == HMCMT_MASS_WM) { ctx->err = std::string(fn) + ": the mass is HMCMT_MASS_WM"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    const int n = ctx->v.nAC, r = M.kind == HMCMT_MASS_LOWRANK ? M.lrRank : 0;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    *rank = r;
    if (invM && r > 0 && !M.lrInvM.empty()) HIPCHK(hipMemcpyAsync(invM, M.lrInvM.data(), sizeof(double) * n, on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost, st));
    else if (invM) HIPCHK(hipMemcpyAsync(invM, ctx->d_invM, sizeof(double) * n, kind, st));
    if (r > 0 && U) HIPCHK(hipMemcpyAsync(U, M.d_lrU, sizeof(double) * (size_t)r * n, kind, st));
    HIPCHK(hipStreamSynchronize(st));
    if (r > 0 && lambda) {                                   // (the bits that were given or estimated, not 1 + the stored lambda - 1)
        if (on_device) HIPCHK(hipMemcpy(lambda, M.lrLambda.data(), sizeof(double) * r, hipMemcpyHostToDevice));
        else std::copy(M.lrLambda.begin(), M.lrLambda.begin() + r, lambda);
    }
    return 0;
}

int hmcmt_debug_adapt_lowrank(hmcmt_ctx* ctx, int32_t n, const double* X, const double* G, const double* invM, double* K_out,
                              const double* B, int32_t r, double* U_out) {
    const char* fn = "hmcmt_debug_adapt_lowrank";
    if (!ctx) return HMCMT_EINVAL;
    if (!ctx->havePrior) { ctx->err = std::string(fn) + ": hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    if (!X || !G || !invM || !K_out || n < ADAPT_LR_NMIN || n > ADAPT_LR_NMAX || r < 0 || r > HMCMT_MASS_RANK_MAX || (B && r > 0 && !U_out)) {
        ctx->err = std::string(fn) + ": need X, G, invM, K_out, 4 <= n <= 128, 0 <= r <= HMCMT_MASS_RANK_MAX and U_out with B";
        return HMCMT_EINVAL;
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    const size_t nAC = (size_t)ctx->v.nAC, N2 = (size_t)2 * n, D = sizeof(double);
    const bool lift = B && r > 0;
    std::vector<void*> own;
    double *d_X = nullptr, *d_G = nullptr, *d_invM = nullptr, *d_mx = nullptr, *d_mg = nullptr, *d_s = nullptr, *d_K = nullptr, *d_B = nullptr, *d_U = nullptr;
    int rc = 0;
    for (const auto& b : std::vector<std::pair<double**, size_t>>{{&d_X, n * nAC * D}, {&d_G, n * nAC * D}, {&d_invM, nAC * D}, {&d_mx, nAC * D},
                                                                   {&d_mg, nAC * D}, {&d_s, nAC * D}, {&d_K, N2 * N2 * D},
                                                                   {&d_B, std::max<size_t>(N2 * r, 1) * D}, {&d_U, std::max<size_t>(r * nAC, 1) * D}})
        if ((rc = chain_acc_zeroed(ctx, fn, own, (void**)b.first, b.second))) break;
    auto run = [&]() -> int {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(d_X, X, n * nAC * D, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_G, G, n * nAC * D, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_invM, invM, nAC * D, hipMemcpyHostToDevice));
        if (lift) HIPCHK(hipMemcpy(d_B, B, N2 * r * D, hipMemcpyHostToDevice));
        const AdaptLr w = chain_adapt_lr_gram(st, (int)nAC, n, d_X, d_G, d_invM, d_mx, d_mg, d_s, d_K);
        if (lift) chain_adapt_lr_lift(st, w, d_B, r, d_U);
        HIPCHK(hipMemcpyAsync(K_out, d_K, N2 * N2 * D, hipMemcpyDeviceToHost, st));
        if (lift) HIPCHK(hipMemcpyAsync(U_out, d_U, r * nAC * D, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        return 0;
    };
    if (!rc) rc = run();
    const std::string e = ctx->err;
    (void)hipStreamSynchronize(st);
    chain_acc_free(own);
    ctx->err = e;
    return rc;
}

int hmcmt_debug_adapt_lowrank_time(hmcmt_ctx* ctx, double* out) {
    const char* fn = "hmcmt_debug_adapt_lowrank_time";
    if (!ctx) return HMCMT_EINVAL;
    if (!out) { ctx->err = std::string(fn) + ": out is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_adapt_ready(ctx, fn);
    if (rc) return rc;
    const auto& L = ctx->chain.adapt.lr;
    if (!L.on) { ctx->err = std::string(fn) + ": the adaptation was not upgraded (hmcmt_chain_adapt_lowrank)"; return HMCMT_EINVAL; }
    for (int i = 0; i < 4; ++i) out[i] = L.times[i];
    return 0;
}

int hmcmt_debug_adapt_lowrank_rows(hmcmt_ctx* ctx, int32_t* n, double* X, double* G) {
    const char* fn = "hmcmt_debug_adapt_lowrank_rows";
    if (!ctx) return HMCMT_EINVAL;
    if (!n) { ctx->err = std::string(fn) + ": n is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_adapt_ready(ctx, fn);
    if (rc) return rc;
    const auto& L = ctx->chain.adapt.lr;
    if (!L.on) { ctx->err = std::string(fn) + ": the adaptation was not upgraded (hmcmt_chain_adapt_lowrank)"; return HMCMT_EINVAL; }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const int rows = L.stored > 0 ? L.stored : L.closedStored;   // (an empty open window: the closed one's rows are still there)
    const size_t bytes = sizeof(double) * (size_t)rows * ctx->v.nAC;
    *n = rows;
    if (X && bytes) HIPCHK(hipMemcpyAsync(X, L.d_X, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (G && bytes) HIPCHK(hipMemcpyAsync(G, L.d_G, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- checkpoint and resume (hmcmt_chain_save / hmcmt_chain_restore; include/hmcmt.h has the container and every payload) --------------
// A blob is laid out by ONE function, chain_blob_plan: per section its scalars (8-byte fields) and its arrays as (device pointer, bytes)
// pieces in the payload's order.  hmcmt_chain_save_size adds the plan up, hmcmt_chain_save walks it.  hmcmt_chain_restore parses the
// sections back with BlobCursor in the same order, first without a device (chain_blob_check: everything that can be refused) and then
// with one (chain_blob_build).
constexpr uint32_t blob_tag(char a, char b, char c, char d) {
    return (uint32_t)(unsigned char)a | (uint32_t)(unsigned char)b << 8 | (uint32_t)(unsigned char)c << 16 | (uint32_t)(unsigned char)d << 24;
}
constexpr uint32_t BLOB_CHAN = blob_tag('C', 'H', 'A', 'N'), BLOB_MASS = blob_tag('M', 'A', 'S', 'S'), BLOB_HIST = blob_tag('H', 'I', 'S', 'T'),
                   BLOB_DMOM = blob_tag('D', 'M', 'O', 'M'), BLOB_ACOV = blob_tag('A', 'C', 'O', 'V'), BLOB_COV = blob_tag('C', 'O', 'V', ' '),
                   BLOB_ADPT = blob_tag('A', 'D', 'P', 'T'), BLOB_ADLR = blob_tag('A', 'D', 'L', 'R'), BLOB_SKCH = blob_tag('S', 'K', 'C', 'H');
constexpr uint32_t BLOB_ORDER[] = {BLOB_CHAN, BLOB_MASS, BLOB_HIST, BLOB_DMOM, BLOB_ACOV, BLOB_COV, BLOB_ADPT, BLOB_ADLR, BLOB_SKCH};
constexpr size_t BLOB_HEADER = 64, BLOB_ENTRY = 24;
constexpr char BLOB_MAGIC[8] = {'H', 'M', 'C', 'M', 'T', 'C', 'K', '\0'};
static_assert(sizeof(double) == 8 && sizeof(long long) == 8, "a blob's fields are 8 bytes");

static uint64_t blob_checksum(const unsigned char* p, uint64_t bytes) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint64_t i = 0; i + 8 <= bytes; i += 8) {
        uint64_t w;
        std::memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x100000001b3ull;
    }
    return h;
}

struct BlobPiece { const void* dev; const void* host; uint64_t bytes; };      // one array: on the device, or (small) on the host
struct BlobSection {
    uint32_t tag = 0;
    std::vector<uint64_t> scal;
    std::vector<BlobPiece> pieces;
    void i(long long v) { uint64_t w; std::memcpy(&w, &v, 8); scal.push_back(w); }
    void f(double v) { uint64_t w; std::memcpy(&w, &v, 8); scal.push_back(w); }
    void u(uint64_t v) { scal.push_back(v); }
    void dev(const void* p, uint64_t bytes) { if (bytes) pieces.push_back({p, nullptr, bytes}); }
    void host(const void* p, uint64_t bytes) { if (bytes) pieces.push_back({nullptr, p, bytes}); }
    uint64_t bytes() const {
        uint64_t b = 8 * scal.size();
        for (const auto& p : pieces) b += (p.bytes + 7) & ~(uint64_t)7;
        return b;
    }
};

// the rows of the low-rank adaptation's stores that a later call can still read
static int chain_adapt_lr_rows(const hmcmt_ctx::Chain::Adapt::Lr& L) { return L.stored > 0 ? L.stored : L.closedStored; }

// the chain as it stands, section by section (nothing is copied: the pieces point into the context)
static std::vector<BlobSection> chain_blob_plan(hmcmt_ctx* ctx) {
    const auto& C = ctx->chain;
    const auto& M = ctx->mass;
    const uint64_t n = (uint64_t)ctx->v.nAC, nd2 = 2 * (uint64_t)ctx->v.nData, D = sizeof(double);
    std::vector<BlobSection> out;
    {
        BlobSection s; s.tag = BLOB_CHAN;
        s.f(C.dt); s.f(C.regParam); s.f(C.lo); s.f(C.hi); s.f(C.D); s.f(C.M);
        s.i(C.burnin); s.i(C.nsamples); s.i(C.nmoments);
        s.u(C.seeded ? C.seed : 0); s.u(C.seeded ? C.t : 0);
        s.u((uint64_t)(C.seeded ? C.stream : 0) | (uint64_t)(C.seeded ? 1 : 0) << 32);
        s.dev(C.d_m[C.cur], n * D); s.dev(C.d_pred[C.cur], nd2 * D); s.dev(C.d_mean, n * D); s.dev(C.d_m2, n * D);
        out.push_back(std::move(s));
    }
    {
        BlobSection s; s.tag = BLOB_MASS;
        const bool lr = M.kind == HMCMT_MASS_LOWRANK, given = lr && !M.lrInvM.empty();
        const uint64_t r = lr ? (uint64_t)M.lrRank : 0;
        s.i(M.kind); s.i((long long)r); s.i(M.kind == HMCMT_MASS_WM ? 0 : M.lrCap); s.i(given ? 1 : 0);
        if (M.kind != HMCMT_MASS_WM) s.dev(ctx->d_invM, n * D);
        if (lr) { s.dev(M.d_lrS, n * D); s.dev(M.d_lrU, r * n * D); s.host(M.lrLambda.data(), r * D); }
        if (given) s.host(M.lrInvM.data(), n * D);
        out.push_back(std::move(s));
    }
    if (C.hist.on) {
        const auto& H = C.hist;
        BlobSection s; s.tag = BLOB_HIST;
        s.i(H.ntarget); s.i(H.nbins); s.i(H.count); s.f(H.lo); s.f(H.hi);
        s.dev(H.d_target, (uint64_t)H.ntarget * 8); s.dev(H.d_counts, (uint64_t)H.ntarget * (uint64_t)H.nbins * sizeof(unsigned int));
        out.push_back(std::move(s));
    }
    if (C.dmom.on) {
        BlobSection s; s.tag = BLOB_DMOM;
        s.i(C.dmom.count);
        s.dev(C.dmom.d_mean, nd2 * D); s.dev(C.dmom.d_m2, nd2 * D);
        out.push_back(std::move(s));
    }
    if (C.acov.on) {
        const auto& A = C.acov;
        BlobSection s; s.tag = BLOB_ACOV;
        const uint64_t vb = (uint64_t)A.ntarget * D, lb = vb * (uint64_t)(A.K + 1);
        s.i(A.ntarget); s.i(A.d_target ? 0 : 1); s.i(A.K); s.i(A.count);
        if (A.d_target) s.dev(A.d_target, (uint64_t)A.ntarget * 8);
        s.dev(A.d_x0, vb); s.dev(A.d_tot, vb); s.dev(A.d_S, lb); s.dev(A.d_H, lb); s.dev(A.d_ring, lb);
        out.push_back(std::move(s));
    }
    if (C.cov.on) {
        const auto& V = C.cov;
        BlobSection s; s.tag = BLOB_COV;
        s.i(V.nrow); s.i(V.d_row ? 0 : 1); s.i(V.B); s.i(V.count); s.i(V.npend);
        if (V.d_row) s.dev(V.d_row, (uint64_t)V.nrow * 8);
        s.dev(V.d_x0, n * D); s.dev(V.d_tot, n * D); s.dev(V.d_q, n * D);
        s.dev(V.d_pend, (uint64_t)V.npend * n * D); s.dev(V.d_S, (uint64_t)V.nrow * n * D);
        out.push_back(std::move(s));
    }
    if (C.adapt.begun) {
        const auto& A = C.adapt;
        const hmcmt_adapt_options& o = A.opt;
        BlobSection s; s.tag = BLOB_ADPT;
        s.i(o.nwarmup); s.i(o.adapt_mass); s.i(o.init_buffer); s.i(o.term_buffer); s.i(o.base_window);
        s.f(o.delta); s.f(o.gamma); s.f(o.t0); s.f(o.kappa); s.f(o.dt_min); s.f(o.dt_max);
        s.f(A.da.mu); s.f(A.da.s_bar); s.f(A.da.x_bar); s.f(A.da.x); s.i(A.da.t);
        s.i(A.c); s.i(A.wcount); s.i(A.wnext); s.i(A.wsize); s.i(A.windowsDone);
        s.f(A.alphaLast); s.f(A.alphaSum); s.i(1); s.i(A.active ? 1 : 0);
        if (o.adapt_mass) { s.dev(A.d_mean, n * D); s.dev(A.d_m2, n * D); }
        out.push_back(std::move(s));
        if (A.lr.on) {
            const auto& L = A.lr;
            const uint64_t rows = (uint64_t)chain_adapt_lr_rows(L);
            BlobSection t; t.tag = BLOB_ADLR;
            t.i(L.opt.rank); t.i(L.opt.max_samples); t.f(L.opt.cutoff); t.f(L.opt.gamma);
            t.i(L.winStart); t.i(L.stride); t.i(L.stored); t.i(L.skipped); t.i(L.closedStored); t.i((long long)rows);
            t.i(L.last.windows); t.i(L.last.stored); t.i(L.last.skipped); t.i(L.last.dims); t.i(L.last.rank); t.i(L.last.fallback); t.i(L.last.stride);
            t.f(L.last.theta_min); t.f(L.last.theta_max); t.f(L.last.defect); t.f(L.last.host_ms);
            t.dev(L.d_X, rows * n * D); t.dev(L.d_G, rows * n * D);
            out.push_back(std::move(t));
        }
    }
    if (C.sketch.on) {                                       // (the last of the table: every blob without a sketch keeps its bytes)
        const auto& K = C.sketch;
        BlobSection s; s.tag = BLOB_SKCH;
        s.i(K.ell); s.i(K.fill); s.i(K.count); s.i(K.shrinks); s.i(K.pivotGiven ? 1 : 0); s.f(K.Delta);
        s.dev(K.d_x0, n * D); s.dev(K.d_tot, n * D); s.dev(K.d_q, n * D); s.dev(K.d_B, (uint64_t)K.fill * n * D);
        out.push_back(std::move(s));
    }
    return out;
}

static uint64_t chain_blob_bytes(const std::vector<BlobSection>& plan) {
    uint64_t b = BLOB_HEADER + BLOB_ENTRY * plan.size() + 8;
    for (const auto& s : plan) b += s.bytes();
    return b;
}

int hmcmt_chain_save_size(hmcmt_ctx* ctx, uint64_t* bytes) {
    const char* fn = "hmcmt_chain_save_size";
    if (!ctx) return HMCMT_EINVAL;
    if (!bytes) { ctx->err = std::string(fn) + ": bytes is NULL"; return HMCMT_EINVAL; }
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    *bytes = chain_blob_bytes(chain_blob_plan(ctx));
    return 0;
}

int hmcmt_chain_save(hmcmt_ctx* ctx, void* buf, uint64_t capacity, uint64_t* written) {
    const char* fn = "hmcmt_chain_save";
    if (!ctx) return HMCMT_EINVAL;
    if (written) *written = 0;
    const int rc = chain_ready(ctx, fn, true);
    if (rc) return rc;
    const std::vector<BlobSection> plan = chain_blob_plan(ctx);
    const uint64_t total = chain_blob_bytes(plan);
    if (written) *written = total;
    if (!buf || capacity < total) {
        ctx->err = std::string(fn) + ": the chain needs " + std::to_string(total) + " bytes, the buffer has " + std::to_string(buf ? capacity : 0);
        return HMCMT_EINVAL;
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipStream_t st = ctx->stream;
    const auto& C = ctx->chain;
    unsigned char* b = (unsigned char*)buf;
    auto put = [&](uint64_t at, const void* p, size_t nb) { std::memcpy(b + at, p, nb); };
    auto put32 = [&](uint64_t at, uint32_t v) { put(at, &v, 4); };
    auto put64 = [&](uint64_t at, uint64_t v) { put(at, &v, 8); };
    put(0, BLOB_MAGIC, 8);
    put32(8, HMCMT_BLOB_VERSION); put32(12, (uint32_t)plan.size());
    put64(16, total);
    put64(24, (uint64_t)(long long)ctx->v.nAC); put64(32, (uint64_t)(long long)ctx->v.nData);
    put32(40, (uint32_t)ctx->mass.kind); put32(44, C.seeded ? 1u : 0u);
    put64(48, (uint64_t)C.nsamples); put64(56, (uint64_t)C.nmoments);
    uint64_t at = BLOB_HEADER + BLOB_ENTRY * plan.size();
    for (size_t k = 0; k < plan.size(); ++k) {
        const BlobSection& s = plan[k];
        const uint64_t e = BLOB_HEADER + BLOB_ENTRY * k;
        put32(e, s.tag); put32(e + 4, 0); put64(e + 8, at); put64(e + 16, s.bytes());
        put(at, s.scal.data(), 8 * s.scal.size());
        at += 8 * s.scal.size();
        for (const BlobPiece& p : s.pieces) {
            const uint64_t padded = (p.bytes + 7) & ~(uint64_t)7;
            if (padded != p.bytes) put64(at + padded - 8, 0);                 // (the padding is zero: two saves are the same bytes)
            if (p.host) put(at, p.host, (size_t)p.bytes);
            else HIPCHK(hipMemcpyAsync(b + at, p.dev, (size_t)p.bytes, hipMemcpyDeviceToHost, st));
            at += padded;
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    put64(at, blob_checksum(b, at));
    return 0;
}

// ---- a blob read back ----------------------------------------------------------------------------------------------------------------
struct BlobEntry { uint32_t tag; uint64_t offset, bytes; };
struct BlobParsed {
    hmcmt_chain_blob_header h{};
    std::vector<BlobEntry> entries;
    const BlobEntry* find(uint32_t tag) const {
        for (const auto& e : entries) if (e.tag == tag) return &e;
        return nullptr;
    }
};
// reads one payload in its order; ok turns false where the payload is too short
struct BlobCursor {
    const unsigned char* p; uint64_t left; bool ok = true;
    BlobCursor(const unsigned char* b, const BlobEntry& e) : p(b + e.offset), left(e.bytes) {}
    uint64_t u() { uint64_t w = 0; if (left < 8) { ok = false; return 0; } std::memcpy(&w, p, 8); p += 8; left -= 8; return w; }
    long long i() { const uint64_t w = u(); long long v; std::memcpy(&v, &w, 8); return v; }
    double f() { const uint64_t w = u(); double v; std::memcpy(&v, &w, 8); return v; }
    const unsigned char* arr(uint64_t bytes) {                               // an array of `bytes` bytes, padded to 8
        const uint64_t padded = (bytes + 7) & ~(uint64_t)7;
        if (!ok || padded < bytes || left < padded) { ok = false; return nullptr; }
        const unsigned char* q = p; p += padded; left -= padded; return q;
    }
};

// the container alone: magic, version, sizes, the table's consistency, the checksum, CHAN against the header.  why: what is wrong
static int blob_parse(const void* buf, uint64_t bytes, BlobParsed& P, std::string& why) {
    const unsigned char* b = (const unsigned char*)buf;
    auto get32 = [&](uint64_t at) { uint32_t v; std::memcpy(&v, b + at, 4); return v; };
    auto get64 = [&](uint64_t at) { uint64_t v; std::memcpy(&v, b + at, 8); return v; };
    if (!buf || bytes < BLOB_HEADER + 2 * BLOB_ENTRY + 8 || bytes % 8) { why = "too short for a blob, or no multiple of 8 bytes"; return HMCMT_EINVAL; }
    if (std::memcmp(b, BLOB_MAGIC, 8)) { why = "no blob of this library (the magic is not \"HMCMTCK\")"; return HMCMT_EINVAL; }
    auto& h = P.h;
    h.version = get32(8); h.nsections = get32(12); h.total_bytes = get64(16);
    if (h.version != HMCMT_BLOB_VERSION) { why = "version " + std::to_string(h.version) + " (this library reads version 1)"; return HMCMT_EINVAL; }
    if (h.total_bytes != bytes) { why = "the header says " + std::to_string(h.total_bytes) + " bytes, the buffer has " + std::to_string(bytes); return HMCMT_EINVAL; }
    if (get64(bytes - 8) != blob_checksum(b, bytes - 8)) { why = "the checksum does not match"; return HMCMT_EINVAL; }
    if (h.nsections < 2 || h.nsections > HMCMT_BLOB_SECTIONS_MAX || BLOB_HEADER + BLOB_ENTRY * h.nsections + 8 > bytes) { why = "the section count is out of range"; return HMCMT_EINVAL; }
    std::memcpy(&h.nAC, b + 24, 8); std::memcpy(&h.nData, b + 32, 8);
    std::memcpy(&h.mass_kind, b + 40, 4); h.seeded = get32(44);
    std::memcpy(&h.nsamples, b + 48, 8); std::memcpy(&h.nmoments, b + 56, 8);
    if (h.nAC < 1 || h.nAC > INT32_MAX || h.nData < 0 || h.nData > INT32_MAX / 2 || h.seeded > 1 || h.nsamples < 0 || h.nmoments < 0 || h.nmoments > h.nsamples ||
        h.mass_kind < HMCMT_MASS_DIAGONAL || h.mass_kind > HMCMT_MASS_LOWRANK) { why = "a header field is out of range"; return HMCMT_EINVAL; }
    uint64_t at = BLOB_HEADER + BLOB_ENTRY * h.nsections;
    size_t order = 0;
    for (uint32_t k = 0; k < h.nsections; ++k) {
        const uint64_t e = BLOB_HEADER + BLOB_ENTRY * k;
        const BlobEntry en{get32(e), get64(e + 8), get64(e + 16)};
        while (order < sizeof BLOB_ORDER / sizeof *BLOB_ORDER && BLOB_ORDER[order] != en.tag) ++order;
        if (order == sizeof BLOB_ORDER / sizeof *BLOB_ORDER) { why = "section " + std::to_string(k) + ": an unknown tag, a repeated one, or one out of order"; return HMCMT_EINVAL; }
        ++order;
        if (get32(e + 4) != 0 || en.offset % 8 || en.bytes % 8 || en.offset != at || en.bytes > bytes - 8 - at) {
            why = "section " + std::to_string(k) + ": its offset or length is no multiple of 8, overlaps, leaves a gap or runs past the end";
            return HMCMT_EINVAL;
        }
        at += en.bytes;
        P.entries.push_back(en);
        h.tags[k] = en.tag; h.section_bytes[k] = en.bytes;
    }
    if (at + 8 != bytes) { why = "bytes behind the last section"; return HMCMT_EINVAL; }
    if (P.entries[0].tag != BLOB_CHAN || P.entries[1].tag != BLOB_MASS) { why = "CHAN and MASS must come first"; return HMCMT_EINVAL; }
    if (P.find(BLOB_ADLR) && !P.find(BLOB_ADPT)) { why = "ADLR without ADPT"; return HMCMT_EINVAL; }
    if (P.entries[0].bytes != 96 + 8 * (3 * (uint64_t)h.nAC + 2 * (uint64_t)h.nData)) { why = "CHAN has not the length of nAC and nData"; return HMCMT_EINVAL; }
    BlobCursor c(b, P.entries[0]);
    for (int k = 0; k < 7; ++k) (void)c.u();
    const long long ns = c.i(), nm = c.i();
    (void)c.u(); (void)c.u();
    const uint64_t ss = c.u();
    if (ns != h.nsamples || nm != h.nmoments || (ss >> 32) != h.seeded) { why = "CHAN and the header disagree"; return HMCMT_EINVAL; }
    return 0;
}

int hmcmt_chain_blob_info(const void* buf, uint64_t bytes, hmcmt_chain_blob_header* out) {
    if (!buf || !out) return HMCMT_EINVAL;
    BlobParsed P;
    std::string why;
    const int rc = blob_parse(buf, bytes, P, why);
    if (rc) return rc;
    *out = P.h;
    return 0;
}

// what a restore reads out of a blob before it touches the context: every scalar, and where the arrays lie
struct BlobChain {
    double dt, regParam, lo, hi, D, M;
    long long burnin, nsamples, nmoments;
    uint64_t seed, t; uint32_t stream; bool seeded;
    const unsigned char *m, *pred, *mean, *m2;
    struct { int kind, rank, cap; bool given; const unsigned char *invM, *s, *U, *lambda, *invM0; } mass{};
    struct { bool on; long long ntarget, count; int nbins; double lo, hi; const unsigned char *target, *counts; } hist{};
    struct { bool on; long long count; const unsigned char *mean, *m2; } dmom{};
    struct { bool on, all; long long ntarget, count; int K; const unsigned char *target, *x0, *tot, *S, *H, *ring; } acov{};
    struct { bool on, all; long long nrow, count; int B, npend; const unsigned char *row, *x0, *tot, *q, *pend, *S; } cov{};
    struct { bool on, active; hmcmt_adapt_options opt; AdaptDA da; long long c, wcount, wnext, wsize; int windowsDone; double alphaLast, alphaSum;
             const unsigned char *mean, *m2; } adapt{};
    struct { bool on; hmcmt_adapt_lowrank_options opt; long long winStart, stride; int stored, skipped, closedStored, rows;
             hmcmt_adapt_lowrank_info last; const unsigned char *X, *G; } lr{};
    struct { bool on, given; int ell, fill; long long count, shrinks; double Delta; const unsigned char *x0, *tot, *q, *B; } sketch{};
};

static bool blob_finite(const unsigned char* p, uint64_t n, bool positive) {
    for (uint64_t k = 0; k < n; ++k) {
        double v;
        std::memcpy(&v, p + 8 * k, 8);
        if (!std::isfinite(v) || (positive && !(v > 0.0))) return false;
    }
    return true;
}
static bool blob_cells(const unsigned char* p, uint64_t n, long long nAC) {
    for (uint64_t k = 0; k < n; ++k) {
        long long v;
        std::memcpy(&v, p + 8 * k, 8);
        if (v < 0 || v >= nAC) return false;
    }
    return true;
}

// every section against the context's sizes and the ranges the begin calls check; nothing of the context changes
static int chain_blob_check(hmcmt_ctx* ctx, const unsigned char* b, const BlobParsed& P, BlobChain& R) {
    const char* fn = "hmcmt_chain_restore";
    const long long nAC = ctx->v.nAC, nData = ctx->v.nData;
    const uint64_t n = (uint64_t)nAC, nd2 = 2 * (uint64_t)nData, D = 8;
    auto bad = [&](const std::string& what) { ctx->err = std::string(fn) + ": " + what; return HMCMT_EINVAL; };
    if (P.h.nAC != nAC || P.h.nData != nData)
        return bad("the blob is of a problem with nAC = " + std::to_string(P.h.nAC) + ", nData = " + std::to_string(P.h.nData) + "; the context has " +
                   std::to_string(nAC) + ", " + std::to_string(nData));
    {
        BlobCursor c(b, P.entries[0]);
        R.dt = c.f(); R.regParam = c.f(); R.lo = c.f(); R.hi = c.f(); R.D = c.f(); R.M = c.f();
        R.burnin = c.i(); R.nsamples = c.i(); R.nmoments = c.i();
        R.seed = c.u(); R.t = c.u();
        const uint64_t ss = c.u();
        R.stream = (uint32_t)ss; R.seeded = (ss >> 32) != 0;
        R.m = c.arr(n * D); R.pred = c.arr(nd2 * D); R.mean = c.arr(n * D); R.m2 = c.arr(n * D);
        if (!c.ok || c.left) return bad("CHAN: wrong length");
        if (!(R.dt > 0) || !std::isfinite(R.dt) || !std::isfinite(R.regParam) || !std::isfinite(R.lo) || !std::isfinite(R.hi) || !(R.hi > R.lo) ||
            R.burnin < 0 || !std::isfinite(R.D) || !std::isfinite(R.M) || !blob_finite(R.m, n, false))
            return bad("CHAN: need finite dt > 0, regParam, lnSigMax > lnSigMin, D, M, burnin >= 0 and a finite model");
    }
    {
        BlobCursor c(b, P.entries[1]);
        auto& Q = R.mass;
        const long long kind = c.i(), rank = c.i(), cap = c.i(), given = c.i();
        if (!c.ok || kind != P.h.mass_kind || rank < 0 || rank > HMCMT_MASS_RANK_MAX || cap < 0 || cap > HMCMT_MASS_RANK_MAX || (given != 0 && given != 1) ||
            (kind == HMCMT_MASS_LOWRANK ? (rank < 1 || cap < rank) : (rank != 0 || given != 0)) || (kind == HMCMT_MASS_WM && cap != 0))
            return bad("MASS: kind, rank or capacity out of range");
        Q.kind = (int)kind; Q.rank = (int)rank; Q.cap = (int)cap; Q.given = given != 0;
        if (kind == HMCMT_MASS_WM && ctx->mass.kind != HMCMT_MASS_WM) return bad("the blob was saved under HMCMT_MASS_WM: hmcmt_set_mass(HMCMT_MASS_WM) first");
        if (kind != HMCMT_MASS_WM) Q.invM = c.arr(n * D);
        if (kind == HMCMT_MASS_LOWRANK) { Q.s = c.arr(n * D); Q.U = c.arr((uint64_t)rank * n * D); Q.lambda = c.arr((uint64_t)rank * D); }
        if (Q.given) Q.invM0 = c.arr(n * D);
        if (!c.ok || c.left) return bad("MASS: wrong length");
        if ((Q.invM && !blob_finite(Q.invM, n, true)) || (Q.s && !blob_finite(Q.s, n, true)) || (Q.U && !blob_finite(Q.U, (uint64_t)rank * n, false)) ||
            (Q.lambda && !blob_finite(Q.lambda, (uint64_t)rank, true)) || (Q.invM0 && !blob_finite(Q.invM0, n, true)))
            return bad("MASS: every scale and lambda must be finite and > 0, every direction finite");
    }
    if (const BlobEntry* e = P.find(BLOB_HIST)) {
        BlobCursor c(b, *e);
        auto& H = R.hist;
        H.on = true;
        H.ntarget = c.i(); const long long nbins = c.i(); H.count = c.i(); H.lo = c.f(); H.hi = c.f();
        if (!c.ok || H.ntarget < 1 || H.ntarget > INT32_MAX || nbins < 1 || nbins > CHAIN_HIST_MAXBINS || H.count < 0 || !std::isfinite(H.lo) || !std::isfinite(H.hi) ||
            !(H.hi > H.lo) || !std::isfinite(H.hi - H.lo))
            return bad("HIST: need ntarget >= 1, 1 <= nbins <= 4096, finite lo < hi and count >= 0");
        H.nbins = (int)nbins;
        H.target = c.arr((uint64_t)H.ntarget * 8); H.counts = c.arr((uint64_t)H.ntarget * (uint64_t)nbins * sizeof(unsigned int));
        if (!c.ok || c.left) return bad("HIST: wrong length");
        if (!blob_cells(H.target, (uint64_t)H.ntarget, nAC)) return bad("HIST: a target is no active cell");
    }
    if (const BlobEntry* e = P.find(BLOB_DMOM)) {
        BlobCursor c(b, *e);
        R.dmom.on = true;
        R.dmom.count = c.i();
        R.dmom.mean = c.arr(nd2 * D); R.dmom.m2 = c.arr(nd2 * D);
        if (!c.ok || c.left || R.dmom.count < 0) return bad("DMOM: wrong length or a negative count");
    }
    if (const BlobEntry* e = P.find(BLOB_ACOV)) {
        BlobCursor c(b, *e);
        auto& A = R.acov;
        A.on = true;
        A.ntarget = c.i(); const long long all = c.i(), K = c.i(); A.count = c.i();
        if (!c.ok || A.ntarget < 1 || A.ntarget > INT32_MAX || (all != 0 && all != 1) || (all && A.ntarget != nAC) || K < 1 || K > CHAIN_ACOV_MAXLAG || A.count < 0)
            return bad("ACOV: need ntarget >= 1 (all cells: nAC), 1 <= maxlag <= 1023 and count >= 0");
        A.all = all != 0; A.K = (int)K;
        const uint64_t vb = (uint64_t)A.ntarget * D, lb = vb * (uint64_t)(K + 1);
        if (!A.all) A.target = c.arr((uint64_t)A.ntarget * 8);
        A.x0 = c.arr(vb); A.tot = c.arr(vb); A.S = c.arr(lb); A.H = c.arr(lb); A.ring = c.arr(lb);
        if (!c.ok || c.left) return bad("ACOV: wrong length");
        if (A.target && !blob_cells(A.target, (uint64_t)A.ntarget, nAC)) return bad("ACOV: a target is no active cell");
    }
    if (const BlobEntry* e = P.find(BLOB_COV)) {
        BlobCursor c(b, *e);
        auto& V = R.cov;
        V.on = true;
        V.nrow = c.i(); const long long all = c.i(), B = c.i(); V.count = c.i(); const long long npend = c.i();
        if (!c.ok || V.nrow < 1 || V.nrow > INT32_MAX || (all != 0 && all != 1) || (all && V.nrow != nAC) || B < 1 || B > CHAIN_COV_BATCH_MAX || V.count < 0 ||
            npend < 0 || npend >= B || npend > V.count)
            return bad("COV: need nrow >= 1 (all cells: nAC), 1 <= batch <= 16, count >= 0 and 0 <= npend < batch");
        V.all = all != 0; V.B = (int)B; V.npend = (int)npend;
        if ((uint64_t)V.nrow > c.left / D / n) return bad("COV: wrong length");      // (nrow * nAC * 8 may not wrap: S alone must fit)
        if (!V.all) V.row = c.arr((uint64_t)V.nrow * 8);
        V.x0 = c.arr(n * D); V.tot = c.arr(n * D); V.q = c.arr(n * D); V.pend = c.arr((uint64_t)npend * n * D); V.S = c.arr((uint64_t)V.nrow * n * D);
        if (!c.ok || c.left) return bad("COV: wrong length");
        if (V.row && !blob_cells(V.row, (uint64_t)V.nrow, nAC)) return bad("COV: a row is no active cell");
    }
    if (const BlobEntry* e = P.find(BLOB_ADPT)) {
        BlobCursor c(b, *e);
        auto& A = R.adapt;
        A.on = true;
        hmcmt_adapt_options& o = A.opt;
        o = hmcmt_adapt_options{};
        o.nwarmup = c.i(); const long long am = c.i(), ib = c.i(), tb = c.i(), bw = c.i();
        o.delta = c.f(); o.gamma = c.f(); o.t0 = c.f(); o.kappa = c.f(); o.dt_min = c.f(); o.dt_max = c.f();
        A.da.mu = c.f(); A.da.s_bar = c.f(); A.da.x_bar = c.f(); A.da.x = c.f(); A.da.t = c.i();
        A.c = c.i(); A.wcount = c.i(); A.wnext = c.i(); A.wsize = c.i(); const long long wd = c.i();
        A.alphaLast = c.f(); A.alphaSum = c.f(); const long long begun = c.i(), active = c.i();
        const bool finite = std::isfinite(o.delta) && std::isfinite(o.gamma) && std::isfinite(o.t0) && std::isfinite(o.kappa) && std::isfinite(o.dt_min) &&
                            std::isfinite(o.dt_max);
        if (!c.ok || !finite || o.nwarmup < 1 || !(o.delta > 0 && o.delta < 1) || !(o.gamma > 0) || !(o.t0 > 0) || !(o.kappa > 0.5 && o.kappa <= 1) || o.dt_min < 0 ||
            o.dt_max < 0 || (o.dt_min > 0 && o.dt_max > 0 && o.dt_min > o.dt_max) || (am != 0 && am != 1) || begun != 1 || (active != 0 && active != 1) ||
            (am && (ib < 0 || tb < 0 || bw < 1 || ib > INT32_MAX || tb > INT32_MAX || bw > INT32_MAX || ib + bw + tb > o.nwarmup)) || A.c < 0 || A.c > o.nwarmup ||
            A.wcount < 0 || A.wnext < -1 || A.wsize < 0 || wd < 0 || wd > INT32_MAX || A.da.t < 0 || (active && A.c >= o.nwarmup) ||
            (am && R.mass.kind == HMCMT_MASS_WM))
            return bad("ADPT: an option or a counter is outside the range hmcmt_chain_adapt_begin accepts");
        o.adapt_mass = (int)am; o.init_buffer = (int)ib; o.term_buffer = (int)tb; o.base_window = (int)bw;
        A.windowsDone = (int)wd; A.active = active != 0;
        if (am) { A.mean = c.arr(n * D); A.m2 = c.arr(n * D); }
        if (!c.ok || c.left) return bad("ADPT: wrong length");
    }
    if (const BlobEntry* e = P.find(BLOB_ADLR)) {
        BlobCursor c(b, *e);
        auto& L = R.lr;
        L.on = true;
        const long long rank = c.i(), ms = c.i();
        L.opt = hmcmt_adapt_lowrank_options{};
        L.opt.cutoff = c.f(); L.opt.gamma = c.f();
        L.winStart = c.i(); L.stride = c.i(); const long long stored = c.i(), skipped = c.i(), closed = c.i(), rows = c.i();
        long long w[6];
        for (long long& v : w) v = c.i();
        L.last = hmcmt_adapt_lowrank_info{};
        L.last.stride = c.i(); L.last.theta_min = c.f(); L.last.theta_max = c.f(); L.last.defect = c.f(); L.last.host_ms = c.f();
        bool ok = c.ok && R.adapt.opt.adapt_mass && rank >= 1 && rank <= HMCMT_MASS_RANK_MAX && ms >= ADAPT_LR_NMIN && ms <= ADAPT_LR_NMAX && std::isfinite(L.opt.cutoff) &&
                  L.opt.cutoff > 1.0 && std::isfinite(L.opt.gamma) && L.opt.gamma > 0.0 && L.stride >= 1 && stored >= 0 && stored <= ms && skipped >= 0 &&
                  skipped <= INT32_MAX && closed >= 0 && closed <= ms && rows == (stored > 0 ? stored : closed) && L.winStart >= 0 &&
                  (!R.adapt.active || R.mass.cap >= rank);
        for (long long v : w) ok = ok && v >= INT32_MIN && v <= INT32_MAX;
        if (!ok) return bad("ADLR: an option or a counter is outside the range hmcmt_chain_adapt_lowrank accepts, or the mass has no room for its rank");
        L.opt.rank = (int)rank; L.opt.max_samples = (int)ms;
        L.stored = (int)stored; L.skipped = (int)skipped; L.closedStored = (int)closed; L.rows = (int)rows;
        L.last.windows = (int)w[0]; L.last.stored = (int)w[1]; L.last.skipped = (int)w[2]; L.last.dims = (int)w[3]; L.last.rank = (int)w[4]; L.last.fallback = (int)w[5];
        L.X = c.arr((uint64_t)rows * n * D); L.G = c.arr((uint64_t)rows * n * D);
        if (!c.ok || c.left) return bad("ADLR: wrong length");
    }
    if (const BlobEntry* e = P.find(BLOB_SKCH)) {
        BlobCursor c(b, *e);
        auto& K = R.sketch;
        K.on = true;
        const long long ell = c.i(), fill = c.i(); K.count = c.i(); K.shrinks = c.i(); const long long given = c.i(); K.Delta = c.f();
        // (a commit that fills the buffer shrinks it in the same call: a saved fill is below 2 ell, and at least ell behind a shrink)
        if (!c.ok || ell < CHAIN_SKETCH_ELL_MIN || ell > CHAIN_SKETCH_ELL_MAX || fill < 0 || fill >= 2 * ell || K.count < 0 || K.shrinks < 0 ||
            (given != 0 && given != 1) || !std::isfinite(K.Delta) || K.Delta < 0.0 || (K.shrinks == 0 ? (fill != K.count || K.Delta != 0.0) : (fill < ell || K.count < 2 * ell)))
            return bad("SKCH: need 2 <= ell <= 64, 0 <= fill < 2 ell, counters that belong together and a finite Delta >= 0");
        K.ell = (int)ell; K.fill = (int)fill; K.given = given != 0;
        K.x0 = c.arr(n * D); K.tot = c.arr(n * D); K.q = c.arr(n * D); K.B = c.arr((uint64_t)fill * n * D);
        if (!c.ok || c.left) return bad("SKCH: wrong length");
        if (!blob_finite(K.x0, n, false) || !blob_finite(K.tot, n, false) || !blob_finite(K.q, n, false) || !blob_finite(K.B, (uint64_t)fill * n, false))
            return bad("SKCH: a pivot, a sum or a row is not finite");
    }
    return 0;
}

// the chain of a checked blob on the device: the context has no chain when this begins; the caller releases what a failure leaves
static int chain_blob_build(hmcmt_ctx* ctx, const BlobChain& R) {
    const char* fn = "hmcmt_chain_restore";
    auto& C = ctx->chain;
    auto& M = ctx->mass;
    const int nAC = ctx->v.nAC, nData = ctx->v.nData;
    const size_t n = (size_t)nAC, D = sizeof(double), vb = n * D, pb = 2 * (size_t)nData * D;
    hipStream_t st = ctx->stream;
    int rc;
    auto up = [&](void* dst, const unsigned char* src, size_t bytes) -> int {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        return 0;
    };
    // the mass first: what hmcmt_chain_set_mass_diag / hmcmt_chain_set_mass_lowrank leave, with the blob's bits
    if (R.mass.kind != HMCMT_MASS_WM) {
        double *d_s = nullptr, *d_U = nullptr, *d_c = nullptr, *d_part = nullptr;
        if (R.mass.cap > 0 && (rc = mass_lr_alloc(ctx, R.mass.cap, &d_s, &d_U, &d_c, &d_part))) {
            (void)hipGetLastError();
            mass_lr_free(ctx, {d_s, d_U, d_c, d_part});
            ctx->err = std::string(fn) + ": device allocation failed (the low-rank mass)";
            return HMCMT_ENOMEM;
        }
        mass_lr_release(ctx);
        M.kind = HMCMT_MASS_DIAGONAL;
        M.d_lrS = d_s; M.d_lrU = d_U; M.d_lrC = d_c; M.d_lrPart = d_part;
        M.lrCap = R.mass.cap;
        if ((rc = up(ctx->d_invM, R.mass.invM, vb))) return rc;
        if (R.mass.kind == HMCMT_MASS_LOWRANK) {
            const int r = R.mass.rank;
            M.lrLambda.resize((size_t)r);
            std::memcpy(M.lrLambda.data(), R.mass.lambda, (size_t)r * D);
            std::vector<double> c((size_t)2 * r);
            for (int k = 0; k < r; ++k) { c[k] = M.lrLambda[k] - 1.0; c[r + k] = 1.0 / std::sqrt(M.lrLambda[k]) - 1.0; }
            if ((rc = up(d_s, R.mass.s, vb)) || (rc = up(d_U, R.mass.U, (size_t)r * vb))) return rc;
            HIPCHK(hipMemcpyAsync(d_c, c.data(), (size_t)2 * r * D, hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));                // (c is this scope's)
            if (R.mass.given) { M.lrInvM.resize(n); std::memcpy(M.lrInvM.data(), R.mass.invM0, vb); }
            M.lrRank = r;
            M.kind = HMCMT_MASS_LOWRANK;
        }
    }
    // the chain's own buffers, as hmcmt_chain_begin makes them
    const std::pair<double**, size_t> bufs[] = {
        {&C.d_m[0], n}, {&C.d_m[1], n}, {&C.d_p, n}, {&C.d_z, n}, {&C.d_mean, n}, {&C.d_m2, n},
        {&C.d_pred[0], (size_t)2 * nData}, {&C.d_pred[1], (size_t)2 * nData}, {&C.d_part, (size_t)2 * LFNB}, {&C.d_scal, (size_t)CHAIN_SCAL}};
    for (const auto& b : bufs)
        if ((rc = chain_alloc(ctx, b.first, b.second))) { ctx->err = std::string(fn) + ": device allocation failed (the chain)"; return rc; }
    if (hipHostMalloc((void**)&C.h_rec, sizeof(double) * (CHAIN_REC + LFNB), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        C.h_rec = nullptr;
        ctx->err = std::string(fn) + ": pinned allocation failed";
        return HMCMT_ENOMEM;
    }
    if ((rc = up(C.d_m[0], R.m, vb)) || (rc = up(C.d_pred[0], R.pred, pb)) || (rc = up(C.d_mean, R.mean, vb)) || (rc = up(C.d_m2, R.m2, vb))) return rc;
    C.dt = R.dt; C.regParam = R.regParam; C.lo = R.lo; C.hi = R.hi; C.D = R.D; C.M = R.M; C.K0 = 0;
    C.burnin = R.burnin; C.nsamples = R.nsamples; C.nmoments = R.nmoments;
    C.seeded = R.seeded; C.seed = R.seed; C.t = R.t; C.stream = R.stream;
    C.cur = 0; C.nextStart = 0; C.haveMomentum = false;
    // a list of cells and the buffers of an accumulator: allocated, zeroed where the blob holds only a part, filled
    auto make = [&](std::vector<void*>& owner, void** p, size_t bytes, const unsigned char* src, size_t have) -> int {
        int r = have < bytes ? chain_acc_zeroed(ctx, fn, owner, p, std::max<size_t>(bytes, 1)) : chain_acc_alloc(ctx, fn, owner, p, std::max<size_t>(bytes, 1));
        if (!r && src) r = up(*p, src, have);
        return r;
    };
    if (R.hist.on) {
        auto& H = C.hist;
        const size_t cb = (size_t)R.hist.ntarget * (size_t)R.hist.nbins * sizeof(unsigned int);
        if ((rc = make(H.allocs, (void**)&H.d_target, (size_t)R.hist.ntarget * 8, R.hist.target, (size_t)R.hist.ntarget * 8)) ||
            (rc = make(H.allocs, (void**)&H.d_counts, cb, R.hist.counts, cb))) return rc;
        H.ntarget = R.hist.ntarget; H.nbins = R.hist.nbins; H.lo = R.hist.lo; H.hi = R.hist.hi; H.count = R.hist.count;
        H.scale = (double)H.nbins / (H.hi - H.lo);           // (hmcmt_chain_hist_begin's two expressions)
        H.w = (H.hi - H.lo) / (double)H.nbins;
        H.on = true;
    }
    if (R.dmom.on) {
        auto& Q = C.dmom;
        if ((rc = make(Q.allocs, (void**)&Q.d_mean, pb, R.dmom.mean, pb)) || (rc = make(Q.allocs, (void**)&Q.d_m2, pb, R.dmom.m2, pb))) return rc;
        Q.count = R.dmom.count;
        Q.on = true;
    }
    if (R.acov.on) {
        auto& A = C.acov;
        const size_t tb = (size_t)R.acov.ntarget * D, lb = tb * (size_t)(R.acov.K + 1);
        if (!R.acov.all && (rc = make(A.allocs, (void**)&A.d_target, tb, R.acov.target, tb))) return rc;
        if ((rc = make(A.allocs, (void**)&A.d_x0, tb, R.acov.x0, tb)) || (rc = make(A.allocs, (void**)&A.d_tot, tb, R.acov.tot, tb)) ||
            (rc = make(A.allocs, (void**)&A.d_S, lb, R.acov.S, lb)) || (rc = make(A.allocs, (void**)&A.d_H, lb, R.acov.H, lb)) ||
            (rc = make(A.allocs, (void**)&A.d_ring, lb, R.acov.ring, lb))) return rc;
        A.ntarget = R.acov.ntarget; A.K = R.acov.K; A.count = R.acov.count;
        A.on = true;
    }
    if (R.cov.on) {
        auto& V = C.cov;
        const size_t rb = (size_t)R.cov.nrow * 8;
        if (!R.cov.all && (rc = make(V.allocs, (void**)&V.d_row, rb, R.cov.row, rb))) return rc;
        if ((rc = make(V.allocs, (void**)&V.d_x0, vb, R.cov.x0, vb)) || (rc = make(V.allocs, (void**)&V.d_tot, vb, R.cov.tot, vb)) ||
            (rc = make(V.allocs, (void**)&V.d_q, vb, R.cov.q, vb)) ||
            (rc = make(V.allocs, (void**)&V.d_pend, vb * (size_t)R.cov.B, R.cov.pend, vb * (size_t)R.cov.npend)) ||
            (rc = make(V.allocs, (void**)&V.d_S, vb * (size_t)R.cov.nrow, R.cov.S, vb * (size_t)R.cov.nrow))) return rc;
        V.nrow = R.cov.nrow; V.B = R.cov.B; V.npend = R.cov.npend; V.count = R.cov.count;
        V.on = true;
    }
    if (R.adapt.on) {
        auto& A = C.adapt;
        if (R.adapt.opt.adapt_mass && ((rc = make(A.allocs, (void**)&A.d_mean, vb, R.adapt.mean, vb)) || (rc = make(A.allocs, (void**)&A.d_m2, vb, R.adapt.m2, vb))))
            return rc;
        A.opt = R.adapt.opt; A.da = R.adapt.da;
        A.c = R.adapt.c; A.wcount = R.adapt.wcount; A.wnext = R.adapt.wnext; A.wsize = R.adapt.wsize; A.windowsDone = R.adapt.windowsDone;
        A.alphaLast = R.adapt.alphaLast; A.alphaSum = R.adapt.alphaSum;
        if (R.lr.on) {
            auto& L = A.lr;
            const size_t ms = (size_t)R.lr.opt.max_samples, rk = (size_t)R.lr.opt.rank, have = (size_t)R.lr.rows * vb;
            if ((rc = make(A.allocs, (void**)&L.d_X, ms * vb, R.lr.X, have)) || (rc = make(A.allocs, (void**)&L.d_G, ms * vb, R.lr.G, have))) return rc;
            const std::pair<double**, size_t> stage[] = {{&L.d_K, 4 * ms * ms * D}, {&L.d_B, 2 * ms * rk * D}, {&L.d_meanX, vb}, {&L.d_meanG, vb},
                                                         {&L.d_s, vb}, {&L.d_U, rk * vb}, {&L.d_c, 2 * rk * D}, {&L.d_part, rk * LFNB * D}};
            for (const auto& s : stage)
                if ((rc = chain_acc_zeroed(ctx, fn, A.allocs, (void**)s.first, s.second))) return rc;
            L.opt = R.lr.opt;
            L.winStart = R.lr.winStart; L.stride = R.lr.stride;
            L.stored = R.lr.stored; L.skipped = R.lr.skipped; L.closedStored = R.lr.closedStored;
            L.last = R.lr.last;
            L.on = true;
        }
        A.begun = true;
        A.active = R.adapt.active;
    }
    if (R.sketch.on) {
        auto& K = C.sketch;
        const size_t rows = (size_t)2 * R.sketch.ell + 1;
        const size_t stage = std::max((size_t)R.sketch.ell * 2 * R.sketch.ell, rows * (size_t)HMCMT_MASS_RANK_MAX);
        if ((rc = make(K.allocs, (void**)&K.d_B, rows * vb, R.sketch.B, (size_t)R.sketch.fill * vb)) ||
            (rc = make(K.allocs, (void**)&K.d_x0, vb, R.sketch.x0, vb)) || (rc = make(K.allocs, (void**)&K.d_tot, vb, R.sketch.tot, vb)) ||
            (rc = make(K.allocs, (void**)&K.d_q, vb, R.sketch.q, vb)) ||
            (rc = chain_acc_zeroed(ctx, fn, K.allocs, (void**)&K.d_K, rows * rows * D)) ||
            (rc = chain_acc_zeroed(ctx, fn, K.allocs, (void**)&K.d_T, stage * D))) return rc;
        K.hK.assign(rows * rows, 0.0);
        K.ell = R.sketch.ell; K.fill = R.sketch.fill; K.count = R.sketch.count; K.shrinks = R.sketch.shrinks; K.Delta = R.sketch.Delta;
        K.pivotGiven = R.sketch.given;
        K.on = true;
    }
    HIPCHK(hipStreamSynchronize(st));                        // (the caller's blob is free again on return)
    HIPCHK(hipGetLastError());
    ctx->lfHaveGrad = false;
    C.gen = ctx->stateGen;
    C.active = true;
    return 0;
}

int hmcmt_chain_restore(hmcmt_ctx* ctx, const void* buf, uint64_t bytes) {
    const char* fn = "hmcmt_chain_restore";
    if (!ctx) return HMCMT_EINVAL;
    if (!buf) { ctx->err = std::string(fn) + ": buf is NULL"; return HMCMT_EINVAL; }
    int rc = chain_ready(ctx, fn, false);
    if (rc) return rc;
    if (!ctx->havePrior) { ctx->err = std::string(fn) + ": hmcmt_set_prior has not been called"; return HMCMT_EINVAL; }
    BlobParsed P;
    BlobChain R{};
    std::string why;
    if ((rc = blob_parse(buf, bytes, P, why))) { ctx->err = std::string(fn) + ": " + why; return rc; }
    if ((rc = chain_blob_check(ctx, (const unsigned char*)buf, P, R))) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));               // (a commit of the chain this one replaces may still be running)
    chain_release(ctx);
    if ((rc = chain_blob_build(ctx, R))) {                   // the context stays usable, without a chain
        const std::string e = ctx->err;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
        chain_release(ctx);
        ctx->err = e;
        return rc;
    }
    return 0;
}

int hmcmt_chain_end(hmcmt_ctx* ctx) {
    if (!ctx) return HMCMT_EINVAL;
    if (ctx->statsPending) { ctx->err = "hmcmt_chain_end: an asynchronous evaluation is in flight (hmcmt_wait first)"; return HMCMT_EINVAL; }
    chain_release(ctx);
    return 0;
}
