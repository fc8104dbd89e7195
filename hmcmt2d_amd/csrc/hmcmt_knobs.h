// The one reader of the library's environment variables: read_knobs is called once per hmcmt_create and
// gives the raw, mesh-independent reading of every variable -- one line per variable.  What a value means for a given mesh (the
// tile heights, the boundary-field shapes, the launch shapes) is resolved next to the heuristic it overrides (make_config,
// hmcmt_hip.hip).  Plain C++17, no HIP: tests/emul/emul_knobs.cpp holds the rules below to literals (tests/test_knobs_host.py).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>

namespace hmcmt {

// the constants of the kernel headers that bound a knob: EXT_NP (hmcmt_items.h), STALL_IT (kernels_fused.h), PS_SPIN_LIMIT
// (kernels_persist.h)
struct KnobLimits { int extNp; int stallIt; unsigned psSpinLimit; };

enum KnobStamps { STAMPS_NONE = 0, STAMPS_UPD = 1, STAMPS_SPMV = 2, STAMPS_PERSIST = 3 };   // (1, 2: Solver::stampKernel)

struct Knobs {
    // present means on (a set-but-empty value counts)
    bool wantTicks = false;               // HMCMT_TICKS: in-kernel wall-clock stamps (View::ticks), printed at destroy
    bool noFusedStart = false, noSigmaRows = false, noCoefAll = false;     // HMCMT_NO_FUSED_START / _NO_SIGMA_ROWS / _NO_COEF_ALL
    bool fwdStamps = false, backStamps = false;      // HMCMT_FWD_STAMPS / HMCMT_BACK_STAMPS: per-block stamps of k_fdm_fwd / k_back_post (debug entries only)
    // on unless the first character is '0'
    bool persist = true;                  // HMCMT_PERSIST=0: the launch-per-phase loop only (the initial SolveState::persistOn)
    bool psInKernelStart = true;          // HMCMT_PS_START=0: k_resid0 / k_solve_begin in launches of their own, as until round 5 (A/B)
    bool psBalance = true;                // HMCMT_PERSIST_BALANCE=0: never
    bool twistOn = true;                  // HMCMT_TWIST=0: classic one-sided sweeps in the fused kernel as well
    bool fusedBack = true;                // HMCMT_FUSED_BACK=0: back transform and post-smoother in separate kernels
    bool specOn = true;                   // HMCMT_SPEC=0: followers are queued after the host has seen the solve's outcome
    bool lazyDinv = true;                 // HMCMT_LAZY_DINV=0: k_coef_all writes every system's Jacobi diagonal in every evaluation, as until round 6 (A/B)
    bool streamPriority = true;           // HMCMT_STREAM_PRIORITY=0: both streams at the default priority
    bool persistWidthK = true;            // HMCMT_PERSIST_WIDTHK=0: the generic persistent kernels, not the width-specialised ones (A/B runs, tests)
    bool persistLock = true;              // HMCMT_PERSIST_LOCK=0: no advisory lock per device
    // tri-state on the first character
    int fusedFwdMode = 1;                 // HMCMT_FUSED_FWD: '0' -> 0 separate kernels, '2' -> 2 forced, else 1 (where the heuristic prefers it)
    int sensFusedMode = 2;                // HMCMT_SENS_FUSED: '0' -> 0 never, '1' -> 1 always, else 2 automatic
    int xfwd = -1;                        // HMCMT_XFWD: unset -1 (the size heuristic), '0' -> 0 off, else 1 on
    // atoi / atol, then clamp
    unsigned persistSpin = 0;             // HMCMT_PS_SPIN: polls before a wait of the persistent kernel gives up, >= 1024 (default: PS_SPIN_LIMIT)
    int sweepsMode = 0;                   // HMCMT_SWEEPS: 1 / 2 damped Jacobi sweeps on each side of the FDM stage, 0 (default) = per solve
    int sweepsUp = 12, sweepsDown = 6;    // HMCMT_SWEEPS_UP (>= 1) / HMCMT_SWEEPS_DOWN (>= 0).  auto: one sweep -> two above sweepsUp iterations (rounds 2-4: 30 -- a two-sweep iteration of the launch-per-phase loop cost 1.20 one-sweep
                                          // ones; in the persistent kernel 1.15 / 1.10, and solves of 18-24 iterations near the true model gain 2-7 % from two), two -> one below sweepsDown (12: the first,
                                          // cheap steps of every clamped burn-in trajectory switched back and the next ones up again)
    int guardEvery = 100;                 // HMCMT_GUARD_EVERY (>= 0; 0: off): the initial SolveState::guardEvery
    int extrapNp = 0;                     // HMCMT_EXTRAP_POINTS = 2..EXT_NP (default: EXT_NP)
    int stallIt = 0;                      // HMCMT_STALL_IT (>= 1; default: STALL_IT)
    int sideIt = 0;                       // HMCMT_SIDE_IT = n > 0: the adjoint side launches at iteration n; 0: automatic
    int eventFlags = 1;                   // HMCMT_EVENT_FLAGS: 1 hipEventDisableSystemFence, 2 hipEventReleaseToDevice, else 0 system-scope release
    int debugFlags = 0;                   // HMCMT_DEBUG_FLAGS: the initial SolveState::dbgFlags (hmcmt_debug_flags)
    int persistCsForce = 0;               // HMCMT_PERSIST_CS = 1 | 2 forces the persistent kernel's column parts; 0: not forced
    int persistStrips = 2;                // HMCMT_PERSIST_STRIPS: only 4 selects the four-strip kernel
    // atoi, accepted only from a set (0: not given, the heuristic's choice)
    int resid = 0, upd1 = 0, spmv = 0;    // HMCMT_RESID {256, 512, 1024}, HMCMT_UPD1 {256, 512}, HMCMT_SPMV {256, 512, 1024}
    // atof
    double jacobiW = 0.8;                 // HMCMT_JACOBI_W in [0.1, 1.2]: damping of the point-Jacobi halves (0.7 in round 1: 0.8 saves 3-8 % of the iterations on structured models, costs 6-25 % on white-noise models of std >= 1)
    float psSmooth = 0.75f;               // HMCMT_PERSIST_BALANCE_SMOOTH in [0, 0.95]: weight of the older costs (cfg5, 96-step chains: 0 -> 84.3, 0.5 -> 84.8, 0.75 -> 85.0 steps/s, index order 83.4)
    double guardLimit = 1e-6;             // HMCMT_GUARD_LIMIT: a checked residual above it is a "trip" (warning, next evaluation starts cold)
    float w2 = 1.0f;                      // HMCMT_JACOBI_W2 (Solver::w2)
    // overrides of mesh-dependent choices: "given" and the raw integers
    bool rtGiven = false, rt2Given = false, rtsGiven = false, bcFusedGiven = false;
    int rt = 0, rt2 = 0, rts = 0, bcFused = 0;       // HMCMT_RT / HMCMT_RT2 / HMCMT_RTS / HMCMT_BC_FUSED
    int upd2N = 0, upd2[3] = {0, 0, 0};              // HMCMT_UPD2 = "threads,batch,rows": fields parsed, their values
    int bcBlockedN = 0, bcBlocked[4] = {0, 0, 0, 0}; // HMCMT_BC_BLOCKED = "columns[,threads[,up layers[,down layers]]]": likewise
    // strings
    int stamps = STAMPS_NONE;             // HMCMT_STAMPS = upd | spmv | persist
    std::string lockDir = "/tmp";         // HMCMT_LOCK_DIR (empty counts as unset)
};

namespace knob {
template <class L> bool present(L& env, const char* name) { return env(name) != nullptr; }
template <class L> bool on_unless_0(L& env, const char* name) { const char* e = env(name); return !(e && e[0] == '0'); }
// first character `a` -> va, `b` -> vb, anything else that is set -> other, unset -> unset
template <class L> int tri(L& env, const char* name, char a, int va, char b, int vb, int other, int unset) {
    const char* e = env(name);
    return !e ? unset : e[0] == a ? va : e[0] == b ? vb : other;
}
template <class L> long raw_long(L& env, const char* name, long def) { const char* e = env(name); return e ? atol(e) : def; }
template <class L> int raw_int(L& env, const char* name, int def, bool* given = nullptr) {
    const char* e = env(name);
    if (given) *given = e != nullptr;
    return e ? atoi(e) : def;
}
template <class L> double clamped_f(L& env, const char* name, double def, double lo, double hi) {
    const char* e = env(name);
    return e ? std::min(hi, std::max(lo, atof(e))) : def;
}
template <class L> double raw_f(L& env, const char* name, double def) { const char* e = env(name); return e ? atof(e) : def; }
// unset -> unset, a member of the set -> itself, anything else -> 0
template <class L> int one_of(L& env, const char* name, std::initializer_list<int> set, int unset = 0) {
    const char* e = env(name);
    if (!e) return unset;
    const int v = atoi(e);
    return std::find(set.begin(), set.end(), v) != set.end() ? v : 0;
}
// "%d,%d,.." into out[0..n): the number of fields parsed
template <class L> int tuple(L& env, const char* name, int* out, int n) {
    const char* e = env(name);
    if (!e) return 0;
    int v[4] = {0, 0, 0, 0};
    const int got = std::max(0, sscanf(e, "%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3]));
    for (int i = 0; i < std::min(got, n); ++i) out[i] = v[i];
    return std::min(got, n);
}
}  // namespace knob

template <class Lookup>
Knobs read_knobs(Lookup& env, const KnobLimits& lim) {
    using namespace knob;
    Knobs k;
    k.wantTicks = present(env, "HMCMT_TICKS");
    k.noFusedStart = present(env, "HMCMT_NO_FUSED_START");
    k.noSigmaRows = present(env, "HMCMT_NO_SIGMA_ROWS");
    k.noCoefAll = present(env, "HMCMT_NO_COEF_ALL");
    k.fwdStamps = present(env, "HMCMT_FWD_STAMPS");
    k.backStamps = present(env, "HMCMT_BACK_STAMPS");
    k.persist = on_unless_0(env, "HMCMT_PERSIST");
    k.psInKernelStart = on_unless_0(env, "HMCMT_PS_START");
    k.psBalance = on_unless_0(env, "HMCMT_PERSIST_BALANCE");
    k.twistOn = on_unless_0(env, "HMCMT_TWIST");
    k.fusedBack = on_unless_0(env, "HMCMT_FUSED_BACK");
    k.specOn = on_unless_0(env, "HMCMT_SPEC");
    k.lazyDinv = on_unless_0(env, "HMCMT_LAZY_DINV");
    k.streamPriority = on_unless_0(env, "HMCMT_STREAM_PRIORITY");
    k.persistWidthK = on_unless_0(env, "HMCMT_PERSIST_WIDTHK");
    k.persistLock = on_unless_0(env, "HMCMT_PERSIST_LOCK");
    k.fusedFwdMode = tri(env, "HMCMT_FUSED_FWD", '0', 0, '2', 2, 1, 1);
    k.sensFusedMode = tri(env, "HMCMT_SENS_FUSED", '0', 0, '1', 1, 2, 2);
    k.xfwd = tri(env, "HMCMT_XFWD", '0', 0, '0', 0, 1, -1);
    k.persistSpin = (unsigned)std::max(1024l, raw_long(env, "HMCMT_PS_SPIN", (long)lim.psSpinLimit));
    k.sweepsMode = std::max(0, std::min(2, raw_int(env, "HMCMT_SWEEPS", 0)));
    k.sweepsUp = std::max(1, raw_int(env, "HMCMT_SWEEPS_UP", 12));
    k.sweepsDown = std::max(0, raw_int(env, "HMCMT_SWEEPS_DOWN", 6));
    k.guardEvery = std::max(0, raw_int(env, "HMCMT_GUARD_EVERY", 100));
    k.extrapNp = std::max(2, std::min(lim.extNp, raw_int(env, "HMCMT_EXTRAP_POINTS", lim.extNp)));
    k.stallIt = std::max(1, raw_int(env, "HMCMT_STALL_IT", lim.stallIt));
    k.sideIt = std::max(0, raw_int(env, "HMCMT_SIDE_IT", 0));
    k.eventFlags = one_of(env, "HMCMT_EVENT_FLAGS", {1, 2}, 1);
    k.debugFlags = raw_int(env, "HMCMT_DEBUG_FLAGS", 0);
    k.persistCsForce = raw_int(env, "HMCMT_PERSIST_CS", 0);
    k.persistStrips = raw_int(env, "HMCMT_PERSIST_STRIPS", 2);
    k.resid = one_of(env, "HMCMT_RESID", {256, 512, 1024});
    k.upd1 = one_of(env, "HMCMT_UPD1", {256, 512});
    k.spmv = one_of(env, "HMCMT_SPMV", {256, 512, 1024});
    k.jacobiW = clamped_f(env, "HMCMT_JACOBI_W", 0.8, 0.1, 1.2);
    k.psSmooth = (float)clamped_f(env, "HMCMT_PERSIST_BALANCE_SMOOTH", 0.75, 0.0, 0.95);
    k.guardLimit = raw_f(env, "HMCMT_GUARD_LIMIT", 1e-6);
    k.w2 = (float)raw_f(env, "HMCMT_JACOBI_W2", 1.0);
    k.rt = raw_int(env, "HMCMT_RT", 0, &k.rtGiven);
    k.rt2 = raw_int(env, "HMCMT_RT2", 0, &k.rt2Given);
    k.rts = raw_int(env, "HMCMT_RTS", 0, &k.rtsGiven);
    k.bcFused = raw_int(env, "HMCMT_BC_FUSED", 0, &k.bcFusedGiven);
    k.upd2N = tuple(env, "HMCMT_UPD2", k.upd2, 3);
    k.bcBlockedN = tuple(env, "HMCMT_BC_BLOCKED", k.bcBlocked, 4);
    if (const char* e = env("HMCMT_STAMPS")) k.stamps = !strcmp(e, "upd") ? STAMPS_UPD : !strcmp(e, "spmv") ? STAMPS_SPMV : !strcmp(e, "persist") ? STAMPS_PERSIST : STAMPS_NONE;
    if (const char* e = env("HMCMT_LOCK_DIR")) if (e[0]) k.lockDir = e;
    return k;
}

}  // namespace hmcmt
