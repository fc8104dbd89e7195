// TEST-ONLY stand-alone program over hmcmt2d_amd/csrc/hmcmt_knobs.h (tests/test_knobs_host.py): prints what read_knobs makes of
// the environment it runs in, one "NAME value" line per variable, or with --list the names read_knobs asks for.
//   flags and switches 0 / 1; tri-states their code; HMCMT_RT, _RT2, _RTS, _BC_FUSED "unset" or the raw integer; HMCMT_UPD2 and
//   HMCMT_BC_BLOCKED the parsed fields joined by commas ("-" for none); HMCMT_STAMPS none | upd | spmv | persist
#include "../../hmcmt2d_amd/csrc/hmcmt_knobs.h"
#include <cstdio>
#include <set>
#include <string>

using namespace hmcmt;

struct Env { const char* operator()(const char* name) { return getenv(name); } };
struct Recording {
    std::set<std::string> names;
    const char* operator()(const char* name) { names.insert(name); return nullptr; }
};

static std::string fields(const int* v, int n) {
    std::string s;
    for (int i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return n ? s : "-";
}
static std::string given(bool g, int v) { return g ? std::to_string(v) : "unset"; }

int main(int argc, char** argv) {
    const KnobLimits lim{6, 30, 1u << 22};       // EXT_NP, STALL_IT, PS_SPIN_LIMIT of the kernel headers
    if (argc > 1 && std::string(argv[1]) == "--list") {
        Recording rec;
        read_knobs(rec, lim);
        for (const std::string& n : rec.names) printf("%s\n", n.c_str());
        return 0;
    }
    Env env;
    const Knobs k = read_knobs(env, lim);
    static const char* const stamps[] = {"none", "upd", "spmv", "persist"};
#define I(name, v) printf("%s %lld\n", name, (long long)(v))
#define F(name, v) printf("%s %.9g\n", name, (double)(v))
#define S(name, v) printf("%s %s\n", name, std::string(v).c_str())
    I("HMCMT_TICKS", k.wantTicks); I("HMCMT_NO_FUSED_START", k.noFusedStart); I("HMCMT_NO_SIGMA_ROWS", k.noSigmaRows);
    I("HMCMT_NO_COEF_ALL", k.noCoefAll); I("HMCMT_FWD_STAMPS", k.fwdStamps); I("HMCMT_BACK_STAMPS", k.backStamps);
    I("HMCMT_PERSIST", k.persist); I("HMCMT_PS_START", k.psInKernelStart); I("HMCMT_PERSIST_BALANCE", k.psBalance);
    I("HMCMT_TWIST", k.twistOn); I("HMCMT_FUSED_BACK", k.fusedBack); I("HMCMT_SPEC", k.specOn); I("HMCMT_LAZY_DINV", k.lazyDinv);
    I("HMCMT_STREAM_PRIORITY", k.streamPriority); I("HMCMT_PERSIST_WIDTHK", k.persistWidthK); I("HMCMT_PERSIST_LOCK", k.persistLock);
    I("HMCMT_FUSED_FWD", k.fusedFwdMode); I("HMCMT_SENS_FUSED", k.sensFusedMode); I("HMCMT_XFWD", k.xfwd);
    I("HMCMT_PS_SPIN", k.persistSpin); I("HMCMT_SWEEPS", k.sweepsMode); I("HMCMT_SWEEPS_UP", k.sweepsUp); I("HMCMT_SWEEPS_DOWN", k.sweepsDown);
    I("HMCMT_GUARD_EVERY", k.guardEvery); I("HMCMT_EXTRAP_POINTS", k.extrapNp); I("HMCMT_STALL_IT", k.stallIt); I("HMCMT_SIDE_IT", k.sideIt);
    I("HMCMT_EVENT_FLAGS", k.eventFlags); I("HMCMT_DEBUG_FLAGS", k.debugFlags); I("HMCMT_PERSIST_CS", k.persistCsForce);
    I("HMCMT_PERSIST_STRIPS", k.persistStrips); I("HMCMT_RESID", k.resid); I("HMCMT_UPD1", k.upd1); I("HMCMT_SPMV", k.spmv);
    F("HMCMT_JACOBI_W", k.jacobiW); F("HMCMT_PERSIST_BALANCE_SMOOTH", k.psSmooth); F("HMCMT_GUARD_LIMIT", k.guardLimit); F("HMCMT_JACOBI_W2", k.w2);
    S("HMCMT_RT", given(k.rtGiven, k.rt)); S("HMCMT_RT2", given(k.rt2Given, k.rt2)); S("HMCMT_RTS", given(k.rtsGiven, k.rts));
    S("HMCMT_BC_FUSED", given(k.bcFusedGiven, k.bcFused));
    S("HMCMT_UPD2", fields(k.upd2, k.upd2N)); S("HMCMT_BC_BLOCKED", fields(k.bcBlocked, k.bcBlockedN));
    S("HMCMT_STAMPS", stamps[k.stamps]); S("HMCMT_LOCK_DIR", k.lockDir);
    return 0;
}
