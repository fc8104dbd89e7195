"""The seeded device chain (hmcmt_chain_seed, hmcmt_chain_sample, hmcmt_chain_run; k_chain_draw_momentum, k_chain_draw_clip): the
device's normals against tests/rng_ref.py, a seeded chain bit for bit against the host-fed chain that is handed the library's own
numbers -- under the diagonal, the Wm and the low-rank mass --, a run against its samples one by one, with the accumulators and a
warm-up riding on the commit, the state rules of the generator, and the sampler's library_rng keyword.  Sizes: one partly filled
workgroup (tiny, 96 parameters), a full one plus a partial one (the ragged problem, 390); the normals also at the second grid-stride
pass (cfg3, 20000)."""
import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd.lib import HmcmtError
from tests import rng_ref as R
from tests.test_gpu_chain import prior_of, run, same_bits
from tests.test_gpu_chain_adapt import REC_KEYS, WINDOWS, begin_accumulators, bits, read_accumulators, rec_bits
from tests.test_gpu_chain_kernels import FORCE, HI, LO, REG, problem

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
LD = np.longdouble
SEED = 0x5EED0123456789AB
LMIN, LMAX = 6, 10
T_HIGH = (1 << 32) + 5                          # a draw whose index reaches the counter's fourth word
MASSES = ["diagonal", "wm", "lowrank"]


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def context(P, mass="diagonal"):
    """a context with the problem's prior and non-unit diagonal; "wm": M = Wm; "lowrank": five directions on top of the diagonal"""
    ctx = P.context("wm" if mass == "wm" else None)
    if mass == "lowrank":
        try:
            rng = np.random.default_rng(P.n + 5)
            U = np.linalg.qr(rng.standard_normal((P.n, 5)))[0].T
            ctx.set_mass_lowrank(None, U, rng.uniform(0.3, 3.0, 5))
        except Exception:
            ctx.close()
            raise
    return ctx


def begin(ctx, P, stream=0, burnin=1, seed=SEED):
    D, Mn = ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=burnin)
    ctx.chain_seed(seed, stream)
    return D, Mn


# ---- 1. the device's normals ------------------------------------------------------------------------------------------------------
_ref_normals = {}


def ref_clipped(stream, t, n):
    """clip(rng_ref.normals) of the first n cells: computed once per (stream, t) at the largest n asked for, shared, left unchanged"""
    key = (stream, t)
    if key not in _ref_normals or len(_ref_normals[key]) < n:
        _ref_normals[key] = R.clipped(R.normals(SEED, stream, t, n))
    return _ref_normals[key][:n]


@pytest.mark.parametrize("name,draws", [("tiny", [(0, 0), (0, T_HIGH), (3, 0), (3, T_HIGH)]), ("ragged", [(0, 0), (0, T_HIGH), (3, 0), (3, T_HIGH)]),
                                        ("cfg3", [(0, 0), (3, T_HIGH)])])
def test_device_normals_against_the_reference(name, draws):
    """hmcmt_chain_normals(t) = k_chain_draw_clip against clip(rng_ref, +-2.5) within rng_ref.NORMAL_TOL (4e-14 absolute, derived
    there), host and device read-out bit for bit, for t = 0 and t = 2^32 + 5 and two streams.  No cell is left out or written twice:
    every value is its own cell's."""
    import torch
    P = problem(name)
    ctx = context(P)
    try:
        worst = 0.0
        for stream, t in draws:
            begin(ctx, P, stream)
            z = ctx.chain_normals(t)
            d = torch.full((P.n + 8,), 7.0, dtype=torch.float64, device=torch.device("cuda", 0))
            torch.cuda.synchronize()
            ctx.chain_normals(t, d_z=d.data_ptr())
            dz = d.cpu().numpy()
            assert np.array_equal(dz[:P.n], z) and np.all(dz[P.n:] == 7.0)               # (nothing is written behind nAC)
            ref = ref_clipped(stream, t, P.n)
            err = float(np.abs(z.astype(LD) - ref).max())
            worst = max(worst, err)
            assert np.abs(z).max() <= 2.5 and int((np.abs(z) == 2.5).sum()) == int((np.abs(ref) == LD(2.5)).sum())      # (the clip's cells)
            assert len(set(z[np.abs(z) < 2.5].tolist())) == int((np.abs(z) < 2.5).sum())                                # (no value twice)
            assert ctx.chain_rng_state() == (SEED, stream, 0)                             # (a read-out moves nothing)
        print(f"\n[device normals, {name}] nAC {P.n}: largest |z - clip(ref)| {worst:.3g} (bound {R.NORMAL_TOL})")
        assert worst <= R.NORMAL_TOL
    finally:
        ctx.close()


# ---- 2. a seeded chain is the host-fed chain that is handed the library's numbers -----------------------------------------------------
FORCED = "-AR-RA"                               # per sample: A / R forces the decision through chain_set_energy, - leaves it to the draw


def chain_by_hand(P, mass, how, stream=2, forced=FORCED):
    """len(forced) samples on a context of its own.  how = "seeded": chain_sample(LMIN, LMAX).  how = "fed": chain_momentum with the
    clipped normals chain_normals(t) returns (the clip is idempotent), then chain_step with rng_draw's L and u of draw t."""
    ctx = context(P, mass)
    try:
        D, Mn = begin(ctx, P, stream)
        out = {"recs": [], "models": [], "preds": [], "states": [], "Ls": []}
        for t, force in enumerate(forced):
            if force in "AR":
                ctx.chain_set_energy(D + FORCE if force == "A" else D - FORCE, Mn)
            if how == "seeded":
                assert ctx.chain_rng_state() == (SEED, stream, t)
                rec, m, pred = ctx.chain_sample(LMIN, LMAX)
            else:
                z = ctx.chain_normals(t)
                K = ctx.chain_momentum(z)
                Lt, ut = L.rng_draw(SEED, stream, t, LMIN, LMAX)
                out["Ls"].append(Lt)
                rec, m, pred = ctx.chain_step(Lt, ut)
                assert rec["K0"] == K
                assert ctx.chain_rng_state() == (SEED, stream, 0)                         # (host-fed calls do not move t)
            if force in "AR":
                assert rec["accepted"] == int(force == "A")
            if rec["accepted"]:
                D, Mn = rec["D"], rec["M"]
            elif force == "R":
                ctx.chain_set_energy(D, Mn)
            out["recs"].append(rec); out["models"].append(m); out["preds"].append(pred)
            out["states"].append(ctx.chain_state())
        out["moments"] = ctx.chain_moments()
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_seeded_chain_is_the_fed_chain_bit_for_bit(name, mass):
    P = problem(name)
    seeded, fed = chain_by_hand(P, mass, "seeded"), chain_by_hand(P, mass, "fed")
    acc = [r["accepted"] for r in seeded["recs"]]
    print(f"\n[seeded against fed, {name}, {mass}] L {fed['Ls']}, decisions {acc}, K0 {[round(r['K0'], 3) for r in seeded['recs']]}")
    assert 1 in acc and 0 in acc
    assert len(set(fed["Ls"])) > 1 and all(LMIN <= l <= LMAX for l in fed["Ls"])
    assert [r["nfevals"] for r in seeded["recs"]] == [r["nfevals"] for r in fed["recs"]]
    assert rec_bits(seeded["recs"]) == rec_bits(fed["recs"])
    for key in ("models", "preds"):
        assert bits(np.array(seeded[key])) == bits(np.array(fed[key])), key
    for a, b in zip(seeded["states"], fed["states"]):
        assert all(bits(x) == bits(y) for x, y in zip(a, b))                              # (model, momentum buffer, predicted data)
    assert seeded["moments"][0] == fed["moments"][0] == len(FORCED) - 1
    assert all(bits(a) == bits(b) for a, b in zip(seeded["moments"][1:], fed["moments"][1:]))


# ---- 3. a run is its samples ---------------------------------------------------------------------------------------------------------
NRUN = 8
LRUN = (1, 3)                                   # short trajectories, which this step size mostly accepts: the chains of this section move


def seeded_run(P, how, adapt=None, replay=None, accs=False, stream=1, nsamples=NRUN):
    """NRUN samples with drawn decisions on a context of its own.  how = "run": one chain_run; "samples": chain_sample one by one, with
    the step size and the mass in force read out in front of each; replay: an earlier result of "samples" -- no adaptation, its step
    sizes and masses through the setters."""
    ctx = context(P)
    try:
        begin(ctx, P, stream, burnin=0)
        if accs:
            begin_accumulators(ctx, P.n)
        if adapt is not None:
            ctx.chain_adapt_begin(**adapt)
        out = {"dts": [], "masses": []}
        if how == "run":
            out["recs"], models, preds = ctx.chain_run(nsamples, *LRUN)
            out["models"], out["preds"] = list(models), list(preds)
        else:
            out.update(recs=[], models=[], preds=[])
            for it in range(nsamples):
                if replay is not None:
                    if it == 0 or bits(replay["masses"][it]) != bits(replay["masses"][it - 1]):
                        ctx.chain_set_mass_diag(replay["masses"][it])
                    ctx.chain_set_dt(replay["dts"][it])
                out["dts"].append(ctx.chain_adapt_info()["dt"] if adapt is not None else None)
                out["masses"].append(ctx.chain_mass_diag())
                rec, m, pred = ctx.chain_sample(*LRUN)
                out["recs"].append(rec); out["models"].append(m); out["preds"].append(pred)
        out["moments"] = ctx.chain_moments()
        out["rng"] = ctx.chain_rng_state()
        out["invM"] = ctx.chain_mass_diag()
        if accs:
            out["accs"] = read_accumulators(ctx)
        return out
    finally:
        ctx.close()


def assert_same_chain(a, b, accs=False):
    assert rec_bits(a["recs"]) == rec_bits(b["recs"])
    for key in ("models", "preds"):
        assert bits(np.array(a[key])) == bits(np.array(b[key])), key
    assert a["moments"][0] == b["moments"][0] and all(bits(x) == bits(y) for x, y in zip(a["moments"][1:], b["moments"][1:]))
    assert bits(a["invM"]) == bits(b["invM"])
    if accs:
        for key, got in a["accs"].items():
            assert all(bits(x) == bits(y) for x, y in zip(got, b["accs"][key])), key


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_run_is_its_samples_bit_for_bit(name):
    P = problem(name)
    whole, single = seeded_run(P, "run"), seeded_run(P, "samples")
    assert_same_chain(whole, single)
    assert whole["rng"] == single["rng"] == (SEED, 1, NRUN)
    assert [r["nsamples"] for r in whole["recs"]] == list(range(1, NRUN + 1)) and whole["moments"][0] == NRUN
    acc = [r["accepted"] for r in whole["recs"]]
    print(f"\n[run against samples, {name}] decisions {acc}")
    assert 1 in acc and 0 in acc and np.any(whole["moments"][2] > 0)                      # (the chain moves, and the moments see it)


def test_run_with_accumulators_and_a_warm_up_is_its_samples_and_their_replay():
    """a histogram and the other accumulators on the commit and a warm-up of 7 steps (one mass window, closed by step 5) under 8
    samples: the run equals the samples one by one, and both equal the chain without adaptation that is given the adapted chain's step
    sizes and masses through chain_set_dt and chain_set_mass_diag"""
    P = problem("tiny")
    adapt = dict(nwarmup=7, **WINDOWS)
    single = seeded_run(P, "samples", adapt=adapt, accs=True)
    whole = seeded_run(P, "run", adapt=adapt, accs=True)
    assert_same_chain(whole, single, accs=True)
    assert len({bits(m) for m in single["masses"]}) == 2 and len(set(single["dts"])) >= 6       # (the warm-up did adapt)
    assert_same_chain(seeded_run(P, "samples", replay=single, accs=True), single, accs=True)


# ---- 4. the state rules -------------------------------------------------------------------------------------------------------------
def test_state_rules_of_the_generator():
    P = problem("tiny")
    ctx = context(P)
    try:
        assert code_of(lambda: ctx.chain_seed(1, 0)) == EINVAL                            # no chain
        D, Mn = ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        for call in (lambda: ctx.chain_sample(LMIN, LMAX), lambda: ctx.chain_run(2, LMIN, LMAX), lambda: ctx.chain_rng_state(),
                     lambda: ctx.chain_rng_seek(3), lambda: ctx.chain_normals(0)):
            assert code_of(call) == EINVAL                                                # no seed
        assert "hmcmt_chain_seed" in str(pytest.raises(HmcmtError, ctx.chain_sample, LMIN, LMAX).value)
        ctx.chain_seed(SEED, 4)
        for lmin, lmax in ((0, 3), (-2, 3), (5, 4)):
            assert code_of(lambda: ctx.chain_sample(lmin, lmax)) == EINVAL
            assert code_of(lambda: ctx.chain_run(2, lmin, lmax)) == EINVAL
        assert code_of(lambda: ctx.chain_run(-1, LMIN, LMAX)) == EINVAL
        assert ctx.lib.hmcmt_chain_sample(ctx.h, LMIN, LMAX, None, None, None) == EINVAL
        assert ctx.lib.hmcmt_chain_run(ctx.h, 2, LMIN, LMAX, None, None, None, None) == EINVAL
        assert ctx.lib.hmcmt_chain_normals(ctx.h, 0, None, 0) == EINVAL
        assert ctx.chain_rng_state() == (SEED, 4, 0)                                      # (a refused call draws nothing)
        assert ctx.chain_run(0, LMIN, LMAX)[0] == [] and ctx.chain_rng_state() == (SEED, 4, 0)
        first = ctx.chain_normals(0)
        recs = []
        for k in range(1, 4):
            recs.append(ctx.chain_sample(1, 2)[0])
            assert ctx.chain_rng_state() == (SEED, 4, k) and recs[-1]["nsamples"] == k
        # a sample's L is draw t's: the trajectory's evaluations say which was taken (the first evaluates its start gradient too)
        Ls = [L.rng_draw(SEED, 4, t, 1, 2)[0] for t in range(3)]
        assert [r["nfevals"] for r in recs] == [Ls[0] + 1, Ls[1], Ls[2]]
        ctx.chain_rng_seek(0)
        assert ctx.chain_rng_state() == (SEED, 4, 0) and np.array_equal(ctx.chain_normals(0), first)
        assert not np.array_equal(ctx.chain_normals(1), first)
        ctx.chain_rng_seek(T_HIGH)
        assert ctx.chain_rng_state() == (SEED, 4, T_HIGH)
        # host-fed calls on the seeded chain do not move t
        ctx.chain_momentum(first)
        ctx.chain_step(1, 0.5)
        assert ctx.chain_rng_state() == (SEED, 4, T_HIGH)
        # a second seed restarts the counter; a begin forgets the seed
        ctx.chain_seed(SEED + 1, 0)
        assert ctx.chain_rng_state() == (SEED + 1, 0, 0) and not np.array_equal(ctx.chain_normals(0), first)
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        assert code_of(lambda: ctx.chain_sample(LMIN, LMAX)) == EINVAL and code_of(lambda: ctx.chain_rng_state()) == EINVAL
    finally:
        ctx.close()


def test_a_failed_sample_consumes_its_draw_and_leaves_the_chain():
    """the iteration-cap route of tests/test_gpu_chain.py: maxit = 2 is met by no solve on this mesh"""
    P = problem("tiny")
    ctx = context(P)
    try:
        begin(ctx, P, 5, burnin=1)
        for _ in range(3):
            rec, _, _ = ctx.chain_sample(1, 3)
        before = (ctx.chain_state()[0], ctx.chain_state()[2], ctx.chain_moments())
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)
        assert code_of(lambda: ctx.chain_sample(1, 3)) == ENOCONV
        assert ctx.chain_rng_state() == (SEED, 5, 4)                                      # t advanced by one
        recs, models, preds, rc = ctx.chain_run(3, 1, 3, check=False)
        assert rc == ENOCONV and recs == [] and len(models) == 0 and ctx.chain_rng_state() == (SEED, 5, 5)
        after = (ctx.chain_state()[0], ctx.chain_state()[2], ctx.chain_moments())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2][0] == after[2][0] == 2 and all(np.array_equal(a, b) for a, b in zip(before[2][1:], after[2][1:]))
        ctx.set_options(maxit=maxit)
        rec2, m2, _ = ctx.chain_sample(1, 3)
        assert rec2["nsamples"] == rec["nsamples"] + 1 == 4 and ctx.chain_rng_state() == (SEED, 5, 6)
        assert rec2["nfevals"] == L.rng_draw(SEED, 5, 5, 1, 3)[0] + 1                     # (draw 5's L; the start gradient is evaluated again)
    finally:
        ctx.close()


def test_a_run_that_fails_midway_reports_what_it_completed():
    """A cap on the solves' iterations between the easiest and the hardest sample of a run cuts the run short inside.  Which cap does
    depends on the solves, so the test looks for one: caps from 2 upwards, each on the chain begun again, until a run of NCUT samples
    completes; some cap on the way must complete some and not all of them (the samples' trajectories differ in length and in how far
    they move, and the cold first solves are taken out by one sample in front of the cap).  For that run: done records, each valid by
    the decision rule with the draws' own u, models and state in step, t advanced by done + 1, and the chain goes on."""
    NCUT, LCUT = 5, (1, 3)
    P = problem("tiny")
    ctx = context(P)
    try:
        maxit = ctx.opts.maxit
        found, seen = None, []
        for cap in range(2, 200):
            ctx.set_options(maxit=maxit)
            D, Mn = begin(ctx, P, 6, burnin=0)
            rec0, _, _ = ctx.chain_sample(LCUT[0], LCUT[1])
            ctx.set_options(maxit=cap)
            recs, models, preds, rc = ctx.chain_run(NCUT, LCUT[0], LCUT[1], check=False)
            seen.append(len(recs))
            if 0 < len(recs) < NCUT:
                found = (cap, recs, models, preds, rc, rec0)
                break
            if len(recs) == NCUT:
                break
        print(f"\n[a run cut short] completed samples by cap, from 2: {seen}")
        assert found is not None, seen
        cap, recs, models, preds, rc, rec0 = found
        done = len(recs)
        assert rc == ENOCONV and len(models) == len(preds) == done
        assert ctx.chain_rng_state() == (SEED, 6, 1 + done + 1)                           # (the failing sample consumed its draw)
        D, Mn = rec0["D"], rec0["M"]
        for k, rec in enumerate(recs):
            u = L.rng_draw(SEED, 6, 1 + k, LCUT[0], LCUT[1])[1]
            hdif = (D + Mn + rec["K0"]) - (rec["D1"] + rec["K1"] + rec["M1"])
            assert rec["hdif"] == hdif and rec["accepted"] == int(hdif > 0 or u < np.exp(hdif))
            assert rec["nsamples"] == k + 2 and all(np.isfinite(rec[key]) for key in REC_KEYS)
            D, Mn = rec["D"], rec["M"]
        m, _, pred = ctx.chain_state()
        assert np.array_equal(m, models[-1])
        count, mean, _ = ctx.chain_moments()
        assert count == done + 1
        ctx.set_options(maxit=maxit)
        more, _, _ = ctx.chain_run(2, LCUT[0], LCUT[1])
        assert [r["nsamples"] for r in more] == [done + 2, done + 3]
    finally:
        ctx.set_options(maxit=maxit)
        ctx.close()


# ---- 5. the sampler ----------------------------------------------------------------------------------------------------------------
def test_sampler_library_rng_keyword():
    """runHMCSampler(device_chain=True, library_rng=(7, 0)) twice: the same hmcstats, samples and data bit for bit; keep_samples=False:
    the same statistics and moments; stream 1: another chain; hmcstats.rng is the generator's state behind the run; hmstats' kinetic
    column is the records' K0, and its last entry the next draw's."""
    ns, burn = 8, 2
    hm, st, hd, moments, _ = run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 0))
    hm2, st2, hd2, *_ = run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 0))
    assert bits(hm) == bits(hm2) and bits(hd) == bits(hd2)
    for f in ("nAccept", "nReject", "acceptstats", "hmstats", "moments", "rng"):
        assert same_bits(getattr(st, f), getattr(st2, f)), f
    assert st.rng == (7, 0, ns) and st.moments[0] == ns - burn and hm.shape[1] == ns and 0 < st.nAccept
    assert np.all(np.isfinite(st.hmstats)) and np.all(st.hmstats[2] > 0)
    assert np.array_equal(st.hmstats[3], st.hmstats[0] + st.hmstats[1] + st.hmstats[2])
    hm3, st3, hd3, *_ = run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 0), keep_samples=False)
    assert hm3.shape[1] == 0 and hd3.shape[1] == 1
    for f in ("nAccept", "nReject", "acceptstats", "hmstats", "moments", "rng"):
        assert same_bits(getattr(st, f), getattr(st3, f)), f
    hm4, st4, *_ = run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 1))
    assert st4.rng == (7, 1, ns) and not np.array_equal(st4.hmstats[2], st.hmstats[2]) and not np.array_equal(hm4, hm)
    # verbose (blocks of chain_run) and adapt (single samples) give the chain of the one call
    hm5, st5, *_ = run("tiny", prior_of(20, burn), device_chain=True, library_rng=(7, 0), verbose=True)
    hm6, st6, *_ = run("tiny", prior_of(20, burn), device_chain=True, library_rng=(7, 0))
    assert bits(hm5) == bits(hm6) and same_bits(st5.hmstats, st6.hmstats) and bits(hm6[:, :ns]) == bits(hm)
    with pytest.raises(ValueError, match="library_rng needs device_chain=True"):
        run("tiny", prior_of(ns, burn), library_rng=(7, 0))
    with pytest.raises(ValueError, match="library_rng"):
        run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 1 << 32))
