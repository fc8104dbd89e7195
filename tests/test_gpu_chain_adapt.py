"""The chain's warm-up adaptation on the device (hmcmt_chain_set_dt, hmcmt_chain_set_mass_diag, hmcmt_chain_mass_diag,
hmcmt_chain_adapt_*; k_chain_adapt_mass) against tests/adapt_ref.py, a longdouble replay of the adaptation from what the chain itself
returned: at one partly filled workgroup (tiny, 96 cells) and a full one plus a partial one (the ragged problem, 390).  Forced and
drawn decisions, a bitwise replay of an adapted chain through the two setters, adaptation that changes nothing, the commit's
accumulators beside it, M = Wm, the state rules, the direction of the step size, and the sampler's adapt= keyword."""
import ctypes

import numpy as np
import pytest

from hmcmt2d_amd import sampler
from hmcmt2d_amd.lib import AdaptInfo, HipContext, HmcmtError, HMCMT_MASS_WM
from tests import adapt_ref as A
from tests.test_gpu_chain import DT, LTRAJ, RHO, fresh, prior_of, problem as chain_problem
from tests.test_gpu_chain_kernels import FORCE, HI, LO, REG, normals, problem

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
SEQ14 = "AARRRARAARRARA"
WINDOWS = dict(init_buffer=2, term_buffer=2, base_window=3)
REC_KEYS = ("accepted", "nfevals", "K0", "K1", "D1", "M1", "D", "M", "hdif", "nsamples", "nmoments")


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def rec_bits(recs):
    return [tuple(bits(np.float64(r[k])) for k in REC_KEYS) for r in recs]


def begin_accumulators(ctx, n):
    ctx.chain_hist_begin(np.arange(0, n, 3), 40, LO, HI)
    ctx.chain_data_moments_begin()
    ctx.chain_acov_begin(None, 3)
    ctx.chain_cov_begin(np.array([0, n // 2, n - 1]), 2)


def read_accumulators(ctx):
    return {"hist": ctx.chain_hist(), "dmom": ctx.chain_data_moments(raw=True), "acov": ctx.chain_acov(), "ess": ctx.chain_ess(),
            "cov": ctx.chain_cov(), "corr": (ctx.chain_corr(),)}


def drive(P, nsteps, seed, dt=None, seq=None, adapt=None, replay=None, burnin=0, accs=False, mass=None, before_first=None, invM=None):
    """A chain by hand on a context of its own.  seq[i] in "AR" forces step i's decision through chain_set_energy (alpha exactly 1 or
    0), anything else or no seq leaves it to the draw.  adapt: the keywords of chain_adapt_begin, begun behind chain_begin.  replay:
    an earlier result -- no adaptation, chain_set_dt with that chain's step size in front of every step and chain_set_mass_diag with
    its read-out mass behind the steps that closed a window.  Returns records, models, the info behind every step, the step size
    every step used, the masses read out behind a mass update (by steps completed), the moments and the accumulators' results.
    invM: the diagonal of the context's prior instead of the problem's."""
    if invM is None:
        ctx = P.context(mass)
    else:
        ctx = HipContext(P.mesh, P.data, P.inv, device_id=0)
    try:
        if invM is not None:
            ctx.set_prior(P.mref, P.inv.Wm, invM)
        rng = np.random.default_rng(seed)
        n = P.n
        dt0 = P.dt if dt is None else dt
        D, Mn = ctx.chain_begin(P.start, dt0, REG, LO, HI, burnin=burnin)
        if accs:
            begin_accumulators(ctx, n)
        if adapt is not None:
            ctx.chain_adapt_begin(**adapt)
        if before_first is not None:
            before_first(ctx)
        out = {"recs": [], "models": [], "infos": [], "dts": [], "masses": {}}
        done = 0
        for it in range(nsteps):
            if replay is not None and it in replay["masses"]:
                ctx.chain_set_mass_diag(replay["masses"][it])
            ctx.chain_momentum(normals(rng, n))
            if replay is not None:
                ctx.chain_set_dt(replay["dts"][it])
            out["dts"].append(ctx.chain_adapt_info()["dt"] if adapt is not None else (replay["dts"][it] if replay is not None else dt0))
            force = seq[it] if seq is not None and it < len(seq) else "-"
            if force in "AR":
                ctx.chain_set_energy(D + FORCE if force == "A" else D - FORCE, Mn)
            rec, m, _ = ctx.chain_step((1, 2)[it % 2], rng.random())
            if force in "AR":
                assert rec["accepted"] == int(force == "A")
            if rec["accepted"]:
                D, Mn = rec["D"], rec["M"]
            elif force == "R":
                ctx.chain_set_energy(D, Mn)
            out["recs"].append(rec); out["models"].append(m)
            if adapt is not None:
                info = ctx.chain_adapt_info()
                out["infos"].append(info)
                if info["windows_done"] > done:
                    done = info["windows_done"]
                    out["masses"][it + 1] = ctx.chain_mass_diag()
        out["moments"] = ctx.chain_moments()
        out["invM"] = ctx.chain_mass_diag()
        if accs:
            out["accs"] = read_accumulators(ctx)
        return out
    finally:
        ctx.close()


def check_against_reference(P, run, ref, label):
    """every step size and every mass of an adapted chain against the longdouble replay of its own records and samples"""
    worst_dt, worst_mass = 0.0, 0.0
    for it, (rec, m, info) in enumerate(zip(run["recs"], run["models"], run["infos"])):
        was_active = ref.active
        ref.step(rec["hdif"], m)
        if was_active:
            err, bound = abs(float(A.LD(np.log(info["dt"])) - np.log(ref.dt))), ref.bound()
            worst_dt = max(worst_dt, err / bound)
            assert err <= bound, (label, it, info["dt"], float(ref.dt), err, bound)
            assert info["step"] == it + 1 and info["active"] == int(ref.active)
        else:
            assert info["dt"] == run["infos"][it - 1]["dt"] and info["active"] == 0
    assert sorted(run["masses"]) == [s for s, *_ in ref.masses], (label, sorted(run["masses"]), ref.closed)
    for steps, mass, nw, mean, m2, w in ref.masses:
        got = run["masses"][steps]
        bound = A.mass_bound(mass, mean, m2, nw, w)
        err = np.abs(got - np.asarray(mass, dtype=np.float64))
        worst_mass = max(worst_mass, float((err / bound).max()))
        assert np.all(err <= bound), (label, steps, float((err / bound).max()))
        fixed = np.asarray(m2 == 0)
        assert np.all(got[fixed] == 1e-3 * 5.0 / (nw + 5.0)) and np.all(got > 0)
    print(f"\n[{label}] dt {[float('%.4g' % i['dt']) for i in run['infos']]}; alpha {[round(A.alpha_of(r['hdif']), 3) for r in run['recs']]}; "
          f"largest error over its bound: ln dt {worst_dt:.2g}, mass {worst_mass:.2g}")


# ---- the two setters -----------------------------------------------------------------------------------------------------------------
def test_set_dt_before_the_first_step_gives_the_chain_begun_with_it():
    P = problem("tiny")
    a = drive(P, 4, seed=71, dt=0.035)
    b = drive(P, 4, seed=71, dt=0.01, before_first=lambda ctx: ctx.chain_set_dt(0.035))
    assert rec_bits(a["recs"]) == rec_bits(b["recs"]) and bits(np.array(a["models"])) == bits(np.array(b["models"]))
    c = drive(P, 4, seed=71, dt=0.01)
    assert rec_bits(a["recs"]) != rec_bits(c["recs"])          # (the step size does matter to these records)


def test_set_mass_diag_before_the_first_momentum_gives_the_chain_of_that_prior():
    P = problem("ragged")
    invM2 = np.random.default_rng(5).uniform(0.1, 3.0, P.n)
    seen = {}

    def swap(ctx):
        assert np.array_equal(ctx.chain_mass_diag(), P.invM)
        ctx.chain_set_mass_diag(invM2)
        seen["mass"] = ctx.chain_mass_diag()
        import torch
        d = torch.zeros(P.n, dtype=torch.float64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        assert ctx.chain_mass_diag(d.data_ptr()) is None
        seen["device"] = d.cpu().numpy()

    b = drive(P, 4, seed=72, before_first=swap)
    assert np.array_equal(seen["mass"], invM2) and np.array_equal(seen["device"], invM2) and np.array_equal(b["invM"], invM2)
    a = drive(P, 4, seed=72, invM=invM2)
    assert rec_bits(a["recs"]) == rec_bits(b["recs"]) and bits(np.array(a["models"])) == bits(np.array(b["models"]))


def test_set_mass_diag_drops_a_momentum_and_checks_its_argument():
    P = problem("tiny")
    ctx = P.context()
    try:
        rng = np.random.default_rng(73)
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        ctx.chain_momentum(normals(rng, P.n))
        ctx.chain_set_dt(0.015)                                # (keeps the momentum)
        ctx.chain_set_mass_diag(2.0 * P.invM)
        assert code_of(lambda: ctx.chain_step(1, 0.5)) == EINVAL
        assert "no momentum" in ctx.lib.hmcmt_last_error(ctx.h).decode()
        ctx.chain_momentum(normals(rng, P.n))
        rec, _, _ = ctx.chain_step(1, 0.5)
        assert rec["nsamples"] == 1
        for bad in (0.0, -1.0, np.inf, np.nan):
            v = P.invM.copy(); v[P.n - 1] = bad
            assert code_of(lambda: ctx.chain_set_mass_diag(v)) == EINVAL
            assert code_of(lambda: ctx.chain_set_dt(bad)) == EINVAL
        assert np.array_equal(ctx.chain_mass_diag(), 2.0 * P.invM)
        ctx.chain_end()
        assert code_of(lambda: ctx.chain_set_dt(0.01)) == EINVAL and code_of(lambda: ctx.chain_mass_diag()) == EINVAL
        assert code_of(lambda: ctx.chain_set_mass_diag(P.invM)) == EINVAL
    finally:
        ctx.close()


# ---- forced decisions, the replay, the accumulators -----------------------------------------------------------------------------------
BURNIN, NSTEPS = 14, 18


@pytest.fixture(scope="module")
def forced():
    """A A R R R A R A A R R A R A over a warm-up of 14 steps (buffers 2 / 2, base 3: windows close behind steps 5 and 12), then four
    steps more, the commit's accumulators on behind a burn-in of 14 (shared, left unchanged)"""
    return drive(problem("tiny"), NSTEPS, seed=74, seq=SEQ14, adapt=dict(nwarmup=14, **WINDOWS), burnin=BURNIN, accs=True)


def test_forced_decisions_against_the_reference(forced):
    P = problem("tiny")
    ref = A.Warmup(P.dt, 14, True, 2, 2, 3)
    check_against_reference(P, forced, ref, "forced decisions, tiny")
    assert [A.alpha_of(r["hdif"]) for r in forced["recs"][:14]] == [float(c == "A") for c in SEQ14]
    assert sorted(forced["masses"]) == [5, 12] and ref.closed == [(5, 3), (12, 7)]
    infos = forced["infos"]
    assert [i["windows_done"] for i in infos[:14]] == [0] * 4 + [1] * 7 + [2] * 3
    assert [i["next_window_end"] for i in infos[:14]] == [4] * 4 + [11] * 7 + [-1] * 3
    assert [i["window_count"] for i in infos[:12]] == [0, 0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 0]
    assert infos[12]["active"] == 1 and infos[13]["active"] == 0 and infos[13]["step"] == 14
    assert infos[13]["dt"] == infos[13]["dt_bar"]              # dt = exp(x_bar) at the end
    assert forced["dts"][14] == infos[13]["dt"] and all(i["dt"] == infos[13]["dt"] and i["step"] == 14 for i in infos[14:])
    assert infos[13]["alpha_sum"] == SEQ14.count("A") and infos[13]["alpha_last"] == 1.0
    assert np.array_equal(forced["invM"], forced["masses"][12])  # the adapted mass stays the context's


def test_replay_through_the_setters_is_bitwise_the_adapted_chain(forced):
    """A second context without adaptation: chain_set_dt with the first chain's value in front of every step, chain_set_mass_diag with
    its read-out mass behind steps 5 and 12, the same normals and uniforms.  Records, samples, moments and every accumulator's
    result are the adapted chain's, bit for bit; the accumulators count the samples behind the burn-in."""
    replay = drive(problem("tiny"), NSTEPS, seed=74, seq=SEQ14, replay=forced, burnin=BURNIN, accs=True)
    assert rec_bits(replay["recs"]) == rec_bits(forced["recs"])
    assert bits(np.array(replay["models"])) == bits(np.array(forced["models"]))
    assert replay["moments"][0] == forced["moments"][0] == NSTEPS - BURNIN
    assert all(bits(a) == bits(b) for a, b in zip(replay["moments"][1:], forced["moments"][1:]))
    for key, got in forced["accs"].items():
        if key not in ("ess", "corr"):
            assert got[0] == NSTEPS - BURNIN, key
        assert all(bits(a) == bits(b) for a, b in zip(got, replay["accs"][key])), key


# ---- drawn decisions -----------------------------------------------------------------------------------------------------------------
# (chosen on the device: the drawn alphas of the 16 warm-up steps hold 0.79, 0.7, 0.026, 0.828, 0.575 on tiny and 0.881, 0.667, 0.09 on
# the ragged problem, whose acceptance is nearly all or nothing at the step sizes the dual averaging visits)
NATURAL = {"tiny": dict(dt=0.02, seed=81), "ragged": dict(dt=0.02, seed=91)}


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_drawn_decisions_against_the_reference(name):
    """delta = 0.65 over 16 warm-up steps (windows close behind steps 5 and 14), two steps more: the reference reproduces every step
    size from the records' hdif and every mass from the returned samples; at least three steps had 0 < alpha < 1.  Then the replay."""
    P = problem(name)
    cfg = NATURAL[name]
    run = drive(P, 18, seed=cfg["seed"], dt=cfg["dt"], adapt=dict(nwarmup=16, delta=0.65, **WINDOWS))
    ref = A.Warmup(cfg["dt"], 16, True, 2, 2, 3, delta=0.65)
    check_against_reference(P, run, ref, f"drawn decisions, {name}")
    alphas = [A.alpha_of(r["hdif"]) for r in run["recs"][:16]]
    assert sum(0.0 < a < 1.0 for a in alphas) >= 3, alphas
    assert sorted(run["masses"]) == [5, 14] and not ref.active and run["infos"][15]["active"] == 0
    replay = drive(P, 18, seed=cfg["seed"], dt=cfg["dt"], replay=run)
    assert rec_bits(replay["recs"]) == rec_bits(run["recs"]) and bits(np.array(replay["models"])) == bits(np.array(run["models"]))
    assert bits(replay["invM"]) == bits(run["invM"])


# ---- off means off -------------------------------------------------------------------------------------------------------------------
def test_an_adaptation_that_changes_nothing_leaves_every_bit():
    """Step size only with dt_min = dt_max = dt, and an adaptation begun and ended before any step: every record, sample, moment and
    accumulator bit is that of a chain without adaptation."""
    P = problem("ragged")
    plain = drive(P, 7, seed=83, burnin=2, accs=True)
    clipped = drive(P, 7, seed=83, burnin=2, accs=True, adapt=dict(nwarmup=5, adapt_mass=0, dt_min=P.dt, dt_max=P.dt))

    def begin_and_end(ctx):
        ctx.chain_adapt_begin(nwarmup=7, **WINDOWS)
        ctx.chain_adapt_end()
        info = ctx.chain_adapt_info()
        assert info["active"] == 0 and info["step"] == 0 and info["dt"] == P.dt == info["dt_bar"]
        ctx.chain_set_dt(P.dt)                                 # (allowed again)

    ended = drive(P, 7, seed=83, burnin=2, accs=True, before_first=begin_and_end)
    assert [i["dt"] for i in clipped["infos"]] == [P.dt] * 7 and clipped["infos"][4]["active"] == 0
    assert clipped["infos"][3]["s_bar"] != 0.0                 # (the dual averaging did run)
    for other in (clipped, ended):
        assert rec_bits(other["recs"]) == rec_bits(plain["recs"]) and bits(np.array(other["models"])) == bits(np.array(plain["models"]))
        assert other["moments"][0] == plain["moments"][0] == 5
        assert all(bits(a) == bits(b) for a, b in zip(other["moments"][1:], plain["moments"][1:]))
        assert bits(other["invM"]) == bits(plain["invM"]) == bits(P.invM)
        for key, got in plain["accs"].items():
            assert all(bits(a) == bits(b) for a, b in zip(got, other["accs"][key])), key


# ---- M = Wm --------------------------------------------------------------------------------------------------------------------------
def test_step_size_only_with_the_wm_mass():
    P = problem("ragged")

    def refused(ctx):
        before = ctx.chain_adapt_info()
        assert code_of(lambda: ctx.chain_adapt_begin(nwarmup=8, adapt_mass=1, **WINDOWS)) == EINVAL
        assert code_of(lambda: ctx.chain_set_mass_diag(P.invM)) == EINVAL
        assert ctx.chain_adapt_info() == before                # (the refused begin left the running one alone)

    run = drive(P, 9, seed=84, mass="wm", adapt=dict(nwarmup=8, adapt_mass=0, delta=0.65), before_first=refused)
    check_against_reference(P, run, A.Warmup(P.dt, 8, False, delta=0.65), "step size only, M = Wm, ragged")
    assert run["masses"] == {} and run["infos"][7]["active"] == 0 and run["infos"][7]["windows_done"] == 0


# ---- state rules ---------------------------------------------------------------------------------------------------------------------
BAD_OPTIONS = [dict(nwarmup=0), dict(nwarmup=-3), dict(nwarmup=7, **WINDOWS, adapt_mass=1) | dict(base_window=4),
               dict(nwarmup=14, init_buffer=-1, term_buffer=2, base_window=3), dict(nwarmup=14, init_buffer=2, term_buffer=-1, base_window=3),
               dict(nwarmup=14, init_buffer=2, term_buffer=2, base_window=0), dict(nwarmup=14, **WINDOWS, delta=0.0),
               dict(nwarmup=14, **WINDOWS, delta=1.0), dict(nwarmup=14, **WINDOWS, gamma=0.0), dict(nwarmup=14, **WINDOWS, t0=0.0),
               dict(nwarmup=14, **WINDOWS, t0=-1.0), dict(nwarmup=14, **WINDOWS, kappa=0.5), dict(nwarmup=14, **WINDOWS, kappa=1.01),
               dict(nwarmup=14, **WINDOWS, dt_min=0.2, dt_max=0.1), dict(nwarmup=14, **WINDOWS, delta=np.nan),
               dict(nwarmup=14, **WINDOWS, gamma=np.inf), dict(nwarmup=14, **WINDOWS, dt_max=np.inf), dict(nwarmup=14, **WINDOWS, dt_min=np.nan),
               dict(nwarmup=100)]                              # (the default buffers 75 + 50 + 25 do not fit)


def info_bytes(ctx):
    info = AdaptInfo()
    ctx._check(ctx.lib.hmcmt_chain_adapt_info(ctx.h, ctypes.byref(info)))
    return bytes(info)


def test_state_rules_of_the_adaptation():
    P = problem("tiny")
    ctx = P.context()
    try:
        rng = np.random.default_rng(85)
        assert code_of(lambda: ctx.chain_adapt_begin(nwarmup=14, **WINDOWS)) == EINVAL       # no chain
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        assert ctx.lib.hmcmt_chain_adapt_begin(ctx.h, None) == EINVAL                        # the defaults leave nwarmup open
        assert code_of(lambda: ctx.chain_adapt_info()) == EINVAL and code_of(lambda: ctx.chain_adapt_end()) == EINVAL
        for bad in BAD_OPTIONS:
            assert code_of(lambda: ctx.chain_adapt_begin(**bad)) == EINVAL, bad
        assert code_of(lambda: ctx.chain_adapt_info()) == EINVAL                             # a refused begin begins nothing
        ctx.chain_adapt_begin(nwarmup=7, **WINDOWS)                                          # 2 + 3 + 2: fits exactly
        ctx.chain_adapt_begin(nwarmup=14, kappa=1.0, dt_min=1e-4, **WINDOWS)                 # a second begin replaces the first
        assert ctx.chain_adapt_info()["nwarmup"] == 14
        assert code_of(lambda: ctx.chain_set_dt(0.01)) == EINVAL                             # while it is active
        assert code_of(lambda: ctx.chain_set_mass_diag(P.invM)) == EINVAL
        ctx.chain_adapt_begin(nwarmup=14, adapt_mass=0)
        ctx.chain_set_mass_diag(P.invM)                                                      # step size only: the mass is the caller's
        ctx.chain_adapt_begin(nwarmup=14, **WINDOWS)
        # between hmcmt_grad_device_async and hmcmt_wait
        import torch
        dev = torch.device("cuda", 0)
        d_m = torch.tensor(P.start, dtype=torch.float64, device=dev)
        d_pred, d_mis, d_g = (torch.zeros(k, dtype=torch.float64, device=dev) for k in (2 * ctx.nData, 1, P.n))
        torch.cuda.synchronize()
        ctx.grad_device_async(d_m.data_ptr(), d_pred.data_ptr(), d_mis.data_ptr(), d_g.data_ptr())
        codes = [code_of(lambda: ctx.chain_adapt_begin(nwarmup=14, **WINDOWS)), code_of(lambda: ctx.chain_adapt_info()),
                 code_of(lambda: ctx.chain_adapt_end()), code_of(lambda: ctx.chain_set_dt(0.01)), code_of(lambda: ctx.chain_mass_diag())]
        ctx.wait()
        assert codes == [EINVAL] * 5
        # a trajectory that fails leaves the adaptation where it was, byte for byte
        for _ in range(3):
            ctx.chain_momentum(normals(rng, P.n))
            ctx.chain_step(LTRAJ, rng.random())
        before, mass_before = info_bytes(ctx), ctx.chain_mass_diag()
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)                               # an iteration cap no solve on this mesh meets
        ctx.chain_momentum(normals(rng, P.n))
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == ENOCONV
        assert info_bytes(ctx) == before and np.array_equal(ctx.chain_mass_diag(), mass_before)
        ctx.set_options(maxit=maxit)
        ctx.chain_momentum(normals(rng, P.n))
        ctx.chain_step(LTRAJ, 0.5)
        info = ctx.chain_adapt_info()
        assert info["step"] == 4 and info["window_count"] == 2 and info_bytes(ctx) != before
        # hmcmt_chain_begin and hmcmt_set_prior end it
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        assert code_of(lambda: ctx.chain_adapt_info()) == EINVAL
        ctx.chain_set_dt(0.01)
        ctx.chain_adapt_begin(nwarmup=14, **WINDOWS)
        assert ctx.chain_adapt_info()["dt"] == 0.01
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
        assert code_of(lambda: ctx.chain_adapt_info()) == EINVAL
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        assert code_of(lambda: ctx.chain_adapt_info()) == EINVAL
        ctx.chain_adapt_begin(nwarmup=14, **WINDOWS)
        ctx.set_mass(HMCMT_MASS_WM)
        assert code_of(lambda: ctx.chain_adapt_info()) == EINVAL
    finally:
        ctx.close()


# ---- the direction -------------------------------------------------------------------------------------------------------------------
def test_the_step_size_moves_towards_the_target_from_either_side():
    """40 warm-up steps (step size only) with one seed on tiny, from 8 times and from an eighth of the step size of
    tests/test_gpu_chain.py: the final step size lies below and above its start.  Only the direction is asserted."""
    final = {}
    for key, dt0 in (("down", 8 * DT), ("up", DT / 8)):
        ctx, inv, _ = fresh()
        try:
            rng = np.random.default_rng(86)
            n = ctx.nAC
            ctx.chain_begin(np.full(n, np.log(1.0 / RHO["tiny"])), dt0, REG, LO, HI)
            ctx.chain_adapt_begin(nwarmup=40, adapt_mass=0)
            for _ in range(40):
                ctx.chain_momentum(rng.standard_normal(n))
                ctx.chain_step(LTRAJ, rng.random(), outputs=False)
            info = ctx.chain_adapt_info()
            assert info["active"] == 0 and info["step"] == 40
            final[key] = (dt0, info["dt"], info["alpha_sum"] / 40)
        finally:
            ctx.close()
    print(f"\n[direction] (start, final dt, mean alpha): {final}")
    assert final["down"][1] < final["down"][0] and final["up"][1] > final["up"][0]


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def test_sampler_adapt_keyword():
    """runHMCSampler(device_chain=True, adapt={...}): the reference reproduces the dt trace from hmcstats.adapt's alpha and the returned
    samples, and the mass from the samples; hmcprior.dt is not modified; invM= starts a chain with that diagonal."""
    mesh, data, inv, _ = chain_problem("tiny")
    prior = prior_of(18, 14)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        hm, st, hd = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(21), rhoref=RHO["tiny"], ctx=ctx, device_chain=True,
                                           adapt=dict(delta=0.65, **WINDOWS))
        mass = ctx.chain_mass_diag()
    finally:
        ctx.close()
    ad = st.adapt
    assert prior.dt == DT and ad["nwarmup"] == 14 and ad["dt"].shape == ad["alpha"].shape == (18,) and ad["dt"][0] == DT
    assert ad["windows"] == [(5, 3), (12, 7)] and np.array_equal(ad["invM"], mass) and st.moments[0] == 4
    ref = A.Warmup(DT, 14, True, 2, 2, 3, delta=0.65)
    for it in range(18):
        assert abs(float(A.LD(np.log(ad["dt"][it])) - np.log(ref.dt))) <= ref.bound(), it
        ref.step(None, hm[:, it], alpha=ad["alpha"][it])
    assert abs(float(A.LD(np.log(ad["dt_final"])) - np.log(ref.dt))) <= ref.bound() and np.all(ad["dt"][14:] == ad["dt_final"])
    steps, m_ref, nw, mean, m2, w = ref.masses[-1]
    assert steps == 12 and np.all(np.abs(mass - np.asarray(m_ref, dtype=np.float64)) <= A.mass_bound(m_ref, mean, m2, nw, w))
    # invM=: the chain starts with that diagonal
    mesh, data, inv, _ = chain_problem("tiny")
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        _, st2, _ = sampler.runHMCSampler(mesh, data, inv, prior_of(2, 0), np.random.default_rng(21), rhoref=RHO["tiny"], ctx=ctx,
                                          device_chain=True, invM=mass)
        assert np.array_equal(ctx.chain_mass_diag(), mass) and st2.adapt is None
    finally:
        ctx.close()
