"""The kernels of the device-resident HMC chain (kernels_chain.h, k_lf_mnorm behind hmcmt_chain_begin) and their launches in
host_chain.h against tests/chain_ref.py, a longdouble evaluation of what the chain itself returns: at one partly filled workgroup
(tiny, 96 parameters), a full one plus a partial one (the ragged problem, 390) and a second grid-stride pass (cfg3, 20000 = 16384 +
14 full workgroups + 32 threads); with a non-unit mass, a start model off the reference model, and accept / reject sequences that
the test decides through chain_set_energy; then M = Wm, a begin over a live chain, every other call of the context between two
steps, and a trajectory of the chain that clamps and reflects."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from hmcmt2d_amd import sampler
from hmcmt2d_amd.lib import HipContext, HMCMT_MASS_WM, HMCMT_MASS_OP_INV
from hmcmt2d_amd.structs import HMCParameter, HMCPrior
from tests import chain_ref as R
from tests.helpers import make_problem, ragged_problem, relmax
from tests.golden.make_chain import chain_prior_of, start_model_of
from tests.test_gpu_chain import hm_err
from tests.test_gpu_mass import banded_factor

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
LO, HI = float(np.log(1e-4)), 0.0
REG = 1.0
RHO = {"tiny": 122.0, "ragged": 90.0}          # the homogeneous start models of tests/test_gpu_chain.py
FORCE = 1e12                                   # added to / taken from the chain's misfit: hdif > 0, or exp(hdif) == 0
SEQ = "AARRRARA"
BURNIN = 2


class Problem:
    """A problem with what the chain needs around it: a start model, a reference model shifted off it by a smooth, non-constant
    field (M0 != 0), a non-unit diagonal mass"""

    def __init__(self, name):
        self.name = name
        if name == "ragged":
            self.mesh, self.data, self.inv, self.m_other = ragged_problem(23, 17, 3, 3, 3, 4)
        else:
            self.mesh, self.data, self.inv, self.m_other = make_problem(name)
        inv = self.inv
        self.n = n = len(inv.strModel)
        if name == "cfg3":
            self.dt = chain_prior_of("cfg3").dt
            self.start = start_model_of("cfg3", self.mesh, inv)
        else:
            self.dt = 0.02
            self.start = np.full(n, np.log(1.0 / RHO[name]))
        ny, nz = self.mesh.gridSize
        ky, kz = inv.activeIdx % ny, inv.activeIdx // ny
        self.mref = self.start - (0.2 * np.sin(2 * np.pi * ky / ny) * np.cos(np.pi * kz / nz) + 0.1 * kz / nz)
        self.invM = np.random.default_rng(n).uniform(0.25, 4.0, n)
        self.rownnz = int(np.diff(inv.Wm.tocsr().indptr).max())

    def context(self, mass=None):
        ctx = HipContext(self.mesh, self.data, self.inv, device_id=0)
        try:
            ctx.set_prior(self.mref, self.inv.Wm, self.invM)
            if mass == "wm":
                ctx.set_mass(HMCMT_MASS_WM)
        except Exception:
            ctx.close()
            raise
        return ctx


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]


def normals(rng, n):
    """z = 2 N(0, 1) with the clip's cases planted: beyond it on either side, exactly on it, a negative zero"""
    z = 2.0 * rng.standard_normal(n)
    z[0], z[-1], z[1], z[2] = 7.5, -3.25, 2.5, -0.0
    return z


class Maxima:
    """the largest value seen of each checked quantity, in units of its bound"""

    def __init__(self):
        self.v = {}

    def check(self, key, err, bound, what=""):
        err, bound = np.asarray(err, dtype=float), np.asarray(bound, dtype=float)
        ok = err <= bound
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
        self.v[key] = max(self.v.get(key, 0.0), ratio)
        assert np.all(ok), f"{key} {what}: {ratio:.3g} of its bound"

    def __str__(self):
        return ", ".join(f"{k} {v:.2g}" for k, v in self.v.items())


def check_energy(mx, P, ctx, key, D, Mn, pred, m):
    """a data misfit and a prior term of the chain against the reference at the chain's own pred and model"""
    Dref = R.misfit(pred, P.inv)
    Mref, S = R.mnorm(m, P.mref, P.inv.Wm, REG)
    # D: positive terms; serial adds per thread of k_src (128 threads share nData), the wave and LDS tree, the residual's own roundings
    mx.check("D" + key, abs(D - Dref), (np.ceil(ctx.nData / 128) + 24) * 2.0 ** -52 * Dref)
    # M: the row's adds, the partial sums' tree and final loop, the differences' and products' roundings, against the absolute-value sum
    mx.check("M" + key, abs(Mn - Mref), (P.rownnz + 96) * 2.0 ** -53 * S)
    assert Dref > 0 and Mref > 0


def check_moments(mx, ctx, committed, count, device=False):
    got = ctx.chain_moments()
    assert got[0] == count == len(committed)
    cr, mean_ref, m2_ref = R.moments(np.array(committed).T)
    bmean, bvar = R.moments_bounds(mean_ref, m2_ref, cr)
    moved = m2_ref > 0
    assert moved.any()
    mx.check("mean", np.abs(got[1] - mean_ref).max(), bmean)
    mx.check("var", np.abs(got[2] / count - m2_ref / cr)[moved], bvar[moved])
    assert np.all(got[2][~moved] == 0.0)
    if device:
        import torch
        d = torch.zeros(2, ctx.nAC, dtype=torch.float64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        assert ctx.chain_moments_device(d[0].data_ptr(), d[1].data_ptr()) == count
        assert np.array_equal(d.cpu().numpy(), np.stack(got[1:]))
    return got


def run_chain(P, ctx, seq, seed, start=None, burnin=BURNIN, mass=None, full=True, between=None, moments_at=(), Ls=(1, 2)):
    """A chain by hand on ctx: seq[i] in "AR" forces step i's decision through chain_set_energy, "-" leaves it to the draw.  Every
    step is held to the reference (full=False: the decision rule only).  Returns (records, models, kinetic energies, maxima)."""
    rng = np.random.default_rng(seed)
    n, inv, invM = P.n, P.inv, P.invM
    mx = Maxima()
    start = P.start if start is None else start
    D, Mn = ctx.chain_begin(start, P.dt, REG, LO, HI, burnin=burnin)
    m0, _, pred0 = ctx.chain_state()
    assert np.array_equal(m0, start)
    if full:
        check_energy(mx, P, ctx, "0", D, Mn, pred0, start)
    if mass == "wm":
        _, lmul = banded_factor(inv.Wm)
        lu = spla.splu(sp.csc_matrix(inv.Wm))
    recs, models, ks, committed = [], [], [], []
    for it, force in enumerate(seq):
        z = normals(rng, n)
        K = ctx.chain_momentum(z)
        m_before, p, pred_before = ctx.chain_state()
        if full and mass == "wm":
            # the bars of test_mass_apply_against_scipy: L clip(z) to 1e-13, 0.5 p' Wm^-1 p to 1e-10
            mx.check("p", relmax(p, lmul(np.clip(z, -2.5, 2.5))), 1e-13)
            mx.check("K", abs(K - 0.5 * float(p @ lu.solve(p))), 1e-10 * K)
        elif full:
            p_ref, K_ref = R.momentum(z, invM)
            assert np.abs(z).max() > 2.5 and p_ref[2] == 0.0
            mx.check("p", np.abs(p - p_ref), 4 * EPS * np.abs(p_ref), "per element")      # two correctly rounded operations
            mx.check("K", abs(K - K_ref), 1e-14 * K_ref)               # positive terms, some 80 roundings: 80 * 2^-53 = 8.9e-15
        if between is not None:
            between(it)
        D_set = D + FORCE if force == "A" else D - FORCE if force == "R" else D
        if force != "-":
            ctx.chain_set_energy(D_set, Mn)
        u = rng.random()
        rec, m_out, pred_out = ctx.chain_step(Ls[it % len(Ls)], u)
        m_after, p_after, pred_after = ctx.chain_state()
        # the decision, from the record's own fields and the energies the step started from
        hdif, accepted = R.decision(D_set, Mn, rec["K0"], rec["D1"], rec["K1"], rec["M1"], u)
        assert rec["hdif"] == hdif and rec["accepted"] == int(accepted), (it, rec, hdif, accepted)
        if force != "-":
            assert accepted == (force == "A"), (it, rec)
        assert rec["K0"] == K                                  # (host_chain.h: the same partial sums in the same order)
        assert rec["nsamples"] == it + 1 and rec["nmoments"] == max(0, it + 1 - burnin)
        assert np.array_equal(m_out, m_after) and np.array_equal(pred_out, pred_after)
        if accepted:
            assert rec["D"] == rec["D1"] and rec["M"] == rec["M1"]
            assert not np.array_equal(m_out, m_before)
            D, Mn = rec["D"], rec["M"]
        else:
            assert np.array_equal(m_out, m_before) and np.array_equal(pred_out, pred_before)
            assert rec["D"] == D_set and rec["M"] == Mn
            if force == "R":
                ctx.chain_set_energy(D, Mn)                    # (an accepted step resets them itself)
        if full:
            # chain_state's momentum is the trajectory's end momentum whether or not the step was accepted
            if mass == "wm":
                mx.check("K1", abs(rec["K1"] - 0.5 * float(p_after @ lu.solve(p_after))), 1e-10 * rec["K1"])
            else:
                mx.check("K1", abs(rec["K1"] - R.kinetic(p_after, invM=invM)), 1e-14 * rec["K1"])
            if accepted:
                check_energy(mx, P, ctx, "1", rec["D1"], rec["M1"], pred_out, m_out)
        recs.append(rec); models.append(m_out); ks.append(K)
        if it >= burnin:
            committed.append(m_out)
        if it + 1 in moments_at:
            check_moments(mx, ctx, committed, it + 1 - burnin, device=(it + 1 == len(seq)))
    return recs, models, ks, mx, committed


def forced_run(P, ctx, mass=None):
    """A A R R R A R A behind a burn-in of 2, every check after every step, the moments after steps 5, 6 and 8"""
    seen = {}

    def between(it):
        if it == 5:                                            # after A A R R R: three times the model of step 2
            count, mean, m2 = ctx.chain_moments()
            seen["m"] = ctx.chain_state()[0]
            assert count == 3 and np.array_equal(mean, seen["m"]) and np.all(m2 == 0.0)

    recs, models, ks, mx, committed = run_chain(P, ctx, SEQ, seed=31, mass=mass, between=between, moments_at=(6, 8))
    assert np.array_equal(seen["m"], models[1]) and np.array_equal(models[4], models[1])
    assert len(committed) == 6 and [r["nmoments"] for r in recs] == [0, 0, 1, 2, 3, 4, 5, 6]
    assert [r["accepted"] for r in recs] == [int(c == "A") for c in SEQ]
    print(f"\n[forced chain, {P.name}{', M = Wm' if mass else ''}] nAC {P.n}, nData {ctx.nData}; largest error over its bound: {mx}")
    return recs


def unforced_run(P, ctx):
    recs, _, _, _, _ = run_chain(P, ctx, "-" * 6, seed=32, full=False)
    print(f"\n[unforced chain, {P.name}] decisions {[r['accepted'] for r in recs]}, hdif {[round(r['hdif'], 3) for r in recs]}")


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_forced_chain_against_the_reference(name):
    P = problem(name)
    ctx = P.context()
    try:
        forced_run(P, ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_decision_rule_with_drawn_decisions(name):
    P = problem(name)
    ctx = P.context()
    try:
        unforced_run(P, ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_forced_chain_with_the_wm_mass(name):
    """tiny: the mass separates; the ragged problem: PCG"""
    P = problem(name)
    ctx = P.context(mass="wm")
    try:
        assert ctx.mass_info()["separable"] == (name == "tiny")
        forced_run(P, ctx, mass="wm")
    finally:
        ctx.close()


def test_begin_over_a_live_chain():
    """hmcmt_chain_begin on a context that holds a chain keeps the buffers and zeroes them: the counts restart, no mean or m2 of the
    first chain survives, and the records are those of a fresh context with the same inputs to 1e-6 (the solves start elsewhere)."""
    P = problem("tiny")
    start2 = P.start + 0.05 * np.cos(np.arange(P.n) / 5.0)
    ctx = P.context()
    try:
        first, *_ = run_chain(P, ctx, "AARA", seed=41, burnin=1)
        assert first[-1]["nsamples"] == 4 and first[-1]["nmoments"] == 3 and ctx.chain_moments()[0] == 3
        recs, models, ks, mx, committed = run_chain(P, ctx, "ARAA", seed=42, start=start2, burnin=2, moments_at=(4,))
        moments = ctx.chain_moments()
    finally:
        ctx.close()
    assert [r["nsamples"] for r in recs] == [1, 2, 3, 4] and [r["nmoments"] for r in recs] == [0, 0, 1, 2]
    ctx = P.context()
    try:
        ref, models_ref, ks_ref, _, _ = run_chain(P, ctx, "ARAA", seed=42, start=start2, burnin=2, moments_at=(4,))
        moments_ref = ctx.chain_moments()
    finally:
        ctx.close()
    assert ks == ks_ref                                        # (the momentum draw depends on z and the mass alone)
    errs = {k: hm_err(np.array([r[k] for r in recs]), np.array([r[k] for r in ref])) for k in ("K1", "D1", "M1", "D", "M")}
    em = max(relmax(a, b) for a, b in zip(models, models_ref))
    print(f"\n[begin over a live chain] moments over their bounds: {mx}; against a fresh context: {errs}, models {em:.2e}")
    assert max(errs.values()) < 1e-6 and em < 1e-7
    assert moments[0] == moments_ref[0] == 2 and relmax(moments[1], moments_ref[1]) < 1e-7


# ---- every other call of the context between two steps -----------------------------------------------------------------------------
LB = 2                                         # trajectory length of these chains
CALLS = ["forward", "leapfrog", "jacobian", "linearize_products", "jvp_block", "sensitivity", "mass_apply", "set_options",
         "chain_state", "chain_moments"]
EVALUATES = {"forward": True, "leapfrog": True, "linearize_products": True, "set_options": True, "chain_state": False, "chain_moments": False}
PLACE = {"after_accept": "AAAA", "after_reject": "ARAA"}       # the call comes behind step 2: nextStart 1 / 2


def call_between(ctx, P, which):
    m, n = P.m_other, P.n
    rng = np.random.default_rng(5)
    if which == "forward":
        ctx.forward(m)
    elif which == "leapfrog":
        ctx.leapfrog(m, rng.standard_normal(n), P.dt, 1, REG, LO, HI)
    elif which == "jacobian":
        ctx.jacobian(m, rows=(1, 4))
    elif which == "linearize_products":
        ctx.linearize(m)
        ctx.jvp(rng.standard_normal(n)); ctx.jtvp(rng.standard_normal(ctx.nData) + 0j); ctx.gn_hessvec(rng.standard_normal(n))
    elif which == "jvp_block":
        ctx.linearize(m)                                       # (a step ends the linearisation: the block needs its own)
        ctx.jvp_block(rng.standard_normal((2, n)))
    elif which == "sensitivity":
        ctx.sensitivity(m)
    elif which == "mass_apply":
        ctx.mass_apply(HMCMT_MASS_OP_INV, rng.standard_normal(n))
    elif which == "set_options":
        ctx.set_options(maxit=ctx.opts.maxit, tol=ctx.opts.tol)
    elif which == "chain_state":
        ctx.chain_state()
    elif which == "chain_moments":
        ctx.chain_moments()
    else:
        raise KeyError(which)


def between_run(place, which=None):
    P = problem("tiny")
    ctx = P.context()
    try:
        def between(it):
            if it == 2 and which is not None:
                call_between(ctx, P, which)
        recs, models, ks, _, _ = run_chain(P, ctx, PLACE[place], seed=51, burnin=1, full=False, between=between, Ls=(LB,))
    finally:
        ctx.close()
    return recs, models, ks


@pytest.fixture(scope="module")
def undisturbed():
    """the two chains without a call in between (shared, left unchanged)"""
    return {place: between_run(place) for place in PLACE}


@pytest.mark.parametrize("which", CALLS)
@pytest.mark.parametrize("place", list(PLACE))
def test_a_call_between_two_steps(place, which, undisturbed):
    """A step whose start gradient the last decision left on the device (the proposal's after an acceptance, the start's after a
    rejection) evaluates it again after any evaluating call on the context, and gives the undisturbed chain's sample either way."""
    ref, models_ref, ks_ref = undisturbed[place]
    recs, models, ks = between_run(place, which)
    assert [r["accepted"] for r in recs] == [r["accepted"] for r in ref] == [int(c == "A") for c in PLACE[place]]
    assert ks == ks_ref and [r["K0"] for r in recs] == [r["K0"] for r in ref]
    errs = {k: hm_err(np.array([r[k] for r in recs]), np.array([r[k] for r in ref])) for k in ("K1", "D1", "M1")}
    em = max(relmax(a, b) for a, b in zip(models, models_ref))
    counts = [r["nfevals"] for r in recs]
    print(f"\n[{which} {place.replace('_', ' ')}] nfevals {counts}: the step behind it "
          f"{'evaluated its start gradient again' if counts[2] == LB + 1 else 'kept its start gradient'}; {errs}, models {em:.2e}")
    assert max(errs.values()) < 1e-6 and em < 1e-7
    assert [r["nfevals"] for r in ref] == [LB + 1, LB, LB, LB]
    assert counts[:2] == [LB + 1, LB] and counts[3] == LB
    if which in EVALUATES:
        assert counts[2] == (LB + 1 if EVALUATES[which] else LB)
    else:
        assert counts[2] in (LB, LB + 1)


# ---- the chain's own bounds and step clamp -----------------------------------------------------------------------------------------
def test_chain_trajectory_that_clamps_and_reflects(monkeypatch):
    """The chain's lo / hi / dt in leapfrog_core: the upper half of the start model within 0.01 of hi, the lower half within 0.01 of
    lo, and a light mass (M^-1 of some 1e4), so that dt M^-1 p exceeds maxStepSize = 3 and the clamped step crosses the bounds.
    Against sampler.proposeLeapfrog on a context of its own, from the chain's start and the chain's own momentum (chain_state),
    at the bars of test_device_trajectory_with_the_step_clamp_active for the same kernels: 1e-9 (m), 5e-9 (p)."""
    P = problem("tiny")
    n, L, dt = P.n, 2, 0.03
    rng = np.random.default_rng(61)
    near = 0.01 * rng.random(n)
    start = np.where(np.arange(n) < n // 2, HI - near, LO + near)
    invM = 1e4 * P.invM
    ctx = HipContext(P.mesh, P.data, P.inv, device_id=0)
    try:
        ctx.set_prior(P.mref, P.inv.Wm, invM)
        D0, M0 = ctx.chain_begin(start, dt, REG, LO, HI)
        ctx.chain_momentum(normals(rng, n))
        p0 = ctx.chain_state()[1]
        ctx.chain_set_energy(D0 + FORCE, M0)
        rec, m_out, _ = ctx.chain_step(L, 0.5)
        p_out = ctx.chain_state()[1]
    finally:
        ctx.close()
    assert rec["accepted"] == 1 and rec["nfevals"] == L + 1
    seen = {"clamped": 0, "reflected": 0}
    kinetic_gradient, check_bound = sampler.getKineticGradient, sampler.checkParameterBound

    def watched_gradient(momentum, par):
        out = kinetic_gradient(momentum, par)
        seen["clamped"] += int(np.abs(dt * out).max() > 3.0)
        return out

    def watched_bound(model, momentum, prior):
        seen["reflected"] += int(((model < LO) | (model > HI)).sum())
        return check_bound(model, momentum, prior)

    monkeypatch.setattr(sampler, "getKineticGradient", watched_gradient)
    monkeypatch.setattr(sampler, "checkParameterBound", watched_bound)
    inv = copy.deepcopy(P.inv)
    inv.refModel = P.mref.copy()
    prior = HMCPrior(dt=dt, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=REG)
    assert np.log(prior.sigBounds[0]) == LO and np.log(prior.sigBounds[1]) == HI
    par = HMCParameter(n, start.copy(), p0.copy(), invM, np.sqrt(1.0 / invM))
    ref = HipContext(P.mesh, P.data, P.inv, device_id=0)
    try:
        m_ref, p_ref = sampler.proposeLeapfrog(par, P.mesh, P.data, inv, prior, None, L, ref)
    finally:
        ref.close()
    em, ep = relmax(m_out, m_ref), relmax(p_out, p_ref)
    print(f"\n[chain at its bounds] reference: {seen['clamped']} of {L} steps clamped, {seen['reflected']} reflections; "
          f"|m1 - m0| {np.abs(m_ref - start).max():.3f}; chain against it: m {em:.2e} (1e-9), p {ep:.2e} (5e-9)")
    assert seen["clamped"] >= 1 and seen["reflected"] >= 1
    assert m_out.min() >= LO and m_out.max() <= HI
    assert em < 1e-9 and ep < 5e-9


# ---- the headline size, on one context (last in the module: no other context of these tests lives beside it) ------------------------
@pytest.fixture(scope="module")
def cfg3_ctx():
    ctx = problem("cfg3").context()
    yield ctx
    ctx.close()


def test_forced_chain_against_the_reference_on_cfg3(cfg3_ctx):
    """20000 parameters: the reductions' second grid-stride pass (3616 parameters: 14 full workgroups and 32 threads), 79 workgroups of
    k_chain_welford"""
    P = problem("cfg3")
    assert P.n == 20000 > 64 * 256
    forced_run(P, cfg3_ctx)


def test_decision_rule_with_drawn_decisions_on_cfg3(cfg3_ctx):
    unforced_run(problem("cfg3"), cfg3_ctx)
