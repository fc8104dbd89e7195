"""The HMC chain on the device (hmcmt_chain_*): against the host sampler and the oracle's chain, its evaluation counts, its streaming
moments, repeatability, the state rules and a failed trajectory."""
import copy
import os

import numpy as np
import pytest

from hmcmt2d_amd import sampler
from hmcmt2d_amd.lib import HipContext, HmcmtError, HMCMT_MASS_WM
from hmcmt2d_amd.structs import HMCPrior
from tests.helpers import GOLDEN, make_problem, ragged_problem, relmax
from tests.golden.make_chain import chain_prior_of, start_model_of, SEED, RHOREF

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
LO, HI = float(np.log(1e-4)), 0.0
DT, REG, LTRAJ = 0.02, 1.0, 2
RHO = {"tiny": 122.0, "ragged": 90.0}          # homogeneous start / reference models from which proposals get accepted
STEPS = {"tiny": [1, 3], "ragged": [2, 4]}
SEED_RUN = 21


def problem(name):
    return ragged_problem(13, 10, 2, 2, 2, 3) if name == "ragged" else make_problem(name)


def prior_of(nsamples, burn, mass="diagonal", name="tiny"):
    return HMCPrior(totalsamples=nsamples, burninsamples=burn, dt=DT, timestep=list(STEPS[name]), sigBounds=[1e-4, 1.0], regParam=REG, massType=mass)


def run(name, prior, seed=SEED_RUN, **kw):
    mesh, data, inv, _ = problem(name)
    ctx = HipContext(mesh, data, inv, device_id=0)
    recs, step = [], ctx.chain_step

    def recording_step(L, u, outputs=True):                # (L, record) of every step the sampler takes
        out = step(L, u, outputs=outputs)
        recs.append((L, out[0]))
        return out

    ctx.chain_step = recording_step
    try:
        hm, st, hd = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(seed), rhoref=RHO[name], ctx=ctx, **kw)
        moments = ctx.chain_moments() if kw.get("device_chain") else None
    finally:
        ctx.close()
    return hm, st, hd, moments, recs


def hm_err(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max())


@pytest.fixture(scope="module")
def tiny12():
    """12 samples on `tiny`, burn-in 3: the host sampler with the device leapfrog, and the device chain (shared, left unchanged)"""
    ref = run("tiny", prior_of(12, 3), device_leapfrog=True)
    pr = prior_of(12, 3)
    dev = run("tiny", pr, device_chain=True)
    return ref, dev, pr


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_chain_against_the_host_sampler(name, tiny12):
    """device_chain=True and device_leapfrog=True from one seed: identical decisions, Hamiltonian terms to 1e-6 (the bound of
    tests/test_gpu_posterior.py), samples to 1e-7.  ragged: the active cells are not a box."""
    if name == "tiny":
        (hm0, st0, hd0, *_), (hm1, st1, hd1, *_), _ = tiny12
    else:
        hm0, st0, hd0, *_ = run(name, prior_of(12, 3, name=name), device_leapfrog=True)
        hm1, st1, hd1, *_ = run(name, prior_of(12, 3, name=name), device_chain=True)
    print(f"\n[chain vs host sampler, {name}] accepted {st1.nAccept} of 12; hmstats {hm_err(st1.hmstats, st0.hmstats):.2e}, samples {relmax(hm1, hm0):.2e}")
    assert 0 < st0.nAccept < 12                            # (both kinds of decision are compared)
    assert np.array_equal(st1.acceptstats, st0.acceptstats)
    assert hm_err(st1.hmstats, st0.hmstats) < 1e-6
    assert relmax(hm1, hm0) < 1e-7 and relmax(hd1, hd0) < 1e-6


def test_chain_against_the_oracle_chain_on_cfg2():
    g = np.load(os.path.join(GOLDEN, "cfg2_chain.npz"))
    mesh, data, inv, _ = make_problem("cfg2")
    prior = chain_prior_of("cfg2")
    prior.totalsamples = 30
    inv.strModel = start_model_of("cfg2", mesh, inv)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        hm, st, hd = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(SEED), rhoref=RHOREF, ctx=ctx, device_chain=True)
    finally:
        ctx.close()
    acc_o, hs_o = g["acceptstats"][:30], g["hmstats"][:, :31]
    same = st.acceptstats == acc_o
    nsame = 30 if same.all() else int(np.argmin(same))
    print(f"\n[chain vs oracle chain, cfg2] identical decisions for the first {nsame} of 30 samples")
    assert nsame >= min(20, 30)
    assert hm_err(st.hmstats[:, :nsame + 1], hs_o[:, :nsame + 1]) < 1e-6


def manual_chain(ctx, inv, nsteps, seed=9, burnin=3, outputs=True, between=None, start=None):
    """the chain API by hand on a context with a prior: records, the draws fixed by the seed"""
    rng = np.random.default_rng(seed)
    n = ctx.nAC
    start = np.full(n, np.log(1.0 / RHO["tiny"])) if start is None else start
    D0, M0 = ctx.chain_begin(start, DT, REG, LO, HI, burnin=burnin)
    recs, ks = [], [ctx.chain_momentum(rng.standard_normal(n))]
    for it in range(nsteps):
        if between is not None:
            between(it)
        rec, m, pred = ctx.chain_step(LTRAJ, rng.random(), outputs=outputs)
        recs.append(rec)
        ks.append(ctx.chain_momentum(rng.standard_normal(n)))
    return (D0, M0), recs, ks


def fresh(name="tiny", mass=None):
    mesh, data, inv, m = problem(name)
    ctx = HipContext(mesh, data, inv, device_id=0)
    n = ctx.nAC
    ctx.set_prior(np.full(n, np.log(1.0 / RHO["tiny"])), inv.Wm, np.ones(n))
    if mass == "wm":
        ctx.set_mass(HMCMT_MASS_WM)
    return ctx, inv, m


def test_nfevals_per_step_and_in_total(tiny12):
    _, (*_, recs), pr = tiny12
    ctx, inv, _ = fresh()
    try:
        _, manual, _ = manual_chain(ctx, inv, 5)
    finally:
        ctx.close()
    assert [r["nfevals"] for r in manual] == [LTRAJ + 1] + [LTRAJ] * 4         # only the first step evaluates its start gradient
    assert [r["nsamples"] for r in manual] == [1, 2, 3, 4, 5] and [r["nmoments"] for r in manual] == [0, 0, 0, 1, 2]
    # the sampler's chain, trajectories of several lengths: every record counts its own L (the first one more), and the sampler's
    # total is the sum of the records
    Ls, counts = [L for L, _ in recs], [r["nfevals"] for _, r in recs]
    assert len(recs) == 12 and len(set(Ls)) > 1
    assert counts == [Ls[0] + 1] + Ls[1:]
    assert pr.nfevals == sum(counts)


def test_moments_on_tiny(tiny12):
    _, (hm, st, _, moments, _), _ = tiny12
    assert st.acceptstats[3:].any()                        # (the chain moves behind the burn-in: the moments are not those of one model)
    for count, mean, m2 in (moments, st.moments):
        post = hm[:, 3:]
        assert count == 9
        assert np.abs(mean - post.mean(axis=1)).max() <= 1e-14 * np.abs(post.mean(axis=1)).max()
        var = post.var(axis=1)
        moved = var > 0
        # Welford subtracts the running mean from a sample, which cancels |mean| / std digits: 16 eps max(|mean| / std, 1) relative,
        # the bound at any number of parameters (tests/chain_ref.py: moments_bounds).  A few cells of this chain barely move (|mean| / std
        # up to 1e4, measured): for them the flat 1e-12 this test has always held is the tighter of the two, and it stays
        err = (np.abs(m2 / count - var)[moved] / var[moved])
        cond = np.maximum(np.abs(post.mean(axis=1)[moved]) / np.sqrt(var[moved]), 1.0)
        bound = np.minimum(16 * np.finfo(float).eps * cond, 1e-12)
        print(f"\n[moments on tiny] |mean| / std {np.median(cond):.1f} (median) to {cond.max():.1f}; relative variance error {err.max():.2e}, "
              f"at most {(err / bound).max():.2f} of its bound ({int((bound == 1e-12).sum())} of {moved.sum()} cells at the flat 1e-12)")
        assert np.all(err <= bound) and np.all(m2[~moved] == 0)
    assert np.array_equal(moments[1], st.moments[1]) and np.array_equal(moments[2], st.moments[2])


def test_outputs_are_side_effect_free_and_the_chain_repeats(tiny12):
    """keep_samples=False on a fresh context: bitwise the records and moments of the run that copied every sample out; a second fresh
    context with the same inputs: bitwise the same records, state and moments."""
    _, (hm, st, hd, moments, _), _ = tiny12
    _, st2, hd2, moments2, _ = run("tiny", prior_of(12, 3), device_chain=True, keep_samples=False)
    assert np.array_equal(st2.hmstats, st.hmstats) and np.array_equal(st2.acceptstats, st.acceptstats)
    assert moments2[0] == moments[0] and np.array_equal(moments2[1], moments[1]) and np.array_equal(moments2[2], moments[2])
    assert np.array_equal(hd2[:, 0], hd[:, 0])
    out = []
    for rep in range(2):
        ctx, inv, _ = fresh()
        try:
            res = manual_chain(ctx, inv, 5, outputs=bool(rep))
            out.append((res, ctx.chain_state(), ctx.chain_moments()))
            if rep:                                        # the moments into device memory: the same count and bits
                import torch
                d = torch.zeros(2, ctx.nAC, dtype=torch.float64, device=torch.device("cuda", 0))
                torch.cuda.synchronize()
                assert ctx.chain_moments_device(d[0].data_ptr(), d[1].data_ptr()) == out[-1][2][0]
                assert np.array_equal(d.cpu().numpy(), np.stack(out[-1][2][1:]))
        finally:
            ctx.close()
    (a, sa, ma), (b, sb, mb) = out
    assert a == b                                          # D0, M0, every field of every record, every kinetic energy: the same bits
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert ma[0] == mb[0] == 2 and np.array_equal(ma[1], mb[1]) and np.array_equal(ma[2], mb[2])


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_chain_with_the_wm_mass(name):
    """M = Wm: tiny (the mass separates) and the ragged problem (PCG), 6 samples against runHMCSampler(massType nondiagonal,
    device_leapfrog=True)."""
    hm0, st0, *_ = run(name, prior_of(6, 2, "nondiagonal", name), device_leapfrog=True)
    hm1, st1, *_ = run(name, prior_of(6, 2, "nondiagonal", name), device_chain=True)
    print(f"\n[chain, M = Wm, {name}] accepted {st1.nAccept} of 6; hmstats {hm_err(st1.hmstats, st0.hmstats):.2e}, samples {relmax(hm1, hm0):.2e}")
    assert 0 < st0.nAccept < 6                             # (both kinds of decision are compared)
    assert np.array_equal(st1.acceptstats, st0.acceptstats)
    assert hm_err(st1.hmstats, st0.hmstats) < 1e-6
    assert relmax(hm1, hm0) < 1e-7


def same_bits(a, b):
    """bit for bit, through what fills an HMCStatus field: tuples, lists, dicts, arrays, numbers, None"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_sampler_outputs_together_are_the_outputs_alone():
    """runHMCSampler(device_chain=True) with hist, data_moments, ess and cov all on, none on and one at a time -- every run on a context
    of its own, so that every chain's solves start cold -- : the chain keeps its bits whatever rides on its commit, and every
    HMCStatus field has the bits its keyword alone gives (a begin in the wrong place would count nothing or meet an ended accumulator,
    a read-out out of order the flush inside a batch of the covariance).  Then the same with a warm-up in front."""
    n = len(problem("tiny")[2].strModel)
    kws = {"hist": {"targets": [3, 3, n - 1, 0], "nbins": 17}, "data_moments": True, "ess": {"maxlag": 3}, "cov": {"rows": [0, 3], "batch": 2}}
    fields = {"hist": "hist", "data_moments": "dataMoments", "ess": "ess", "cov": "cov", "adapt": "adapt"}
    go = lambda **kw: run("tiny", prior_of(6, 2), device_chain=True, **kw)

    def same_chain(a, b):
        (hm0, st0, hd0, mom0, recs0), (hm1, st1, hd1, mom1, recs1) = a, b
        return (same_bits(hm0, hm1) and same_bits(hd0, hd1) and same_bits(st0.hmstats, st1.hmstats) and same_bits(st0.acceptstats, st1.acceptstats)
                and (st0.nAccept, st0.nReject) == (st1.nAccept, st1.nReject) and same_bits(st0.moments, st1.moments) and same_bits(mom0, mom1)
                and [L for L, _ in recs0] == [L for L, _ in recs1] and all(r0 == r1 for (_, r0), (_, r1) in zip(recs0, recs1)))

    none, allon = go(), go(**kws)
    assert 0 < none[1].nAccept < 6 and none[1].moments[0] == 4
    assert all(getattr(none[1], f) is None for f in fields.values())
    assert same_chain(allon, none)
    st = allon[1]
    assert st.hist[0] == st.dataMoments[0] == st.ess["count"] == st.cov["count"] == 4 and st.ess["misfit"]["count"] == 4
    assert st.hist[1].shape == (4, 17) and st.ess["acov"].shape == (4, n) and st.cov["cov"].shape == (2, n) and st.adapt is None
    for key in kws:
        alone = go(**{key: kws[key]})
        assert same_chain(alone, none), key
        assert getattr(st, fields[key]) is not None and same_bits(getattr(st, fields[key]), getattr(alone[1], fields[key])), key
        assert [k for k in fields if getattr(alone[1], fields[k]) is not None] == [key]
    warm, warm_all = go(adapt={"nwarmup": 2}), go(adapt={"nwarmup": 2}, **kws)
    assert same_chain(warm_all, warm)
    assert warm[1].adapt["nwarmup"] == 2 and warm[1].adapt["dt"].shape == (6,) and same_bits(warm_all[1].adapt, warm[1].adapt)
    assert all(getattr(warm_all[1], fields[k]) is not None for k in fields)
    assert all(getattr(warm_all[1], fields[k])[0 if isinstance(getattr(warm_all[1], fields[k]), tuple) else "count"] == 4 for k in kws)


def test_an_evaluation_between_two_steps_is_noticed():
    ctx, inv, m_other = fresh()
    try:
        _, ref, kref = manual_chain(ctx, inv, 6)
    finally:
        ctx.close()
    ctx, inv, m_other = fresh()
    try:
        def between(it):
            if it == 3:
                ctx.grad(m_other)                          # another model, between steps 3 and 4
        _, recs, ks = manual_chain(ctx, inv, 6, between=between)
    finally:
        ctx.close()
    print(f"\n[an evaluation between two steps] decisions {[r['accepted'] for r in ref]}")
    assert [r["accepted"] for r in recs] == [r["accepted"] for r in ref]
    assert [r["nfevals"] for r in recs] == [LTRAJ + 1, LTRAJ, LTRAJ, LTRAJ + 1, LTRAJ, LTRAJ]
    for key in ("K0", "K1", "D1", "M1", "D", "M"):
        a, b = np.array([r[key] for r in recs]), np.array([r[key] for r in ref])
        assert hm_err(a, b) < 1e-6, key


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def test_state_rules():
    mesh, data, inv, m = make_problem("tiny")
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        n = ctx.nAC
        start = np.full(n, np.log(1.0 / RHO["tiny"]))
        z = np.random.default_rng(1).standard_normal(n)
        assert code_of(lambda: ctx.chain_begin(start, DT, REG, LO, HI)) == EINVAL            # no prior
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == EINVAL                         # no chain
        ctx.set_prior(start, inv.Wm, np.ones(n))
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == EINVAL                         # still no chain
        ctx.chain_begin(start, DT, REG, LO, HI)
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == EINVAL                         # no momentum
        ctx.chain_momentum(z)
        rec, _, _ = ctx.chain_step(LTRAJ, 0.5)
        assert rec["nsamples"] == 1
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == EINVAL                         # the momentum was consumed
        # between grad_device_async and wait
        import torch
        dev = torch.device("cuda", 0)
        d_m = torch.from_numpy(m).to(dev)
        d_pred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device=dev)
        d_mis = torch.zeros(1, dtype=torch.float64, device=dev)
        d_g = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.chain_momentum(z)
        ctx.grad_device_async(d_m.data_ptr(), d_pred.data_ptr(), d_mis.data_ptr(), d_g.data_ptr())
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == EINVAL
        assert code_of(lambda: ctx.chain_momentum(z)) == EINVAL
        ctx.wait()
        rec, _, _ = ctx.chain_step(LTRAJ, 0.5)
        assert rec["nsamples"] == 2 and rec["nfevals"] == LTRAJ + 1                          # (the evaluation in between was noticed)
        # set_prior ends the chain
        ctx.chain_momentum(z)
        ctx.set_prior(start, inv.Wm, np.ones(n))
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == EINVAL
        assert code_of(lambda: ctx.chain_moments()) == EINVAL
        ctx.chain_begin(start, DT, REG, LO, HI)
        ctx.chain_momentum(z)
        assert ctx.chain_step(LTRAJ, 0.5)[0]["nsamples"] == 1
    finally:
        ctx.close()


def test_a_failed_trajectory_leaves_the_chain_where_it_was():
    ctx, inv, _ = fresh()
    try:
        rng = np.random.default_rng(2)
        n = ctx.nAC
        ctx.chain_begin(np.full(n, np.log(1.0 / RHO["tiny"])), DT, REG, LO, HI, burnin=1)
        for _ in range(3):
            ctx.chain_momentum(rng.standard_normal(n))
            rec, _, _ = ctx.chain_step(LTRAJ, rng.random())
        before = (ctx.chain_state()[0], ctx.chain_state()[2], ctx.chain_moments())
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)                           # an iteration cap no solve on this mesh meets
        ctx.chain_momentum(rng.standard_normal(n))
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == ENOCONV
        after = (ctx.chain_state()[0], ctx.chain_state()[2], ctx.chain_moments())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2][0] == after[2][0] == 2 and np.array_equal(before[2][1], after[2][1]) and np.array_equal(before[2][2], after[2][2])
        assert code_of(lambda: ctx.chain_step(LTRAJ, 0.5)) == EINVAL                         # the momentum counts as consumed
        ctx.set_options(maxit=maxit)
        ctx.chain_momentum(rng.standard_normal(n))
        rec2, _, _ = ctx.chain_step(LTRAJ, 0.5)
        assert rec2["nfevals"] == LTRAJ + 1 and rec2["nsamples"] == rec["nsamples"] + 1 == 4
    finally:
        ctx.close()
