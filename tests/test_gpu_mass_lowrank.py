"""The low-rank-plus-diagonal mass on the GPU (hmcmt_set_mass_lowrank, kernels_mass.h: k_mass_lr_project, k_mass_lr_expand): the two
operators against numpy at one partly filled workgroup (tiny, 96 cells), a full one plus a partial one (the ragged problem, 390) and a
second grid-stride pass (cfg3, 20000); the refusals; leapfrog trajectories against the oracle's proposeLeapfrog with M^-1 as a numpy
operator; the return to the diagonal mass bit for bit; the chain API against a loop of the test's own; the sampler's keyword."""
import copy

import numpy as np
import pytest

from hmcmt2d_amd import sampler
from hmcmt2d_amd.lib import (HipContext, HmcmtError, HMCMT_MASS_DIAGONAL, HMCMT_MASS_WM, HMCMT_MASS_LOWRANK, HMCMT_MASS_OP_INV,
                             HMCMT_MASS_OP_SQRT)
from hmcmt2d_amd.structs import HMCPrior
from tests import chain_ref
from tests import mass_lowrank_ref as R
from tests.emul import emul_mass_lowrank_py as E
from tests.helpers import make_problem, ragged_problem, relmax
from tests.test_gpu_chain import hm_err
from tests.test_gpu_chain_kernels import problem as chain_problem

pytestmark = pytest.mark.gpu

EINVAL = -1
LO, HI = float(np.log(1e-4)), 0.0
REG = 1.0
RANKS = [1, 5, 32]
FORCE = 1e12                                   # added to / taken from the chain's misfit: hdif > 0, or exp(hdif) == 0
SEQ = "AARARA"


def case(name):
    return ragged_problem(23, 17, 3, 3, 3, 4) if name == "ragged" else make_problem(name)


def code_of(call):
    with pytest.raises(HmcmtError) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("name", ["tiny", "ragged", "cfg3"])
def test_mass_apply_against_numpy(name):
    import torch
    mesh, data, inv, _ = case(name)
    n = len(inv.strModel)
    assert n == {"tiny": 96, "ragged": 390, "cfg3": 20000}[name]
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        ctx.set_prior(inv.strModel, inv.Wm, np.ones(n))
        for rank in RANKS:
            invM, U, lam, x = R.problem(n, rank)
            assert lam.max() == 16.0 and (rank == 1 or lam.min() == 0.25)
            ctx.set_mass_lowrank(invM, U, lam)
            info = ctx.mass_info()
            assert info["kind"] == HMCMT_MASS_LOWRANK == 2
            assert not any(info[k] for k in ("factor_s", "bandwidth", "separable", "pcg_iters", "box_rows", "box_cols"))
            for op in (HMCMT_MASS_OP_INV, HMCMT_MASS_OP_SQRT):
                ref = R.apply_dense(invM, U, lam, x, op)
                y = ctx.mass_apply(op, x)
                d = torch.from_numpy(x.copy()).cuda()
                ctx.mass_apply_device(op, d.data_ptr(), d.data_ptr())          # device pointers, in place
                yd = d.cpu().numpy()
                print(f"\n[{name}, rank {rank}, op {op}] relmax against numpy: host pointers {relmax(y, ref):.2e}, device pointers {relmax(yd, ref):.2e}")
                assert relmax(y, ref) < 1e-13 and relmax(yd, ref) < 1e-13
                assert np.array_equal(ctx.mass_apply(op, x), y) and np.array_equal(yd, y)      # no atomics: the bits repeat
                assert np.array_equal(y, E.apply(invM, U, lam, x, op))                         # ... and are the host instantiation's
        # invM = NULL: the scales are the prior's diagonal
        invM, U, lam, x = R.problem(n, 5)
        ctx.set_mass_lowrank(invM, U, lam)
        y = ctx.mass_apply(HMCMT_MASS_OP_INV, x)
        ctx.set_prior(inv.strModel, inv.Wm, invM)
        assert ctx.mass_info()["kind"] == HMCMT_MASS_DIAGONAL
        ctx.set_mass_lowrank(None, U, lam)
        assert np.array_equal(ctx.mass_apply(HMCMT_MASS_OP_INV, x), y)
    finally:
        ctx.close()


def test_refusals_leave_the_mass_as_it_was():
    P = chain_problem("tiny")
    n = P.n
    invM, U, lam, x = R.problem(n, 5)
    ctx = P.context()
    try:
        def refused(label, kind, probe):
            bad = {"rank 0": (invM, U[:0], lam[:0]), "rank 33": (invM, np.zeros((33, n)), np.ones(33)),
                   "NaN in U": (invM, np.where(U == U[2, 7], np.nan, U), lam), "lambda = 0": (invM, U, np.where(lam == lam[1], 0.0, lam)),
                   "lambda = inf": (invM, U, np.where(lam == lam[1], np.inf, lam)), "invM < 0": (-invM, U, lam),
                   "U not orthonormal": (invM, U * np.where(np.arange(5) == 3, 1 + 1e-6, 1.0)[:, None], lam)}
            for what, args in bad.items():
                assert code_of(lambda: ctx.set_mass_lowrank(*args)) == EINVAL, (label, what)
            assert ctx.lib.hmcmt_set_mass_lowrank(ctx.h, None, 5, None, lam.ctypes.data_as(ctx.lib.hmcmt_set_mass_lowrank.argtypes[4])) == EINVAL
            assert code_of(lambda: ctx.set_mass(HMCMT_MASS_LOWRANK)) == EINVAL
            assert ctx.mass_info()["kind"] == kind, label
            assert np.array_equal(ctx.mass_apply(HMCMT_MASS_OP_INV, x), probe), label      # the context is usable, the mass what it was

        refused("diagonal", HMCMT_MASS_DIAGONAL, P.invM * x)
        with pytest.raises(HmcmtError, match="hmcmt_set_mass_lowrank"):
            ctx.set_mass(HMCMT_MASS_LOWRANK)
        with pytest.raises(HmcmtError, match="orthonormal"):
            ctx.set_mass_lowrank(invM, U * (1 + 1e-6), lam)
        ctx.set_mass(HMCMT_MASS_WM)
        refused("Wm", HMCMT_MASS_WM, ctx.mass_apply(HMCMT_MASS_OP_INV, x))
        ctx.set_mass_lowrank(invM, U, lam)
        y = ctx.mass_apply(HMCMT_MASS_OP_INV, x)
        assert relmax(y, R.apply_dense(invM, U, lam, x, HMCMT_MASS_OP_INV)) < 1e-13
        refused("low rank", HMCMT_MASS_LOWRANK, y)
        # under the low-rank mass the chain has no diagonal to set or to adapt; its step size it has
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        assert code_of(lambda: ctx.chain_set_mass_diag(P.invM)) == EINVAL
        with pytest.raises(HmcmtError, match="HMCMT_MASS_LOWRANK"):
            ctx.chain_set_mass_diag(P.invM)
        assert code_of(lambda: ctx.chain_adapt_begin(nwarmup=4, adapt_mass=1, init_buffer=1, term_buffer=1, base_window=2)) == EINVAL
        ctx.chain_set_dt(0.5 * P.dt)
        ctx.chain_adapt_begin(nwarmup=4, adapt_mass=0)
        assert ctx.chain_adapt_info()["active"] == 1
        assert ctx.mass_info()["kind"] == HMCMT_MASS_LOWRANK and np.array_equal(ctx.mass_apply(HMCMT_MASS_OP_INV, x), y)
        # a refused set call leaves a running chain alone; an accepted one ends it
        assert code_of(lambda: ctx.set_mass_lowrank(invM, U, 0.0 * lam)) == EINVAL
        ctx.chain_momentum(np.zeros(n))
        ctx.set_mass_lowrank(invM, U, lam)
        assert code_of(lambda: ctx.chain_momentum(np.zeros(n))) == EINVAL
    finally:
        ctx.close()


TRAJ = {"tiny": dict(dt=0.005, L=4), "cfg3": dict(dt=0.03, L=2)}            # (tests/test_gpu_mass.py)


@pytest.mark.parametrize("name", ["tiny", "cfg3"])
def test_lowrank_trajectory_against_the_oracle(name):
    """hmcmt_leapfrog and hmcmt_leapfrog_device under the low-rank mass, from p0 = F clip(z), against oracle.proposeLeapfrog with M^-1 as
    a numpy operator"""
    import torch
    from oracle import hmcmt_oracle as O
    mesh, data, inv, m = make_problem(name)
    n = len(inv.strModel)
    inv.refModel = np.full(n, np.log(0.01))
    dt, L = TRAJ[name]["dt"], TRAJ[name]["L"]
    prior = HMCPrior(dt=dt, sigBounds=[1e-4, 1.0], regParam=1.0)
    invM, U, lam, _ = R.problem(n, 5)
    assert invM.max() * lam.max() <= 64.0
    z = np.clip(np.random.default_rng(5).standard_normal(n), -2.5, 2.5)
    p0 = R.apply_dense(invM, U, lam, z, R.OP_SQRT)
    omesh = copy.deepcopy(mesh)
    O.setupTensorMesh2D(omesh)
    om, op = O.proposeLeapfrog(m.copy(), p0.copy(), R.Inverse(invM, U, lam), omesh, data, copy.deepcopy(inv), copy.deepcopy(prior), L, False)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        ctx.set_prior(inv.refModel, inv.Wm, np.ones(n))
        ctx.set_mass_lowrank(invM, U, lam)
        assert relmax(ctx.mass_apply(HMCMT_MASS_OP_SQRT, z), p0) < 1e-13
        m1, p1, _, _, _, nf = ctx.leapfrog(m, p0, dt, L, 1.0, LO, HI)
        assert nf == L + 1
        dm = torch.from_numpy(m.copy()).cuda(); dp = torch.from_numpy(p0.copy()).cuda()
        nfd = ctx.leapfrog_device(dm.data_ptr(), dp.data_ptr(), dt, L, 1.0, LO, HI)
        ctx.wait()
        md, pd = dm.cpu().numpy(), dp.cpu().numpy()
        print(f"\n[{name}] |m1 - m0| {np.abs(om - m).max():.3e}; host err m {relmax(m1, om):.2e} p {relmax(p1, op):.2e}; "
              f"device err m {relmax(md, om):.2e} p {relmax(pd, op):.2e}")
        assert np.abs(om - m).max() > 1e-3
        assert relmax(m1, om) < 1e-8 and relmax(p1, op) < 1e-8
        assert nfd == L + 1 and relmax(md, om) < 1e-8 and relmax(pd, op) < 1e-8
    finally:
        ctx.close()


def test_diagonal_trajectory_unchanged_after_the_lowrank_mass():
    """hmcmt_set_mass(DIAGONAL) after the low-rank mass, and a new hmcmt_set_prior after it, run the diagonal trajectory bit for bit
    (cold starts: every evaluation depends on its model only) -- with a non-unit diagonal, which the low-rank call must not write"""
    mesh, data, inv, m = make_problem("tiny")
    n = len(inv.strModel)
    mref = np.full(n, np.log(0.01))
    p0 = np.random.default_rng(9).standard_normal(n)
    args = (0.01, 3, 1.0, np.log(1e-4), 0.0)
    invM, U, lam, _ = R.problem(n, 5)
    diag = np.random.default_rng(4).uniform(0.5, 2.0, n)
    ctx = HipContext(mesh, data, inv, device_id=0, warm_start="cold")
    try:
        ctx.set_prior(mref, inv.Wm, diag)
        a = ctx.leapfrog(m, p0, *args)
        ctx.set_mass_lowrank(invM, U, lam)
        w = ctx.leapfrog(m, p0, *args)
        assert np.abs(w[0] - a[0]).max() > 1e-6                    # (the low-rank trajectory is another one)
        ctx.set_mass(HMCMT_MASS_DIAGONAL)
        assert ctx.mass_info()["kind"] == HMCMT_MASS_DIAGONAL
        b = ctx.leapfrog(m, p0, *args)
        ctx.set_mass_lowrank(None, U, lam)
        ctx.set_prior(mref, inv.Wm, diag)
        assert ctx.mass_info()["kind"] == HMCMT_MASS_DIAGONAL
        c = ctx.leapfrog(m, p0, *args)
        for r in (b, c):
            assert np.array_equal(r[0], a[0]) and np.array_equal(r[1], a[1]) and np.array_equal(r[2], a[2]) and r[3] == a[3] and r[4] == a[4]
    finally:
        ctx.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
LCHAIN = 2


def lowrank_chain(P, mass, nadapt=2):
    """SEQ by the chain API on a context of its own under `mass`, the decisions planted through chain_set_energy; then a warm-up of the
    step size alone over `nadapt` more steps.  Returns what every step saw and gave."""
    rng = np.random.default_rng(17)
    ctx = P.context()
    steps = []
    try:
        ctx.set_mass_lowrank(*mass)
        D, Mn = ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=2)
        begin = (D, Mn)
        for it, force in enumerate(SEQ + "-" * nadapt):
            if it == len(SEQ):
                ctx.chain_adapt_begin(nwarmup=nadapt, adapt_mass=0)
            z = 1.5 * rng.standard_normal(P.n)
            K = ctx.chain_momentum(z)
            m_before, p, _ = ctx.chain_state()
            D_set = D + FORCE if force == "A" else D - FORCE if force == "R" else D
            if force != "-":
                ctx.chain_set_energy(D_set, Mn)
            u = rng.random()
            dt = ctx.chain_adapt_info()["dt"] if it >= len(SEQ) else P.dt
            rec, m_out, _ = ctx.chain_step(LCHAIN, u)
            steps.append(dict(z=z, K=K, p=p, D_set=D_set, M=Mn, u=u, rec=rec, m_before=m_before, m_out=m_out, dt=dt))
            if rec["accepted"]:
                D, Mn = rec["D"], rec["M"]
            elif force == "R":
                ctx.chain_set_energy(D, Mn)
        info = ctx.chain_adapt_info()
    finally:
        ctx.close()
    return begin, steps, info


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_chain_with_the_lowrank_mass(name):
    """6 steps by the chain API with fixed draws against a loop of the test's own: p = F clip(z) and K in numpy, the trajectory by
    hmcmt_leapfrog on a second context with the same mass"""
    P = chain_problem(name)
    invM, U, lam, _ = R.problem(P.n, 5)
    assert not np.array_equal(invM, P.invM)                 # (scales of the mass's own, not the prior's diagonal)
    (D0, M0), steps, info = lowrank_chain(P, (invM, U, lam))
    recs = [s["rec"] for s in steps]
    assert [r["accepted"] for r in recs[:len(SEQ)]] == [int(c == "A") for c in SEQ]
    assert [r["nfevals"] for r in recs] == [LCHAIN + 1] + [LCHAIN] * (len(recs) - 1)       # only the first step evaluates its start gradient
    Minv = R.Inverse(invM, U, lam)
    ref = P.context()
    worst = {k: 0.0 for k in ("p", "K0", "K1", "D1", "M1", "model")}
    try:
        ref.set_mass_lowrank(invM, U, lam)
        m_cur = P.start.copy()
        for it, s in enumerate(steps):
            rec = s["rec"]
            p_ref = R.apply_dense(invM, U, lam, np.clip(s["z"], -2.5, 2.5), R.OP_SQRT)
            K0 = 0.5 * float(p_ref @ (Minv * p_ref))
            m1, p1, _, D1, M1, _ = ref.leapfrog(m_cur, p_ref, s["dt"], LCHAIN, REG, LO, HI)
            K1 = 0.5 * float(p1 @ (Minv * p1))
            hdif, accepted = chain_ref.decision(s["D_set"], s["M"], K0, D1, K1, M1, s["u"])
            assert rec["accepted"] == int(accepted), (it, rec, hdif)
            assert np.array_equal(s["m_before"], P.start if it == 0 else steps[it - 1]["m_out"])
            worst["p"] = max(worst["p"], relmax(s["p"], p_ref))
            for key, got, want in (("K0", rec["K0"], K0), ("K1", rec["K1"], K1), ("D1", rec["D1"], D1), ("M1", rec["M1"], M1)):
                worst[key] = max(worst[key], hm_err(np.array(got), np.array(want)))
            assert rec["K0"] == s["K"]
            if accepted:
                m_cur = m1
            worst["model"] = max(worst["model"], relmax(s["m_out"], m_cur))
    finally:
        ref.close()
    print(f"\n[chain, low-rank mass, {name}] nAC {P.n}; decisions {[r['accepted'] for r in recs]}; largest differences to the loop: {worst}")
    assert worst["p"] < 1e-13
    assert max(worst[k] for k in ("K0", "K1", "D1", "M1")) < 1e-6 and worst["model"] < 1e-7
    # the warm-up of the step size alone ran to its end under the mass
    assert info["active"] == 0 and info["step"] == 2 and info["windows_done"] == 0
    assert np.isfinite(info["dt"]) and info["dt"] > 0 and steps[-1]["dt"] != P.dt
    # a fresh context repeats the chain bit for bit
    again = lowrank_chain(P, (invM, U, lam))
    assert again[0] == (D0, M0) and [s["rec"] for s in again[1]] == recs and [s["K"] for s in again[1]] == [s["K"] for s in steps]
    assert all(np.array_equal(a["m_out"], b["m_out"]) and np.array_equal(a["p"], b["p"]) for a, b in zip(again[1], steps))
    assert again[2] == info


# ---- the sampler's keyword ---------------------------------------------------------------------------------------------------------
RHO = 122.0


def sampler_prior():
    return HMCPrior(totalsamples=6, burninsamples=2, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0], regParam=REG)


def sampled(seed=21, **kw):
    """runHMCSampler(device_chain=True) on tiny on a context of its own; returns (hmcmodel, hmcstats, the records of its steps)"""
    mesh, data, inv, _ = make_problem("tiny")
    ctx = HipContext(mesh, data, inv, device_id=0)
    recs, step = [], ctx.chain_step

    def recording_step(L, u, outputs=True):
        out = step(L, u, outputs=outputs)
        recs.append((L, out[0]))
        return out

    ctx.chain_step = recording_step
    try:
        hm, st, _ = sampler.runHMCSampler(mesh, data, inv, sampler_prior(), np.random.default_rng(seed), rhoref=RHO, ctx=ctx, device_chain=True, **kw)
    finally:
        ctx.close()
    return hm, st, recs


def test_sampler_keyword():
    """mass_lowrank=(invM, U, lam): the records of the same chain by the chain API with the sampler's draws in the sampler's order; no
    direction at all: the bits of invM="""
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    invM, U, lam, _ = R.problem(n, 5)
    hm, st, recs = sampled(mass_lowrank=(invM, U, lam))
    assert len(recs) == 6 and st.nAccept + st.nReject == 6
    # by hand: the first momentum's normals; set_prior, the mass; begin at the homogeneous model, then at the file's; per sample L, u, z
    rng = np.random.default_rng(21)
    pr = sampler_prior()
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        z = rng.standard_normal(n)
        start = np.log(np.ones(n) / RHO)
        ctx.set_prior(start, inv.Wm, invM)
        ctx.set_mass_lowrank(invM, U, lam)
        D0, M0 = ctx.chain_begin(start, pr.dt, REG, LO, HI, burnin=2)
        if not np.array_equal(inv.strModel, start):
            ctx.chain_begin(inv.strModel, pr.dt, REG, LO, HI, burnin=2)
            ctx.chain_set_energy(D0, M0)
        ks, manual, models = [ctx.chain_momentum(z)], [], []
        for it in range(6):
            L = int(rng.integers(1, 4))
            rec, m, _ = ctx.chain_step(L, rng.random())
            manual.append((L, rec)); models.append(m)
            ks.append(ctx.chain_momentum(rng.standard_normal(n)))
    finally:
        ctx.close()
    assert manual == recs
    assert np.array_equal(hm, np.array(models).T) and np.array_equal(st.hmstats[2], np.array(ks))
    # another chain than the diagonal mass's ...
    hm_d, st_d, recs_d = sampled(invM=invM)
    assert not np.array_equal(st_d.hmstats, st.hmstats)
    # ... which is what a mass without directions gives
    hm_0, st_0, recs_0 = sampled(mass_lowrank=(invM, U[:0], lam[:0]))
    assert recs_0 == recs_d and np.array_equal(hm_0, hm_d) and np.array_equal(st_0.hmstats, st_d.hmstats)
    # a warm-up beside the mass adapts the step size alone
    hm_a, st_a, _ = sampled(mass_lowrank=(invM, U, lam), adapt={"nwarmup": 2})
    assert st_a.adapt["nwarmup"] == 2 and st_a.adapt["invM"] is None and np.isfinite(st_a.adapt["dt_final"])
