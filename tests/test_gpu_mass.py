"""The non-diagonal mass matrix M = Wm on the GPU (hmcmt_set_mass / hmcmt_mass_apply, kernels_mass.h): the two operators
against scipy, leapfrog trajectories under HMCMT_MASS_WM against the oracle's proposeLeapfrog with sparse mass operators, a
chain on the reference's coprod2 example with `masstype: nondiagonal` against the oracle's (tests/golden/make_chain_mass.py),
and the return to the diagonal mass bit for bit."""
import copy
import os
import tempfile

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from hmcmt2d_amd import sampler
from hmcmt2d_amd.structs import HMCPrior
from hmcmt2d_amd.lib import HipContext, HMCMT_MASS_DIAGONAL, HMCMT_MASS_WM, HMCMT_MASS_OP_INV, HMCMT_MASS_OP_SQRT
from tests.helpers import GOLDEN, make_problem, ragged_problem, relmax
from tests.test_mass import GEN

pytestmark = pytest.mark.gpu


def case(name):
    """(mesh, data, inv, m) of a configuration, an example directory (its start model) or the ragged problem"""
    if name in ("coprod2", "dprism3d"):
        with tempfile.TemporaryDirectory() as wd:
            mesh, data, inv, _ = GEN.nondiagonal_example(name, wd)
        return mesh, data, inv, inv.strModel.copy()
    if name == "ragged":
        return ragged_problem(13, 10, 2, 2, 2, 3)
    return make_problem(name)


def banded_factor(Wm):
    """scipy's lower banded Cholesky factor (cholesky_banded) and a matvec with it"""
    Wm = sp.csr_matrix(Wm)
    n = Wm.shape[0]
    coo = Wm.tocoo()
    b = int(np.abs(coo.row - coo.col).max())
    ab = np.zeros((b + 1, n))
    for d in range(b + 1):
        ab[d, :n - d] = Wm.diagonal(-d)
    lb = sla.cholesky_banded(ab, lower=True)

    def lmul(z):
        y = np.zeros(n)
        for d in range(b + 1):
            y[d:] += lb[d, :n - d] * z[:n - d]
        return y
    return b, lmul


def wm_context(mesh, data, inv, **kw):
    ctx = HipContext(mesh, data, inv, device_id=0, **kw)
    n = len(inv.strModel)
    ctx.set_prior(inv.refModel if inv.refModel is not None else inv.strModel, inv.Wm, np.ones(n))
    ctx.set_mass(HMCMT_MASS_WM)
    return ctx


@pytest.mark.parametrize("name", ["tiny", "coprod2", "dprism3d", "cfg3", "cfg5", "ragged"])
def test_mass_apply_against_scipy(name):
    mesh, data, inv, _ = case(name)
    n = len(inv.strModel)
    ctx = wm_context(mesh, data, inv)
    try:
        info = ctx.mass_info()
        b, lmul = banded_factor(inv.Wm)
        print(f"\n[{name}] nAC {n}, bandwidth {info['bandwidth']}, box {info['box_rows']} x {info['box_cols']}, "
              f"separable {info['separable']}, factor {info['factor_s']:.3f} s")
        assert info["kind"] == HMCMT_MASS_WM and info["bandwidth"] == b
        x = np.random.default_rng(n).standard_normal(n)
        y = ctx.mass_apply(HMCMT_MASS_OP_SQRT, x)
        assert relmax(y, lmul(x)) < 1e-13
        yi = ctx.mass_apply(HMCMT_MASS_OP_INV, x)
        ref = spla.splu(sp.csc_matrix(inv.Wm)).solve(x)
        assert relmax(yi, ref) < 1e-10
        assert np.linalg.norm(inv.Wm @ yi - x) / np.linalg.norm(x) <= 1e-12
        info = ctx.mass_info()
        if name == "ragged":
            assert not info["separable"] and info["pcg_iters"] >= 1
        else:
            assert info["separable"] and info["pcg_iters"] == 0
        # device pointers, in place
        import torch
        d = torch.from_numpy(x.copy()).cuda()
        ctx.mass_apply_device(HMCMT_MASS_OP_INV, d.data_ptr(), d.data_ptr())
        assert relmax(d.cpu().numpy(), ref) < 1e-10
    finally:
        ctx.close()


class WmInverse:
    def __init__(self, Wm):
        self.lu = spla.splu(sp.csc_matrix(Wm))

    def __mul__(self, p):
        return self.lu.solve(np.asarray(p, dtype=np.float64))


TRAJ = {"tiny": dict(dt=0.005, L=4), "coprod2": dict(dt=0.015, L=3), "cfg3": dict(dt=0.03, L=2)}


@pytest.mark.parametrize("name", ["tiny", "coprod2", "cfg3"])
def test_wm_trajectory_against_the_oracle(name):
    """hmcmt_leapfrog and hmcmt_leapfrog_device under HMCMT_MASS_WM, from p0 = L z, against oracle.proposeLeapfrog with invM = Wm^-1
    and sqrtM = L as scipy operators; and the proposal's kinetic energy 0.5 p'Wm^-1 p through hmcmt_mass_apply.  cfg3: the rough
    state of make_problem."""
    import torch
    from oracle import hmcmt_oracle as O
    mesh, data, inv, m = case(name)
    n = len(inv.strModel)
    inv.refModel = np.full(n, np.log(0.01))
    dt, L = TRAJ[name]["dt"], TRAJ[name]["L"]
    prior = HMCPrior(dt=dt, sigBounds=[1e-4, 1.0], regParam=1.0)
    lo, hi = np.log(prior.sigBounds[0]), np.log(prior.sigBounds[1])
    _, lmul = banded_factor(inv.Wm)
    z = np.clip(np.random.default_rng(5).standard_normal(n), -2.5, 2.5)
    p0 = lmul(z)
    omesh = copy.deepcopy(mesh)
    O.setupTensorMesh2D(omesh)
    om, op = O.proposeLeapfrog(m.copy(), p0.copy(), WmInverse(inv.Wm), omesh, data, copy.deepcopy(inv), copy.deepcopy(prior), L, False)
    ctx = wm_context(mesh, data, inv)
    try:
        ctx.set_prior(inv.refModel, inv.Wm, np.ones(n))
        ctx.set_mass(HMCMT_MASS_WM)
        assert relmax(ctx.mass_apply(HMCMT_MASS_OP_SQRT, z), p0) < 1e-13
        m1, p1, _, _, _, nf = ctx.leapfrog(m, p0, dt, L, 1.0, lo, hi)
        assert nf == L + 1
        print(f"\n[{name}] |m1 - m0| {np.abs(om - m).max():.3e}; host err m {relmax(m1, om):.2e} p {relmax(p1, op):.2e}")
        # coprod2 starts at a misfit of 3e6: its evaluations differ from the oracle's by 1e-9 whatever the mass (measured on the diagonal
        # trajectory below; tests/test_gpu_posterior.py bounds coprod2 the same way), and dt Wm^-1 carries that to 6e-8
        tol = 1e-6 if name == "coprod2" else 1e-8
        assert relmax(m1, om) < tol and relmax(p1, op) < tol
        # the proposal's kinetic energy 0.5 p'Wm^-1 p (getKineticEnergy through hmcmt_mass_apply) at that momentum
        K = 0.5 * float(p1 @ ctx.mass_apply(HMCMT_MASS_OP_INV, p1))
        Ko = 0.5 * float(p1 @ WmInverse(inv.Wm).__mul__(p1))
        assert abs(K - Ko) <= 1e-10 * abs(Ko)
        dm = torch.from_numpy(m.copy()).cuda(); dp = torch.from_numpy(p0.copy()).cuda()
        ctx.leapfrog_device(dm.data_ptr(), dp.data_ptr(), dt, L, 1.0, lo, hi)
        ctx.wait()
        assert relmax(dm.cpu().numpy(), om) < tol and relmax(dp.cpu().numpy(), op) < tol
        if name == "coprod2":
            # the diagonal trajectory from the same state: the evaluations' own difference to the oracle
            ctx.set_mass(HMCMT_MASS_DIAGONAL)
            dm1, dp1 = ctx.leapfrog(m, p0, dt, L, 1.0, lo, hi)[:2]
            odm, odp = O.proposeLeapfrog(m.copy(), p0.copy(), np.ones(n), omesh, data, copy.deepcopy(inv), copy.deepcopy(prior), L, False)
            print(f"[{name}] diagonal mass: err m {relmax(dm1, odm):.2e} p {relmax(dp1, odp):.2e}")
    finally:
        ctx.close()


def test_coprod2_nondiagonal_chain_decisions():
    """The reference's coprod2 example as shipped with `masstype: nondiagonal` appended to a copy of its start-up file, through
    runHMCSampler(device_leapfrog=True): the oracle chain's accept / reject decisions (tests/golden/coprod2_mass_chain.npz)."""
    g = np.load(os.path.join(GOLDEN, "coprod2_mass_chain.npz"))
    with tempfile.TemporaryDirectory() as wd:
        mesh, data, inv, prior = GEN.nondiagonal_example("coprod2", wd)
    assert prior.massType == "nondiagonal"
    prior.totalsamples = GEN.NSAMPLES
    prior.burninsamples = 0
    hm, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(GEN.SEED), rhoref=GEN.RHOREF, device_leapfrog=True)
    sampler.release_context(inv)
    acc = g["acceptstats"]
    print(f"\n[coprod2, M = Wm] accepted {st.nAccept} of {len(acc)} (oracle {int(acc.sum())}); nfevals {prior.nfevals} (oracle {int(g['nfevals'])})")
    assert np.array_equal(st.acceptstats, acc)
    err = np.abs(st.hmstats - g["hmstats"]) / np.maximum(np.abs(g["hmstats"]), 1.0)
    assert err.max() < 1e-6, err.max()
    assert relmax(hm[:, :5], g["first"]) < 1e-6
    assert prior.nfevals == int(g["nfevals"])


def test_diagonal_trajectory_unchanged_after_the_wm_mass():
    """hmcmt_set_mass(DIAGONAL) after WM, and a new hmcmt_set_prior after WM, run the diagonal trajectory bit for bit (cold starts:
    every evaluation depends on its model only)."""
    mesh, data, inv, m = make_problem("tiny")
    n = len(inv.strModel)
    mref = np.full(n, np.log(0.01))
    p0 = np.random.default_rng(9).standard_normal(n)
    args = (0.01, 3, 1.0, np.log(1e-4), 0.0)
    ctx = HipContext(mesh, data, inv, device_id=0, warm_start="cold")
    try:
        ctx.set_prior(mref, inv.Wm, np.ones(n))
        a = ctx.leapfrog(m, p0, *args)
        ctx.set_mass(HMCMT_MASS_WM)
        w = ctx.leapfrog(m, p0, *args)
        assert np.abs(w[0] - a[0]).max() > 1e-6                    # (the WM trajectory is another one)
        ctx.set_mass(HMCMT_MASS_DIAGONAL)
        assert ctx.mass_info()["kind"] == HMCMT_MASS_DIAGONAL
        b = ctx.leapfrog(m, p0, *args)
        ctx.set_mass(HMCMT_MASS_WM)
        ctx.set_prior(mref, inv.Wm, np.ones(n))
        assert ctx.mass_info()["kind"] == HMCMT_MASS_DIAGONAL
        c = ctx.leapfrog(m, p0, *args)
        for r in (b, c):
            assert np.array_equal(r[0], a[0]) and np.array_equal(r[1], a[1]) and np.array_equal(r[2], a[2]) and r[3] == a[3] and r[4] == a[4]
    finally:
        ctx.close()
