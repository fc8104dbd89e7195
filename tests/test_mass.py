"""The non-diagonal mass matrix M = Wm (masstype: nondiagonal; HMCSampler.jl:80-86, :478-489) on the host side, no GPU:
the premise of the library's direct Wm^-1 (Wm is the separable box operator on the meshes the project runs), the sampler's
chain with the mass operators of a context (an oracle-backed stand-in here) against the oracle's chain, and the checkpoint
fingerprint."""
import copy
import hashlib
import importlib.util
import os
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg  # noqa: F401

from hmcmt2d_amd import sampler, lib
from hmcmt2d_amd.structs import HMCPrior
from tests.helpers import GOLDEN, OracleContext, make_problem, ragged_problem


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_chain_mass", os.path.join(GOLDEN, "make_chain_mass.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_generator()


def ddx_t_ddx(n):
    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0
    if n == 1:
        d[0] = 0.0
    return sp.diags([d, -np.ones(n - 1), -np.ones(n - 1)], [0, 1, -1], format="csr")


def box_operator(nzb, nyb):
    """I (x) T_y + T_z (x) I with T_y = ddx'ddx (Neumann), T_z = ddx'ddx + e0 e0' (the air above the top row)"""
    Ty = ddx_t_ddx(nyb)
    Tz = (ddx_t_ddx(nzb) + sp.csr_matrix(([1.0], ([0], [0])), shape=(nzb, nzb))).tocsr()
    return (sp.kron(sp.identity(nzb), Ty) + sp.kron(Tz, sp.identity(nyb))).tocsr()


def active_box(mesh, inv):
    ny = mesh.gridSize[0]
    kz, ky = np.asarray(inv.activeIdx) // ny, np.asarray(inv.activeIdx) % ny
    return kz.min(), kz.max() - kz.min() + 1, ky.min(), ky.max() - ky.min() + 1


def example(name):
    with tempfile.TemporaryDirectory() as wd:
        return GEN.nondiagonal_example(name, wd)


def problems():
    out = {}
    for name in ("tiny", "cfg3"):
        mesh, _, inv, _ = make_problem(name)
        out[name] = (mesh, inv)
    for name in ("coprod2", "dprism3d"):
        mesh, _, inv, prior = example(name)
        assert prior.massType == "nondiagonal"
        out[name] = (mesh, inv)
    return out


@pytest.mark.parametrize("name", ["tiny", "cfg3", "coprod2", "dprism3d"])
def test_wm_is_the_separable_box_operator(name):
    """The active cells fill the earth rectangle and Wm equals the box operator exactly: the transform pair of kernels_mass.h
    is the solve there."""
    mesh, inv = problems()[name]
    kz0, nzb, ky0, nyb = active_box(mesh, inv)
    assert nzb * nyb == len(inv.activeIdx)
    assert kz0 > 0                                         # (air above: the e0 e0' term of T_z)
    assert abs(inv.Wm - box_operator(nzb, nyb)).max() == 0.0


def test_wm_of_the_ragged_problem_is_not_the_box_operator():
    """One frozen earth cell: the active set is not a box, the library must run PCG there."""
    mesh, _, inv, _ = ragged_problem(12, 9, 1, 2, 2, 3)
    kz0, nzb, ky0, nyb = active_box(mesh, inv)
    assert nzb * nyb != len(inv.activeIdx)
    B = box_operator(nzb, nyb)
    keep = np.zeros(nzb * nyb, dtype=bool)
    ny = mesh.gridSize[0]
    keep[(np.asarray(inv.activeIdx) // ny - kz0) * nyb + (np.asarray(inv.activeIdx) % ny - ky0)] = True
    assert inv.Wm.shape != B.shape
    # Wm is the box operator's principal submatrix on the active cells, whose inverse is not the restricted box inverse
    sub = B[keep][:, keep]
    assert abs(inv.Wm - sub).max() == 0.0
    x = np.random.default_rng(1).standard_normal(len(inv.activeIdx))
    xe = np.zeros(nzb * nyb); xe[keep] = x
    assert np.abs(sp.linalg.spsolve(sub.tocsc(), x) - sp.linalg.spsolve(B.tocsc(), xe)[keep]).max() > 1e-3


@pytest.mark.parametrize("n", [1, 2, 7, 45, 76])
def test_closed_form_eigenpairs(n):
    """lambda_y,k = 2 - 2 cos(pi k / n) with DCT-II vectors; lambda_z,k = 2 - 2 cos(pi (2k+1) / (2n+1)) with sin(theta_k (i+1))"""
    k, i = np.arange(n), np.arange(n)
    Ty = ddx_t_ddx(n).toarray()
    Tz = Ty.copy(); Tz[0, 0] += 1.0
    ly = 2 - 2 * np.cos(np.pi * k / n)
    lz = 2 - 2 * np.cos(np.pi * (2 * k + 1) / (2 * n + 1))
    Qy = np.cos(np.pi * np.outer(i + 0.5, k) / n); Qy /= np.linalg.norm(Qy, axis=0)
    th = np.pi * (2 * k + 1) / (2 * n + 1)
    Qz = np.sin(np.outer(i + 1, th)); Qz /= np.linalg.norm(Qz, axis=0)
    assert np.abs(Ty @ Qy - Qy * ly).max() < 1e-13 and np.abs(Tz @ Qz - Qz * lz).max() < 1e-13
    assert np.abs(Qy.T @ Qy - np.eye(n)).max() < 1e-13 and np.abs(Qz.T @ Qz - np.eye(n)).max() < 1e-13
    assert np.abs(np.sort(ly) - np.linalg.eigvalsh(Ty)).max() < 1e-13
    assert np.abs(np.sort(lz) - np.linalg.eigvalsh(Tz)).max() < 1e-13


class MassStandIn(OracleContext):
    """The oracle-backed stand-in of tests/helpers.py with the mass interface of HipContext (set_prior / set_mass /
    mass_apply), served by scipy: a dense Cholesky factor and a sparse LU of Wm."""

    def set_prior(self, mref, Wm, invM):
        self.Wm, self.invM, self.kind = sp.csr_matrix(Wm), np.asarray(invM, dtype=np.float64).copy(), lib.HMCMT_MASS_DIAGONAL

    def set_mass(self, kind):
        self.kind = kind
        if kind == lib.HMCMT_MASS_WM:
            self.inv_op, self.L = GEN.wm_mass(self.Wm)

    def mass_apply(self, op, x):
        if self.kind == lib.HMCMT_MASS_DIAGONAL:
            return self.invM * x if op == lib.HMCMT_MASS_OP_INV else x / np.sqrt(self.invM)
        return self.inv_op * x if op == lib.HMCMT_MASS_OP_INV else self.L @ x


def chain_prior(mass):
    return HMCPrior(totalsamples=6, burninsamples=0, dt=0.005, timestep=[1, 3], sigBounds=[1e-4, 1.0], massType=mass)


def test_sampler_chain_with_the_wm_mass_equals_the_oracle_chain():
    """runHMCSampler with massType = "nondiagonal" (the mass operators of the context: setMassMatrix(invParam, ctx)) takes the
    oracle's decisions and samples (chain loop of tests/golden/make_chain_mass.py, scipy's mass operators)."""
    from oracle import hmcmt_oracle as O
    mesh, data, inv, _ = make_problem("tiny")
    prior = chain_prior("nondiagonal")
    hm, st, _ = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), prior, np.random.default_rng(7), rhoref=100.0,
                                      ctx=MassStandIn(mesh, data, inv))
    omesh = copy.deepcopy(mesh)
    O.setupTensorMesh2D(omesh)
    oprior = chain_prior("nondiagonal")
    ohm, ohs, oacc = GEN.run_chain(omesh, data, copy.deepcopy(inv), oprior, np.random.default_rng(7), 100.0)
    assert np.array_equal(st.acceptstats, oacc) and 0 < oacc.sum() < len(oacc)        # (both kinds of decision)
    assert np.abs(hm - ohm).max() < 1e-10
    assert np.abs(st.hmstats - ohs).max() <= 1e-10 * np.abs(ohs).max()
    assert prior.nfevals == oprior.nfevals
    # (the mass matters: the diagonal chain from the same seed is another chain)
    hd, _, _ = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), chain_prior("diagonal"), np.random.default_rng(7),
                                     rhoref=100.0, ctx=MassStandIn(mesh, data, inv))
    assert np.abs(hd - hm).max() > 1e-6


def test_set_mass_matrix_forms():
    """setMassMatrix(nparam, scaling) stays the diagonal pair; setMassMatrix(invParam, ctx) gives operators whose `*` applies
    Wm^-1 and chol(Wm).L through the context, so the kinetic terms and the momentum draw run unchanged."""
    invM, sqrtM = sampler.setMassMatrix(5, 4.0)
    assert np.array_equal(invM, np.full(5, 0.25)) and np.array_equal(sqrtM, np.full(5, 2.0))
    mesh, data, inv, _ = make_problem("tiny")
    ctx = MassStandIn(mesh, data, inv)
    iM, sM = sampler.setMassMatrix(inv, ctx)
    n = len(inv.strModel)
    p = np.random.default_rng(3).standard_normal(n)
    W = inv.Wm.toarray()
    hp = sampler.HMCParameter(n, np.zeros(n), p, iM, sM)
    assert np.abs(W @ sampler.getKineticGradient(p, hp) - p).max() < 1e-10
    assert abs(sampler.getKineticEnergy(p, hp) - 0.5 * p @ np.linalg.solve(W, p)) < 1e-9 * abs(p @ np.linalg.solve(W, p))
    z = np.clip(np.random.default_rng(4).standard_normal(n), -2.5, 2.5)
    assert np.abs(sampler.getMomentumVector(n, hp, np.random.default_rng(4)) - np.linalg.cholesky(W) @ z).max() < 1e-12


def _fingerprint_before(invParam, hmcprior, shape):
    """the checkpoint fingerprint as it was before the mass type existed"""
    h = hashlib.sha256()
    h.update(np.asarray(shape, dtype=np.int64).tobytes())
    h.update(np.asarray([hmcprior.dt, hmcprior.regParam, *hmcprior.timestep, *hmcprior.sigBounds], dtype=np.float64).tobytes())
    for a in (invParam.obsData, invParam.dataW, invParam.refModel):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_checkpoint_fingerprint_carries_a_non_diagonal_mass_only():
    _, _, inv, _ = make_problem("tiny")
    inv.refModel = inv.strModel.copy()
    shape = (len(inv.strModel), 4)
    fd = sampler._run_fingerprint(inv, chain_prior("diagonal"), shape)
    fn = sampler._run_fingerprint(inv, chain_prior("nondiagonal"), shape)
    assert fd == _fingerprint_before(inv, chain_prior("diagonal"), shape)       # (existing checkpoints stay valid)
    assert fn != fd
