"""The low-rank-plus-diagonal mass without a GPU: the item functions of its two kernels (hmcmt_items.h: item_mass_lr_*), instantiated
for the host (tests/emul/emul_mass_lowrank.cpp), against the numpy reference in the kernels' order bit for bit and against the dense
matrices (tests/mass_lowrank_ref.py); the identities M = F F' behind the momentum draw; sampler.lowRankMassFromSamples on samples
with a known low-rank structure; and the refusals of runHMCSampler(mass_lowrank=...) and HipContext.set_mass_lowrank, raised before
any call reaches a context."""
import numpy as np
import pytest

from hmcmt2d_amd import sampler
from hmcmt2d_amd import lib as L
from hmcmt2d_amd.structs import HMCPrior
from tests import mass_lowrank_ref as R
from tests.emul import emul_mass_lowrank_py as E
from tests.helpers import make_problem, relmax

SIZES = [96, 390, 20000]          # one partly filled workgroup; a full one plus a partial one; a second grid-stride pass
RANKS = [1, 5, 32]                # below a chunk of directions; an odd part of one; RANK_MAX = four whole chunks


def test_constants():
    c = E.constants()
    assert c == {"rank_max": L.HMCMT_MASS_RANK_MAX, "chunk": R.CHUNK, "blocks": R.NB} and c["rank_max"] == 32


def test_the_reference_fma_is_exact():
    """the reference's array fma against exact rational arithmetic, cancellation and ties included"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(4000), rng.standard_normal(4000)
    c = np.concatenate([rng.standard_normal(1000), -(a[1000:2000] * b[1000:2000]), -(a[2000:3000] * b[2000:3000]) * (1 + 2.0 ** -30),
                        rng.standard_normal(1000) * 2.0 ** -60])
    a[:4], b[:4], c[:4] = [1 + 2.0 ** -52, 1.0, 3.0, 1 + 2.0 ** -30], [1 + 2.0 ** -52, 2.0 ** -53, 2.0 ** -53, 1 + 2.0 ** -30], [1.0, 1.0, 1.0, -1.0]
    got = R.fma(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert got[i] == float(exact), (i, a[i], b[i], c[i])              # (float(Fraction) rounds to nearest even, once)


@pytest.mark.parametrize("n, rank", [(n, r) for n in SIZES for r in RANKS] + [(390, 8), (390, 9)])      # (8, 9: one whole chunk, one more)
def test_project_and_expand_in_the_kernels_order_and_against_dense_numpy(n, rank):
    invM, U, lam, x = R.problem(n, rank)
    for op in (R.OP_INV, R.OP_SQRT):
        part = E.project(invM, U, x, op)
        assert np.array_equal(part, R.project(invM, U, x, op))
        y = E.expand(invM, U, lam, x, part, op)
        assert np.array_equal(y, R.expand(invM, U, lam, x, part, op))
        assert np.array_equal(E.expand(invM, U, lam, x, part, op, in_place=True), y)
        # the projections themselves: t = U x' against numpy's, relative to |U| |x'| (what the roundings of a sum scale with)
        xp = R.pre(invM, x, op)
        assert np.abs(R.total(part) - U @ xp).max() <= 1e-13 * (np.abs(U) @ np.abs(xp)).max()
        err = relmax(y, R.apply_dense(invM, U, lam, x, op))    # (20000: the dense matrix would hold 3.2 GB; see apply_dense)
        print(f"[n {n}, rank {rank}, op {op}] relmax against dense numpy {err:.2e}")
        assert err < 1e-13


@pytest.mark.parametrize("rank", RANKS)
def test_kinetic_energy_of_a_drawn_momentum(rank):
    """K = 0.5 (F z)' M^-1 (F z) = 0.5 z'z, and F F' M^-1 = I: the momentum p = F z has covariance M"""
    n = 390
    invM, U, lam, _ = R.problem(n, rank)
    z = np.random.default_rng(7).standard_normal(n)
    for apply in (E.apply, R.apply):
        p = apply(invM, U, lam, z, R.OP_SQRT)
        K = 0.5 * float(p @ apply(invM, U, lam, p, R.OP_INV))
        assert abs(K - 0.5 * float(z @ z)) <= 1e-12 * 0.5 * float(z @ z)
    F, Mi = R.dense_sqrt(invM, U, lam), R.dense_inv(invM, U, lam)
    assert np.abs(F @ F.T @ Mi - np.eye(n)).max() < 1e-13


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def planted(n=390, N=40, seed=11):
    """samples = 1.5 + s Z sqrt(N - 1), Z = U0 Sigma0 V0' with V0 orthonormal and orthogonal to the ones vector: the row mean is
    exactly 1.5's, Z'Z has the eigenvalues Sigma0^2"""
    rng = np.random.default_rng(seed)
    s = np.sqrt(rng.uniform(0.25, 4.0, n))
    U0 = np.linalg.qr(rng.standard_normal((n, 4)))[0]
    sig2 = np.array([16.0, 9.0, 4.0, 2.5])
    V0 = np.linalg.qr(np.column_stack([np.ones(N), rng.standard_normal((N, 4))]))[0][:, 1:]
    Z = U0 @ np.diag(np.sqrt(sig2)) @ V0.T
    return 1.5 + s[:, None] * Z * np.sqrt(N - 1.0), s, U0, sig2


def test_estimator_recovers_a_planted_low_rank_structure():
    samples, s, U0, sig2 = planted()
    invM, U, lam = sampler.lowRankMassFromSamples(samples, rank=8, cutoff=2.0, invM=s ** 2)
    assert np.array_equal(invM, s ** 2) and U.shape == (4, 390) and U.flags["C_CONTIGUOUS"] and lam.shape == (4,)
    assert np.abs(lam - sig2).max() < 1e-10
    assert np.abs(np.abs(U0.T @ U.T) - np.eye(4)).max() < 1e-10
    assert np.abs(U @ U.T - np.eye(4)).max() < 1e-12
    for k in range(4):
        assert U[k, np.argmax(np.abs(U[k]))] > 0
    # the posterior covariance the mass stands for: M^-1 = S (I + U'(Lambda - I)U) S reproduces the samples' covariance along the directions
    C = np.cov(samples)
    Mi = R.dense_inv(invM, U, lam)
    for k in range(4):
        v = U[k] / s
        assert abs(v @ C @ v - v @ Mi @ v) < 1e-9 * abs(v @ Mi @ v)
    for kw, keep in ((dict(rank=3), 3), (dict(cutoff=3.0), 3), (dict(cutoff=20.0), 0), (dict(rank=0), 0)):
        i2, U2, l2 = sampler.lowRankMassFromSamples(samples, **{"rank": 8, "cutoff": 2.0, **kw}, invM=s ** 2)
        assert U2.shape == (keep, 390) and l2.shape == (keep,)
        assert np.allclose(l2, sig2[:keep], rtol=1e-10, atol=0)
    # without invM: the library's window rule for the scales
    N = samples.shape[1]
    i3, U3, l3 = sampler.lowRankMassFromSamples(samples)
    assert np.allclose(i3, samples.var(axis=1, ddof=1) * N / (N + 5) + 1e-3 * 5 / (N + 5), rtol=1e-14, atol=0)
    assert U3.shape[1] == 390 and np.abs(U3 @ U3.T - np.eye(len(l3))).max() < 1e-12 and np.all(l3 > 2.0) and np.all(np.diff(l3) <= 0)
    with pytest.raises(ValueError):
        sampler.lowRankMassFromSamples(samples[:, :1])
    with pytest.raises(ValueError):
        sampler.lowRankMassFromSamples(samples, invM=np.zeros(390))


# ---- refusals before any context call ----------------------------------------------------------------------------------------------
class Untouched:
    """a context (or a library) that no call may reach"""

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched: {name}")


def test_sampler_refuses_before_the_context_is_touched():
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    invM, U, lam, _ = R.problem(n, 3)
    good = (invM, U, lam)
    prior = lambda **kw: HMCPrior(totalsamples=2, burninsamples=0, dt=0.02, timestep=[1, 2], sigBounds=[1e-4, 1.0], **kw)
    go = lambda pr=None, **kw: sampler.runHMCSampler(mesh, data, inv, pr or prior(), np.random.default_rng(1), ctx=Untouched(), **kw)
    with pytest.raises(ValueError, match="needs device_chain=True"):
        go(mass_lowrank=good)
    with pytest.raises(ValueError, match="massType"):
        go(prior(massType="nondiagonal"), device_chain=True, mass_lowrank=good)
    with pytest.raises(ValueError, match="invM"):
        go(device_chain=True, mass_lowrank=good, invM=invM)
    with pytest.raises(ValueError, match="mass=True"):
        go(device_chain=True, mass_lowrank=good, adapt={"nwarmup": 1, "mass": True})
    for bad in ((invM, U[:, :-1], lam), (invM, U, lam[:-1]), (invM[:-1], U, lam), (invM, U.T, lam), (invM, U), (None, U, lam),
                (invM, np.zeros((33, n)), np.ones(33)), (invM, U, -lam), (invM, np.where(U == U[0, 0], np.nan, U), lam)):
        with pytest.raises(ValueError):
            go(device_chain=True, mass_lowrank=bad)
    with pytest.raises(AssertionError, match="touched"):                 # (the stand-in does notice a call: a good mass gets that far)
        go(device_chain=True, mass_lowrank=good)


def test_set_mass_lowrank_checks_shapes_before_the_library_call():
    n = 96
    invM, U, lam, _ = R.problem(n, 3)
    ctx = object.__new__(L.HipContext)
    ctx.nAC, ctx.lib, ctx.h = n, Untouched(), None
    for bad in ((invM, U[:, :-1], lam), (invM, U.T, lam), (invM, U[0], lam[:1]), (invM, U, lam[:-1]), (invM[:-1], U, lam), (None, U, lam[None, :])):
        with pytest.raises(ValueError):
            ctx.set_mass_lowrank(*bad)
    with pytest.raises(AssertionError, match="touched"):
        ctx.set_mass_lowrank(invM, U, lam)
    with pytest.raises(AssertionError, match="touched"):
        ctx.set_mass_lowrank(None, U, lam)
