"""tests/leapfrog_ref.py, the long-double reference of one trajectory, held to oracle.proposeLeapfrog / checkParameterBound: with a
smooth synthetic data gradient in place of compDataGradient, invM as a vector and as an operator, L = 1, 2, 3, and the cases in
which the position update goes wrong: the clamp, both bounds, an element exactly on a bound, bounds 0.7 apart (a clamped step of 3
reflects four times and more).  Agreement to the rounding of the oracle's float64 (leapfrog_ref.bars); every case asserts from the
reference's records that what it is about did happen."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

from hmcmt2d_amd.structs import HMCPrior
from oracle import hmcmt_oracle as O
from tests import leapfrog_ref as R

N = 24
REG = 0.7
LO, HI = float(np.log(1e-4)), float(np.log(1.0))
AMP, FREQ = 2.0, 0.7                            # the synthetic gradient a_i sin(0.7 m_i + phi_i), |a_i| <= 2: Lipschitz constant 1.4


def tridiagonal(n, d, o):
    return sp.diags([np.full(n - 1, o), np.full(n, d), np.full(n - 1, o)], [-1, 0, 1], format="csr")


WM = 0.3 * tridiagonal(N, 2.0, -1.0)            # the prior's Wm
MASS = tridiagonal(N, 2.5, -1.0)                # the operator mass: condition (2.5 + 2) / (2.5 - 2) = 9
COND = 9.0


class SolveOperator:
    """invM of proposeLeapfrog as an operator, in float64"""

    def __init__(self, A):
        self.A = A.toarray()

    def __mul__(self, p):
        return np.linalg.solve(self.A, np.asarray(p, dtype=np.float64))


def synthetic_gradient(rng):
    a, phi = rng.uniform(-AMP, AMP, N), rng.uniform(0, 2 * np.pi, N)
    return lambda m: a * np.sin(FREQ * np.asarray(m, dtype=np.float64) + phi)


def masses(kind, rng):
    """(invM for the oracle, the reference's operator, the relative error of the oracle's x)"""
    if kind == "vector":
        invM = rng.uniform(0.25, 4.0, N)
        return invM, R.DiagonalMass(invM), 0.0
    # LU of a symmetric positive definite matrix, no growth: n cond eps of max|x|
    return SolveOperator(MASS), R.WmMass(MASS), N * COND * R.EPS


def both(monkeypatch, m0, v0, dt, L, lo, hi, sig_bounds, kind, seed):
    rng = np.random.default_rng(seed)
    g = synthetic_gradient(rng)
    invM, mass, solve_rel = masses(kind, rng)
    mref = m0 - 0.1 * np.cos(np.arange(N))
    monkeypatch.setattr(O, "compDataGradient", lambda mesh, data, inv, prior, dense_dbc=True, keep=None: (None, 0.0, g(inv.strModel)))
    inv = types.SimpleNamespace(strModel=m0.copy(), refModel=mref, Wm=WM)
    prior = HMCPrior(dt=dt, sigBounds=list(sig_bounds), regParam=REG)
    assert np.log(prior.sigBounds[0]) == lo and np.log(prior.sigBounds[1]) == hi
    p_start = np.asarray(mass.mul(R._ld(v0)), dtype=np.float64)      # (the start is given as the velocity M^-1 p0 wanted)
    om, op = O.proposeLeapfrog(m0.copy(), p_start.copy(), invM, None, None, inv, prior, L)
    ref = R.trajectory(m0, p_start, dt, L, REG, mref, WM, lo, hi, mass, lambda k, m: g(m))
    assert prior.nfevals == ref["nfevals"] == L + 1
    bm, bp = R.bars(ref, mass, solve_rel=solve_rel, lipschitz=AMP * FREQ)
    em, ep = np.abs(om - ref["m"]), np.abs(op - ref["p"])
    rm, rp = float((em / bm[-1]).max()), float((ep / bp[-1]).max())
    print(f"\n[{kind}, L {L}] mx {[round(s['mx'], 3) for s in ref['steps']]}, reflections {[int(s['count'].sum()) for s in ref['steps']]} "
          f"(most {max(int(s['count'].max()) for s in ref['steps'])}); error over its bar: m {rm:.2g}, p {rp:.2g}")
    # the reference's decisions are not within rounding of going the other way
    for s, b in zip(ref["steps"], bm):
        assert abs(s["mx"] - R.MAX_STEP) > 1e-6
        assert np.all(s["margin"] > 4 * b)
    assert rm <= 1.0 and rp <= 1.0
    assert om.min() >= lo and om.max() <= hi
    return ref, om, op


KINDS = ["vector", "operator"]
LS = [1, 2, 3]


def velocity(rng, top, where=0, others=0.4):
    """the start velocity M^-1 p0 wanted (the gradient's half step moves it): |v| <= others * top but one element of size top"""
    v = others * top * rng.uniform(-1, 1, N)
    v[where] = top
    return v


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("kind", KINDS)
def test_no_clamp(monkeypatch, kind, L):
    rng = np.random.default_rng(1)
    m0 = -4.8 + 0.3 * rng.standard_normal(N)
    ref, _, _ = both(monkeypatch, m0, velocity(rng, 20.0), 0.02, L, LO, HI, (1e-4, 1.0), kind, 11)
    assert not any(s["clamped"] for s in ref["steps"]) and all(s["count"].sum() == 0 for s in ref["steps"])
    assert ref["steps"][0]["mx"] > 0.3


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("kind", KINDS)
def test_clamp(monkeypatch, kind, L):
    rng = np.random.default_rng(2)
    m0 = -4.8 + 0.3 * rng.standard_normal(N)
    ref, om, _ = both(monkeypatch, m0, velocity(rng, 300.0, where=N - 1), 0.02, L, LO, HI, (1e-4, 1.0), kind, 12)
    assert all(s["clamped"] for s in ref["steps"]) and ref["steps"][0]["mx"] > 5.0
    assert ref["steps"][0]["imax"] == N - 1
    if L == 1:
        assert abs(abs(om[N - 1] - m0[N - 1]) - 3.0) < 1e-14 and np.abs(om - m0).argmax() == N - 1


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("kind", KINDS)
def test_both_bounds_hit(monkeypatch, kind, L):
    rng = np.random.default_rng(3)
    near = 0.01 * rng.random(N)
    m0 = np.where(np.arange(N) < N // 2, HI - near, LO + near)
    ref, _, _ = both(monkeypatch, m0, velocity(rng, 300.0, where=5, others=0.8), 0.02, L, LO, HI, (1e-4, 1.0), kind, 13)
    first = ref["steps"][0]
    up, down = first["count"][:N // 2], first["count"][N // 2:]
    assert first["clamped"] and up.sum() >= 2 and down.sum() >= 2          # reflected at hi and at lo
    assert np.all(np.sign(np.asarray(first["p_position"], dtype=float)) == np.sign(np.asarray(first["p_before"], dtype=float)) * (-1) ** first["count"])


@pytest.mark.parametrize("side", ["hi", "lo"])
@pytest.mark.parametrize("kind", KINDS)
def test_an_element_lands_exactly_on_a_bound(monkeypatch, kind, side):
    """the clamped step's largest element moves by 3 exactly (dm / mx = 1): from hi - 3 to hi, from lo + 3 to lo; neither is a
    reflection, the momentum keeps its sign"""
    rng = np.random.default_rng(4)
    m0 = -4.8 + 0.3 * rng.standard_normal(N)
    j = 7
    m0[j] = HI - 3.0 if side == "hi" else LO + 3.0
    assert (m0[j] + 3.0 == HI) if side == "hi" else (m0[j] - 3.0 == LO)
    v = velocity(rng, 300.0 if side == "hi" else -300.0, where=j)
    ref, om, op = both(monkeypatch, m0, v, 0.02, 1, LO, HI, (1e-4, 1.0), kind, 14)
    s = ref["steps"][0]
    assert s["clamped"] and s["imax"] == j and s["count"][j] == 0
    assert om[j] == (HI if side == "hi" else LO)
    assert float(s["m"][j]) == om[j] and np.sign(float(s["p_position"][j])) == np.sign(float(s["p_before"][j]))


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("kind", KINDS)
def test_bounds_0p7_apart(monkeypatch, kind, L):
    """a clamped step of 3 between bounds 0.7 apart: four reflections and more, even and odd counts side by side"""
    sig = (float(np.exp(-5.2)), float(np.exp(-4.5)))
    lo, hi = float(np.log(sig[0])), float(np.log(sig[1]))
    assert 0.69 < hi - lo < 0.71
    rng = np.random.default_rng(5)
    m0 = rng.uniform(lo + 0.05, hi - 0.05, N)
    ref, _, _ = both(monkeypatch, m0, velocity(rng, 300.0, where=0, others=0.9), 0.02, L, lo, hi, sig, kind, 15)
    first = ref["steps"][0]
    assert first["clamped"] and first["count"][0] >= 4
    assert (first["count"] % 2 == 0).any() and (first["count"] % 2 == 1).any() and len(set(first["count"])) >= 3
    flips = np.sign(np.asarray(first["p_position"], dtype=float)) * np.sign(np.asarray(first["p_before"], dtype=float))
    assert np.array_equal(flips, (-1.0) ** first["count"])


def test_reflect_against_the_oracle_loop():
    """reflect() against checkParameterBound element by element, values on the bounds and far outside them included"""
    rng = np.random.default_rng(6)
    lo, hi = -5.2, -4.5
    m = np.concatenate([rng.uniform(lo - 4, hi + 4, 200), [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)]])
    p = rng.standard_normal(len(m))
    prior = HMCPrior(sigBounds=[1.0, 1.0])
    prior.sigBounds = [np.exp(lo), np.exp(hi)]
    lo64, hi64 = np.log(prior.sigBounds[0]), np.log(prior.sigBounds[1])
    om, op = O.checkParameterBound(m.copy(), p.copy(), prior)
    rm, rp, count, margin = R.reflect(R._ld(m), R._ld(p), R.LD(lo64), R.LD(hi64))
    assert np.abs(om - np.asarray(rm, dtype=float)).max() < 64 * R.EPS * 10
    assert np.array_equal(op, np.asarray(rp, dtype=float))
    assert np.array_equal(np.sign(op) * np.sign(p), (-1.0) ** count) and count.max() >= 5
    assert np.all(np.isinf(margin) == (count == 0))
