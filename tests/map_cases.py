"""Shared by tests/test_map_host.py and tests/test_gpu_map.py: the MAP optimiser's test problems, the oracle-driven reference runs
(computed once per process and never changed) and the builders of L-BFGS histories for the direction tests."""
import functools

import numpy as np

from tests import map_ref as R
from tests.helpers import OracleContext, make_problem, ragged_problem

LN = np.log
MREF, LAMBDA, HISTORY, ITERS = LN(0.01), 1.0, 8, 12
# name -> (problem builder, lnSigMin, lnSigMax); the first three are padded meshes, on which the reference's gradient is the
# derivative of its misfit to 2e-6 along -g; on tiny it is not and the run stalls
CASES = {
    "r23_wide": (lambda: ragged_problem(23, 17, 3, 3, 3, 4), LN(1e-4), 0.0),
    "r23_tight": (lambda: ragged_problem(23, 17, 3, 3, 3, 4), LN(0.004), LN(0.03)),
    "r9_wide": (lambda: ragged_problem(9, 7, 2, 3, 3, 3), LN(1e-4), 0.0),
    "tiny": (lambda: make_problem("tiny"), LN(1e-4), 0.0),
}
PADDED = ("r23_wide", "r23_tight", "r9_wide")


def problem(name):
    """(mesh, data, inv, m_start, mref, lo, hi)"""
    mk, lo, hi = CASES[name]
    mesh, data, inv, m = mk()
    return mesh, data, inv, m, np.full(len(m), MREF), lo, hi


def prior_terms(inv, mref, m, lam=LAMBDA):
    """(M, lam Wm (m - mref)) in plain numpy"""
    r = m - mref
    w = inv.Wm.tocsr() @ r
    return 0.5 * lam * float(r @ w), lam * w


def oracle_objective(mesh, data, inv, mref, lam=LAMBDA):
    oc = OracleContext(mesh, data, inv)

    def f(m):
        _, D, g = oc.grad(m)
        M, gp = prior_terms(inv, mref, m, lam)
        return D + M, D, g + gp
    return f


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """dict(recs, phi0, m, nfevals, status, nbound) of the reference over the oracle: history 8, 12 iterations, start = the helper's model"""
    mesh, data, inv, m, mref, lo, hi = problem(name)
    run = R.RefMAP(oracle_objective(mesh, data, inv, mref), m, lo, hi, history=HISTORY)
    phi0, nb0, pginf0 = run.phi, run.nbound, run.pginf
    recs = run.run(ITERS)
    out = {"recs": recs, "phi0": phi0, "nbound0": nb0, "pginf0": pginf0, "m": run.m.copy(), "nfevals": run.nfevals, "status": run.status,
           "nbound": run.nbound}
    out["m"].setflags(write=False)
    return out


def quadratic_history(n, count, rng, cond=1e3):
    """count pairs (s, y = A s) of a convex quadratic with cond(A) <= cond, oldest first: A diagonal with a log-uniform spectrum in
    [1, cond]; the steps are random with a decaying scale, as an optimiser's are"""
    a = np.exp(rng.uniform(0.0, np.log(cond), n))
    pairs = []
    for i in range(count):
        s = rng.standard_normal(n) * 0.5 ** (i / 4.0)
        pairs.append((s, a * s))
    return pairs


def ring_of(pairs, H, head):
    """(rows [2 H, n], sy, yy [H, H] by slot) with pair i in slot (head + i) % H; the unused slots hold NaN so that a kernel that reads
    one shows"""
    n = len(pairs[0][0])
    rows = np.full((2 * H, n), np.nan)
    slots = [(head + i) % H for i in range(len(pairs))]
    for k, (s, y) in zip(slots, pairs):
        rows[k], rows[H + k] = s, y
    sy, yy = np.full((H, H), np.nan), np.full((H, H), np.nan)
    for i, ki in enumerate(slots):
        for j, kj in enumerate(slots):
            sy[ki, kj] = pairs[i][0] @ pairs[j][1]
            yy[ki, kj] = pairs[i][1] @ pairs[j][1]
    return rows, sy, yy


def planted_state(n, rng, lo, hi, bounds=True):
    """(m, g): a model inside the bounds and a gradient; with bounds, cells at lo with g > 0 (in B), at lo with g < 0 (not), at hi with
    g < 0 (in B), at hi with g > 0 (not), and exactly on a bound with g = 0 (not)"""
    m = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), n)
    g = rng.standard_normal(n)
    if bounds:
        idx = rng.permutation(n)[:12 if n < 200 else 40]
        k = len(idx) // 6
        m[idx[:k]], g[idx[:k]] = lo, np.abs(g[idx[:k]]) + 0.1
        m[idx[k:2 * k]], g[idx[k:2 * k]] = lo, -np.abs(g[idx[k:2 * k]]) - 0.1
        m[idx[2 * k:3 * k]], g[idx[2 * k:3 * k]] = hi, -np.abs(g[idx[2 * k:3 * k]]) - 0.1
        m[idx[3 * k:4 * k]], g[idx[3 * k:4 * k]] = hi, np.abs(g[idx[3 * k:4 * k]]) + 0.1
        m[idx[4 * k:5 * k]], g[idx[4 * k:5 * k]] = lo, 0.0
        m[idx[5 * k:]], g[idx[5 * k:]] = hi, 0.0
    return m, g


# (n, pairs, history, head): one partly filled workgroup, a full and a partial one, a second grid-stride pass; 1, 5, 8 and 32 pairs,
# rings that have wrapped (head != 0 with a full ring) and one that has not filled
DIRECTION_SHAPES = [(96, 1, 8, 0), (96, 8, 8, 3), (390, 5, 8, 0), (390, 32, 32, 5), (20000, 8, 8, 6), (20000, 32, 32, 0), (20000, 1, 1, 0)]
# the largest |d - d_ref|inf / |d_ref|inf of the host instantiation against the longdouble two-loop over DIRECTION_SHAPES, with and
# without bound cells, measured on the development machine; the tests assert 16 times it
DIRECTION_ERR_MEASURED = 8.5e-16
DIRECTION_BOUND = 16 * DIRECTION_ERR_MEASURED
