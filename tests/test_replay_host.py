"""The field replay (tests/replay_ref.py) on the CPU: fed with the oracle's own fields it is the oracle; against the host
emulation of the kernel bodies (tests/emul) it fixes the constants of the bars that tests/test_gpu_replay.py holds the
kernels to -- every ratio seen here stays below a quarter of its constant.  No GPU involved."""
import copy

import numpy as np
import pytest

from tests import replay_ref as RR, tipper_ref as TR
from tests.helpers import oracle_eval
from tests.emul.emul_py import Emul

U = RR.U


def _nodal(E, name):
    """The emulation's X / Lam in the oracle's layout: (TE, TM), each (nNode, nFreq)."""
    nF = E.S // 2
    A = E.get(name).reshape(E.S, E.NZP, E.NYP)[:, :E.nz + 1, :E.ny + 1].reshape(E.S, -1)
    return A[:nF].T.copy(), A[nF:].T.copy()


# ---------------------------------------------------------------------------------------- the replay of oracle fields
@pytest.mark.parametrize("name", ["P1", "P4", "P5"])
def test_replay_of_the_oracles_fields_is_the_oracle(name):
    mesh, data, inv, m = RR.problem(name)
    keep = {}
    po, mo, go = oracle_eval(copy.deepcopy(mesh), data, inv, m, dense_dbc=False, keep=keep)
    R = RR.Replay(mesh, data, inv, m)
    assert np.array_equal(R.pred(keep["exTE"], keep["hxTM"]), po)
    assert abs(float(R.misfit(po)) - mo) <= 4 * len(po) * U * mo
    lam = [np.zeros_like(keep["exTE"]), np.zeros_like(keep["hxTM"])]
    for (mode, f), t in keep["terms"].items():
        lam[mode == "TM"][R.ii, f] = t["eVal"]
    g = R.gradient((keep["exTE"], keep["hxTM"]), lam, po, spread=False)
    assert sorted(g["terms"]) == sorted(keep["terms"]) and not g["nodata"]
    for k, t in keep["terms"].items():
        for q in t:
            assert np.array_equal(g["terms"][k][q], t[q]), (k, q)
        assert g["res"][k] < 1e-12, (k, g["res"][k])                  # (the direct solve's residual)
    tot = g["A_a"] + g["A_b"] + g["A_c"]
    assert np.all(np.abs(g["a"] + g["b"] + g["c"] - go) <= 8 * U * tot)     # (the same terms, added in another order)


@pytest.mark.parametrize("name", ["P6-128", "P6-130T"])
def test_replay_of_the_oracles_fields_is_the_tipper_reference(name):
    """The virtual-receiver presentation of the tipper data against tests/tipper_ref.gradient (two separate products)."""
    mesh, data, inv, m = RR.problem(name)
    po, mo, go = TR.gradient(copy.deepcopy(mesh), data, inv, m)
    R = RR.Replay(mesh, data, inv, m)
    _, fwd = TR.forward(copy.deepcopy(mesh), data, TR.sigma_of(inv, m))
    assert np.array_equal(R.pred(fwd.exTE, fwd.hxTM), po)
    # lambda of the summed sources: one direct solve per system with the replay's own recorded right-hand sides
    lam0 = [np.zeros_like(fwd.exTE), np.zeros_like(fwd.hxTM)]
    g0 = R.gradient((fwd.exTE, fwd.hxTM), lam0, po, spread=False)
    lam = [np.zeros_like(fwd.exTE), np.zeros_like(fwd.hxTM)]
    for (mode, f) in g0["terms"]:
        Ainv = (fwd.AinvTE if mode == "TE" else fwd.AinvTM)[f]
        lam[mode == "TM"][R.ii, f] = Ainv.solve(g0["terms"][(mode, f)]["sVec"][R.ii])
    g = R.gradient((fwd.exTE, fwd.hxTM), lam, po, spread=False)
    assert max(g["res"].values()) < 1e-12
    tot = g["A_a"] + g["A_b"] + g["A_c"]
    assert np.all(np.abs(g["a"] + g["b"] + g["c"] - go) <= 1e-10 * tot)        # (two solves per system there, one here)


# ---------------------------------------------------------------------------------------- against the host emulation
@pytest.fixture(scope="module", params=RR.PROBLEMS)
def case(request):
    name = request.param
    mesh, data, inv, m = RR.problem(name)
    E = Emul(mesh, data, inv)
    real = data.dataType != "Impedance"
    pred, misfit, grad = E.grad(m, True, 2, 1e-13)
    pred = pred.real.copy() if real else pred
    X, Lam = _nodal(E, "X"), _nodal(E, "Lam")
    gP = E.get("gPart").reshape(2, -1)[:, inv.activeIdx] * np.exp(m)
    E.debug_flags(no_boundary_terms=True)
    _, _, grad_nb = E.grad(m, True, 2, 1e-13)                         # (the same solves again: same fields, to the bit)
    assert np.array_equal(_nodal(E, "Lam")[0], Lam[0])
    E.close()
    R = RR.Replay(mesh, data, inv, m)
    g = R.gradient(X, Lam, pred)
    return dict(name=name, R=R, g=g, pred=pred, misfit=misfit, grad=grad.copy(), grad_nb=grad_nb.copy(), gP=gP, X=X, Lam=Lam,
                data=data, inv=inv)


def _ratio(err, A):
    return float(np.max(err / (U * np.maximum(A, 1e-300))))


def test_data_and_misfit(case):
    R, pred = case["R"], case["pred"]
    ref = R.pred(*case["X"])
    r = _ratio(np.abs(pred - ref), np.abs(ref))
    mref = float(R.misfit(pred))
    rm = abs(case["misfit"] - mref) / (U * mref)
    print(f"replay host {case['name']}: data {r:.2f}  misfit {rm:.2f}  (units of 2^-53 A)")
    assert r <= RR.C_DATA / 4 and rm <= RR.C_MISFIT / 4, (r, rm)


def test_adjoint_sources(case):
    g = case["g"]
    worst = max(g["res"].values())
    print(f"replay host {case['name']}: adjoint residual {worst:.2e}")
    assert worst < 4e-13                                              # (the emulation's solve: tol 1e-13 on the error estimate)
    for mode, f in g["nodata"]:
        assert not case["Lam"][mode == "TM"][:, f].any()
    if case["name"] == "P6-130T":
        assert len(g["nodata"]) == 1 and not case["Lam"][1].any()     # TM systems off


def test_cell_terms(case):
    g = case["g"]
    ra = _ratio(np.abs(case["gP"][0] - g["a"]), g["A_a"]) if g["A_a"].any() else 0.0
    # the TM share against its own bar, with the kernels' own boundary values allowed for
    eb = np.abs(case["grad_nb"] - case["gP"][0] - g["b"])
    inner = g["A_bc"] == 0.0                                          # cells no edge of which lies on the mesh boundary
    eb = np.maximum(eb - 4 * U * g["A_a"], 0.0)                       # (exp(m) x the TE share: two roundings, of up to 2^-52 each)
    inner &= g["A_b"] > 0.0
    rb = _ratio(eb[inner], g["A_b"][inner]) if inner.any() else 0.0
    assert not eb[g["A_b"] == 0.0].any()
    bc = 0.0
    edge = g["A_bc"] > 0.0
    if edge.any():
        left = np.maximum(eb - rb * U * g["A_b"] - 4.0 * g["spread_b"], 0.0)[edge]
        bc = float(np.max(left / g["A_bc"][edge]))
    print(f"replay host {case['name']}: TE {ra:.2f}  TM+Q {rb:.2f} (units of 2^-53 A)  boundary cells beyond 4 x spread / boundary part of A {bc:.2e}")
    assert ra <= RR.C_TE / 4 and rb <= RR.C_TM / 4 and bc <= RR.BC_REL / 4, (ra, rb, bc)
    assert np.all(np.abs(case["grad_nb"] - g["a"] - g["b"]) <= RR.bar_ab(g))


def test_boundary_terms_and_the_condition_on_the_inputs(case):
    g = case["g"]
    err = np.abs(case["grad"] - case["grad_nb"] - g["c"])
    bar = RR.bar_c(g)
    shallow = ~g["deep"]
    cap = float(np.max(bar[shallow] / g["A_c"][shallow]))
    rc = _ratio(np.maximum(err - 4.0 * g["spread_c"], 0.0), g["A_c"])
    print(f"replay host {case['name']}: boundary terms: worst error / bar {np.max(err / bar):.3f}, beyond 4 x spread {rc:.3g} x 2^-53 A; "
          f"bar / A_c outside the deepest {RR.DEEP_ROWS} rows {cap:.2e}, error / A_c {np.max(err[shallow] / g['A_c'][shallow]):.2e}, "
          f"deep rows: bar / A_c {np.max(bar[~shallow] / g['A_c'][~shallow]):.2e}")
    assert np.all(g["A_c"] > 0)
    assert cap <= RR.CAP_C, cap                                       # the condition on the inputs: the reference alone
    assert np.all(err <= bar)
    assert rc <= RR.C_BND / 4
