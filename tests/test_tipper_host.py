"""CPU tests of the tipper (TZY / RealTZY / ImagTZY): the test reference itself (tests/tipper_ref.py) against differences of
the oracle forward, the component codes and their refusals, the data-file round trip, and the node-window claim of
rx_tipper_deriv (hmcmt_math.h) that HostProblem::build_tipper_tables checks at create."""
import copy
import os

import numpy as np
import pytest

from hmcmt2d_amd import fileio, marshal, synthetic as S
from oracle import hmcmt_oracle as O
from tests import tipper_ref as TR
from tests.helpers import GOLDEN


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.fixture(scope="module")
def tiny_tipper():
    mesh, data, inv, m = TR.tipper_problem("tiny", "Impedance", with_impedance=False)
    return mesh, data, inv, m


def _sample_cells(mesh, inv):
    """active cells of the receiver row (all), the padding next to the edge receivers, and a few deeper ones"""
    ny, nz = mesh.gridSize
    nair = len(mesh.airLayer)
    act = list(inv.activeIdx)
    want = [nair * ny + k for k in range(ny)] + [(nair + 1) * ny, (nair + 1) * ny + ny - 1, (nair + 3) * ny + ny // 2]
    return [act.index(c) for c in want if c in act]


def test_reference_T_and_J_columns_match_central_differences(tiny_tipper):
    """With the Dirichlet values of the four sides held at the model's, central differences of T are exactly the P- and
    Q-terms of the patched oracle J (the reference's boundary-derivative terms approximate the derivative of its boundary
    values: tests/test_gradient_pin.py).  The full J is held against the full differences within the size of its boundary
    terms."""
    mesh, data, inv, m = tiny_tipper
    sig = TR.sigma_of(inv, m)
    keep = {}
    _, fwd = TR.forward(copy.deepcopy(mesh), data, sig, keep=keep)
    J = TR.tipper_jacobian(copy.deepcopy(mesh), data, sig, inv.activeIdx, fwd)          # d T / d sigma
    with TR.without_boundary_terms():
        Jpq = TR.tipper_jacobian(copy.deepcopy(mesh), data, sig, inv.activeIdx, fwd)
    h = 1e-4
    worst_fro = worst_full = 0.0
    for a in _sample_cells(mesh, inv):
        fd = {}
        for frozen in (True, False):
            mp, mm = m.copy(), m.copy()
            mp[a] += h
            mm[a] -= h
            bc = keep["bc"] if frozen else None
            Tp, _ = TR.forward(copy.deepcopy(mesh), data, TR.sigma_of(inv, mp), bc_fixed=bc)
            Tm, _ = TR.forward(copy.deepcopy(mesh), data, TR.sigma_of(inv, mm), bc_fixed=bc)
            fd[frozen] = (Tp - Tm) / (2 * h)
        sc = np.abs(J[:, a] * np.exp(m[a])).max()
        worst_fro = max(worst_fro, float(np.abs(Jpq[:, a] * np.exp(m[a]) - fd[True]).max() / sc))
        share = float(np.abs((J[:, a] - Jpq[:, a]) * np.exp(m[a])).max() / sc)
        e_full = float(np.abs(J[:, a] * np.exp(m[a]) - fd[False]).max() / sc)
        assert e_full < 1e-5 + 2.0 * share, (a, e_full, share)
        worst_full = max(worst_full, e_full)
    # (central differences in ln sigma at h = 1e-4: truncation ~h^2; measured 1e-9 and below)
    assert worst_fro < 1e-6, worst_fro


def test_reference_T_is_the_table_of_the_layout(tiny_tipper):
    """the forward puts T, Re T, Im T where the layout's table has them, after the impedance entries"""
    mesh, data, inv, m = tiny_tipper
    sig = TR.sigma_of(inv, m)
    mz = copy.deepcopy(mesh)
    pred, fwd = TR.forward(mz, data, sig)
    T = TR.tipper_table(mz, data, fwd)
    assert np.array_equal(pred, T.reshape(-1))
    assert np.abs(T).max() > 1e-4                                  # a 2-D model: the tipper is not zero
    dz = S.make_tipper_layout(data.freqs, data.rxLoc[:, 0], "Impedance", with_impedance=True)
    pz, _ = TR.forward(copy.deepcopy(mesh), dz, sig)
    assert np.array_equal(pz.reshape(len(data.freqs), -1, 3)[:, :, 2], T)
    dr = S.make_tipper_layout(data.freqs, data.rxLoc[:, 0], "Rho_Pha", with_impedance=True)
    pr, _ = TR.forward(copy.deepcopy(mesh), dr, sig)
    pr = pr.reshape(len(data.freqs), -1, 6)
    assert np.array_equal(pr[:, :, 4], T.real) and np.array_equal(pr[:, :, 5], T.imag)


# a 2-D model: the tipper is not zero


# ---------------------------------------------------------------------------------------------- codes and refusals
def test_comp_modes_accepts_the_tipper_codes_in_their_family():
    assert list(marshal.comp_modes(["ZXY", "ZYX", "TZY"], "Impedance")) == [1, 2, 7]
    assert list(marshal.comp_modes(["TZY"], "Impedance")) == [7]
    assert list(marshal.comp_modes(["RhoXY", "PhsXY", "RealTZY", "ImagTZY"], "Rho_Pha")) == [3, 4, 8, 9]
    assert list(marshal.comp_modes(["ImagTZY"], "Rho_Pha")) == [9]


@pytest.mark.parametrize("comps,dt", [(["ZXY", "RealTZY"], "Impedance"), (["TZY"], "Rho_Pha"),
                                      (["RhoXY", "TZY"], "Rho_Pha"), (["ImagTZY"], "Impedance")])
def test_comp_modes_refuses_a_tipper_component_of_the_other_family(comps, dt):
    with pytest.raises(ValueError, match="does not belong"):
        marshal.comp_modes(comps, dt)


@pytest.mark.parametrize("comps,dt", [(["TZY", "ZXY"], "Impedance"), (["RealTZY", "RhoXY", "PhsXY"], "Rho_Pha")])
def test_comp_modes_refuses_a_tipper_component_before_the_others(comps, dt):
    with pytest.raises(ValueError, match="after a tipper component"):
        marshal.comp_modes(comps, dt)


@pytest.mark.parametrize("family,withZ", [("Impedance", True), ("Impedance", False), ("Rho_Pha", True), ("Rho_Pha", False)])
def test_make_tipper_layout(family, withZ):
    d = S.make_tipper_layout([1.0, 0.1], [-100.0, 0.0, 100.0], family=family, with_impedance=withZ)
    nC = len(d.dataComp)
    assert d.dataComp[-1] in ("TZY", "ImagTZY")
    assert len(d.rxID) == 2 * 3 * nC and d.dataID.all()
    assert list(d.dtID[:nC]) == list(range(1, nC + 1))
    marshal.comp_modes(d.dataComp, d.dataType)                    # valid for the library


@pytest.mark.parametrize("family", ["Impedance", "Rho_Pha"])
def test_data_file_round_trip(tmp_path, family):
    d = S.make_tipper_layout([10.0, 1.0, 0.1], [-300.0, 0.0, 300.0], family=family)
    keep = np.ones(len(d.rxID), dtype=bool)
    keep[[1, 5, 7]] = False
    d.dataID = keep.copy()
    d.rxID, d.freqID, d.dtID = d.rxID[keep], d.freqID[keep], d.dtID[keep]
    rng = np.random.default_rng(3)
    n = len(d.rxID)
    vals = np.round(rng.standard_normal(n) * 1e-2, 8)
    if family == "Impedance":
        vals = vals + 1j * np.round(rng.standard_normal(n) * 1e-2, 8)
    err = np.round(np.abs(rng.standard_normal(n)) * 1e-3 + 1e-4, 9)
    fn = os.path.join(tmp_path, "tip.dat")
    fileio.writeMT2DData(fn, d, vals, err)
    d2, obs, err2 = fileio.readMT2DData(fn)
    assert d2.dataComp == d.dataComp and d2.dataType == d.dataType
    assert np.array_equal(d2.rxID, d.rxID) and np.array_equal(d2.freqID, d.freqID) and np.array_equal(d2.dtID, d.dtID)
    assert np.array_equal(d2.dataID, d.dataID)
    assert np.allclose(obs, vals, rtol=1e-6, atol=0) and np.allclose(err2, err, rtol=1e-6, atol=0)
    assert d2.compTE
    assert list(marshal.comp_modes(d2.dataComp, d2.dataType))[-1] in (7, 9)


# ---------------------------------------------------------------------------------------------- the window claim
def _window_ok(yNode, rxY):
    """Python mirror of HostProblem::build_tipper_tables: the cells of linRxMap2 read nodes inside the impedance's window."""
    ny = len(yNode) - 1
    yCen = 0.5 * (yNode[:-1] + yNode[1:])
    clampk = lambda k: min(max(k, 1), ny - 1)
    for y in rxY:
        kL, kR, _, _ = O.linearInterp(y, yNode)
        cL, cR, _, _ = O.linearInterp(y, yCen)
        n0 = min(clampk(kL), clampk(kR)) - 1
        if not (n0 <= cL and cR + 1 <= n0 + 3 and cR + 1 <= ny):
            return False
    return True


def _nodes(mesh):
    return np.concatenate([[0.0], np.cumsum(mesh.yLen)]) - mesh.origin[0]


@pytest.mark.parametrize("name", ["tiny", "cfg2", "cfg3"])
def test_window_claim_for_the_configs(name):
    mesh, d, _ = S.make_config(name)
    yN = _nodes(mesh)
    rx = list(d.rxLoc[:, 0])
    # a receiver on a node, at a cell centre, in the first and in the outermost cell, and in the padding
    rx += [yN[3], 0.5 * (yN[4] + yN[5]), yN[0] + 1.0, yN[0] + 0.5 * (yN[1] - yN[0]), yN[-1] - 1.0,
           yN[-1] - 0.25 * (yN[-1] - yN[-2]), yN[1] + 0.3 * (yN[2] - yN[1])]
    assert _window_ok(yN, rx)


def test_window_claim_for_the_example_meshes():
    ex = os.path.join(GOLDEN, "examples")
    found = 0
    for root, _, files in os.walk(ex):
        mods = [f for f in files if f.endswith(".mod")]
        dats = [f for f in files if f.endswith(".dat") and "obs" in f]
        for mf in mods:
            for df in dats:
                mesh = fileio.readEMModel2D(os.path.join(root, mf))
                d, _, _ = fileio.readMT2DData(os.path.join(root, df))
                yN = _nodes(mesh)
                assert _window_ok(yN, d.rxLoc[:, 0])
                found += 1
    assert found >= 1


def test_window_claim_on_random_meshes():
    rng = np.random.default_rng(11)
    for _ in range(200):
        ny = int(rng.integers(3, 30))
        yLen = np.exp(rng.uniform(np.log(10.0), np.log(1e4), ny))
        yN = np.concatenate([[0.0], np.cumsum(yLen)])
        rx = list(rng.uniform(yN[0], yN[-1] * (1 - 1e-12), 20)) + list(yN[:-1]) + list(0.5 * (yN[:-1] + yN[1:]))
        assert _window_ok(yN, rx)
