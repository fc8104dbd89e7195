"""Test reference for the tipper T = Hz/Hy (TZY, RealTZY, ImagTZY), built from the oracle's own pieces.

The oracle has no tipper: the reference package defines it (dataFuncSens.jl:44-112) but never computes it in its forward
solver.  Here
  * the forward restates T = Hzr / Hyr from the fields of oracle.MT2DFwdSolver (direct solves), Hzr = linRxMap2^T (Bz0/mu0),
    Hyr = linRxMap^T Hy0 (tipper_te);
  * J's tipper rows are oracle.compJacMat with getDataFuncSensTE patched to return (dT, dT/dsigma): the tipper data are
    presented as ZXY data, so that function's TE rows are the T rows and P, the boundary terms and Q follow the oracle;
  * the gradient is g_imp + g_tip: the oracle's compDataGradient on the non-tipper data, the patched compJacTMatVec (TZY) or
    the patched J (RealTZY / ImagTZY) on the tipper data.
tests/test_tipper_host.py checks the restatement against central differences of the oracle forward.
"""
from __future__ import annotations

import contextlib
import copy

import numpy as np
import scipy.sparse as sp

from hmcmt2d_amd import synthetic as S, invsetup as I
from hmcmt2d_amd.structs import HMCPrior, MTData
from oracle import hmcmt_oracle as O

TIPPER = ("TZY", "RealTZY", "ImagTZY")


def tipper_te(omega, rx: O.PreRxSens, Ex01):
    """(T, dT/dF, dT/dsigma) of every receiver at one frequency: dataFuncSens.jl:44-112 (T, dT, dT_dsig), with the oracle's
    getDataFuncSensTE for Hy."""
    dEx0, dEx1, sigma1, dsigma1 = rx.dFn0, rx.dFn1, rx.sigma1, rx.dsigma1
    yLen, zLen1 = rx.yLen, rx.zLen1
    ny = len(yLen)
    mu = O.MU0 * np.ones(ny)
    Bz0 = (O.ddx(ny) @ Ex01[:, 0]) / yLen / (1j * omega)
    Bz1 = (O.ddx(ny) @ Ex01[:, 1]) / yLen / (1j * omega)
    dtmp = O.sdiag(1.0 / yLen / (1j * omega)) @ O.ddx(ny)
    dBz0, dBz1 = dtmp @ dEx0, dtmp @ dEx1
    HzQ = (0.75 * Bz0 + 0.25 * Bz1) / mu
    dHzQ = O.sdiag(1.0 / mu) @ (0.75 * dBz0 + 0.25 * dBz1)
    HyH = -(Ex01[1:-1, 1] - Ex01[1:-1, 0]) / zLen1 / (1j * omega * O.MU0)
    dHyH = -(dEx1[1:-1, :] - dEx0[1:-1, :]) / zLen1 / (1j * omega * O.MU0)
    ExQ = 0.75 * Ex01[1:-1, 0] + 0.25 * Ex01[1:-1, 1]
    dExQ = 0.75 * dEx0[1:-1, :] + 0.25 * dEx1[1:-1, :]
    avl = O.avnc(ny - 1) @ yLen
    sigma1v = (O.avnc(ny - 1) @ (sigma1 * yLen)) / avl
    dsigma1v = O.sdiag(1.0 / avl) @ O.avnc(ny - 1) @ O.sdiag(yLen) @ dsigma1
    dHzQ_dy = (O.ddx(ny - 1) @ HzQ) / avl
    ddHzQ = O.sdiag(1.0 / avl) @ O.ddx(ny - 1) @ dHzQ
    Hy0 = np.zeros(ny + 1, dtype=complex)
    Hy0[1:-1] = HyH - (dHzQ_dy - sigma1v * ExQ) * (0.5 * zLen1)
    Hy0[0], Hy0[-1] = Hy0[1], Hy0[-2]
    dHy0 = O._edge_dup(dHyH - (ddHzQ - O.sdiag(sigma1v) @ dExQ) * (0.5 * zLen1))
    dHy0_dsig = O._edge_dup(0.5 * zLen1 * (O.sdiag(ExQ) @ dsigma1v))
    Hyr = rx.linRxMap.T @ Hy0
    Hzr = rx.linRxMap2.T @ (Bz0 / mu)
    dHyr = rx.linRxMap.T @ dHy0
    dHzr = rx.linRxMap2.T @ O.sdiag(1.0 / mu) @ dBz0
    dHyr_dsig = rx.linRxMap.T @ dHy0_dsig
    T = Hzr / Hyr
    dT = O.sdiag(1.0 / Hyr) @ dHzr - O.sdiag(Hzr / Hyr ** 2) @ dHyr
    dT_dsig = -O.sdiag(Hzr / Hyr ** 2) @ dHyr_dsig
    return T, sp.csr_matrix(dT), sp.csr_matrix(dT_dsig)


@contextlib.contextmanager
def without_boundary_terms():
    """oracle.getBCderivTE / TM return a zero dBC inside the block: J is then the derivative with the Dirichlet values held
    (the P- and Q-terms), which central differences with frozen boundary values measure exactly."""
    te, tm = O.getBCderivTE, O.getBCderivTM
    O.getBCderivTE = lambda *a: (lambda r: (0.0 * r[0], r[1]))(te(*a))
    O.getBCderivTM = lambda *a: (lambda r: (0.0 * r[0], r[1]))(tm(*a))
    try:
        yield
    finally:
        O.getBCderivTE, O.getBCderivTM = te, tm


@contextlib.contextmanager
def tipper_rows_as_te():
    """oracle.getDataFuncSensTE returns the tipper's (dT, dT/dsigma) inside the block."""
    orig = O.getDataFuncSensTE
    O.getDataFuncSensTE = lambda omega, rx, Ex01, dataType: tipper_te(omega, rx, Ex01)[1:]
    try:
        yield
    finally:
        O.getDataFuncSensTE = orig


# ---------------------------------------------------------------------------------------------------------- layouts
def n_imp(data):
    return sum(c not in TIPPER for c in data.dataComp)


def split(data):
    """(non-tipper data indices, tipper data indices, non-tipper MTData with its own full-table mask or None)."""
    ni = n_imp(data)
    ii = np.nonzero(data.dtID <= ni)[0]
    it = np.nonzero(data.dtID > ni)[0]
    sub = None
    if ni:
        comps = list(data.dataComp[:ni])
        nF, nR, nC = len(data.freqs), data.rxLoc.shape[0], len(data.dataComp)
        mask = np.asarray(data.dataID, dtype=bool).reshape(nF, nR, nC)[:, :, :ni].reshape(-1)
        sub = MTData(data.rxLoc, data.freqs, data.dataType, comps, data.rxID[ii], data.freqID[ii], data.dtID[ii], mask,
                     any("XY" in c for c in comps), any("YX" in c for c in comps))
    return ii, it, sub


def as_zxy(data, it):
    """The tipper data `it` presented as ZXY data (DataType Impedance), so that the oracle's TE rows are theirs."""
    nF, nR = len(data.freqs), data.rxLoc.shape[0]
    mask = np.zeros((nF, nR), dtype=bool)
    mask[data.freqID[it] - 1, data.rxID[it] - 1] = True
    return MTData(data.rxLoc, data.freqs, "Impedance", ["ZXY"], data.rxID[it], data.freqID[it],
                  np.ones(len(it), dtype=np.int64), mask.reshape(-1), True, False)


def full_impedance(data):
    return S.make_data_layout(data.freqs, data.rxLoc[:, 0], data.rxLoc[0, 1])


def sigma_of(inv, m):
    sig = inv.bgModel.copy()
    sig[inv.activeIdx] += np.exp(m)
    return sig


# ---------------------------------------------------------------------------------------------------------- forward
def _setup(mesh, sigma):
    mesh.sigma = np.asarray(sigma, dtype=float).copy()
    O.setupTensorMesh2D(mesh)


def tipper_table(mesh, data, fwd):
    """T[f, r] from the TE fields of an oracle forward solution, or from an (nNode, nFreq) array of TE fields fetched
    elsewhere (tests/replay_ref.py)."""
    fwd = fwd if hasattr(fwd, "exTE") else O.MT2DFwdData(np.asarray(fwd), None, None, None, "")
    ny, nz = mesh.gridSize
    yN = np.concatenate([[0.0], np.cumsum(mesh.yLen)]) - mesh.origin[0]
    zN = np.concatenate([[0.0], np.cumsum(mesh.zLen)]) - mesh.origin[1]
    rx = O.preSetRxFieldSens(data.rxLoc, yN, zN, mesh.sigma)
    zid = rx.zid
    id0 = slice(zid * (ny + 1), (zid + 1) * (ny + 1))
    id1 = slice((zid + 1) * (ny + 1), (zid + 2) * (ny + 1))
    T = np.zeros((len(data.freqs), data.rxLoc.shape[0]), dtype=complex)
    for f, freq in enumerate(data.freqs):
        Ex01 = np.stack([fwd.exTE[id0, f], fwd.exTE[id1, f]], axis=1)
        T[f] = tipper_te(2 * np.pi * freq, rx, Ex01)[0]
    return T


def forward(mesh, data, sigma, keep=None, bc_fixed=None):
    """(pred in the masked table order, forward fields with both modes); keep / bc_fixed: the oracle's hooks (Dirichlet
    values recorded / held at another model's)."""
    _setup(mesh, sigma)
    ii, it, sub = split(data)
    nF, nR, nC = len(data.freqs), data.rxLoc.shape[0], len(data.dataComp)
    ni = n_imp(data)
    if sub is not None and sub.compTE and sub.compTM:
        subAll = copy.copy(sub)
        subAll.dataID = np.ones(nF * nR * ni, dtype=bool)
        pI, fwd = O.MT2DFwdSolver(mesh, subAll, keep=keep, bc_fixed=bc_fixed)
    else:
        _, fwd = O.MT2DFwdSolver(mesh, full_impedance(data), keep=keep, bc_fixed=bc_fixed)
        pI = None
        if sub is not None:
            subAll = copy.copy(sub)
            subAll.dataID = np.ones(nF * nR * ni, dtype=bool)
            pI, _ = O.MT2DFwdSolver(mesh, subAll, bc_fixed=bc_fixed)
    T = tipper_table(mesh, data, fwd)
    cols = []
    if pI is not None:
        cols.append(np.asarray(pI, dtype=complex).reshape(nF, nR, ni))
    for c in data.dataComp[ni:]:
        cols.append({"TZY": T, "RealTZY": T.real + 0j, "ImagTZY": T.imag + 0j}[c][:, :, None])
    table = np.concatenate(cols, axis=2).reshape(-1)
    pred = table[np.asarray(data.dataID, dtype=bool)]
    if data.dataType != "Impedance":
        pred = pred.real.copy()
    return pred, fwd


# ---------------------------------------------------------------------------------------------------------- J, gradient
def tipper_jacobian(mesh, data, sigma, activeIdx, fwd=None):
    """Complex rows dT/dsigma (active cells) of the tipper data, in data order (rows of the other data: zero)."""
    if fwd is None:
        _, fwd = forward(mesh, data, sigma)
    _setup(mesh, sigma)
    _, it, _ = split(data)
    J = np.zeros((len(data.rxID), len(activeIdx)), dtype=complex)
    if len(it):
        with tipper_rows_as_te():
            J[it] = O.compJacMat(mesh, as_zxy(data, it), activeIdx, fwd)
    return J


def tipper_row_values(data, Jt):
    """J's rows as the library returns them: complex for TZY, Re / Im for RealTZY / ImagTZY."""
    ni = n_imp(data)
    out = Jt.copy()
    for k, d in enumerate(data.dtID):
        if d > ni:
            c = data.dataComp[d - 1]
            if c == "RealTZY":
                out[k] = out[k].real
            elif c == "ImagTZY":
                out[k] = out[k].imag
    return out


def gradient(mesh, data, inv, m):
    """(pred, misfit, d misfit / d m) of a data set with tipper components, m = ln(sigma) on the active cells."""
    sigma = sigma_of(inv, m)
    pred, fwd = forward(mesh, data, sigma)
    r = inv.dataW * (pred - inv.obsData)
    misfit = 0.5 * float(np.sum(np.abs(r) ** 2))
    wr = inv.dataW * r
    ii, it, sub = split(data)
    g = np.zeros(len(m))
    if sub is not None and len(ii):
        invS = copy.copy(inv)
        invS.obsData, invS.dataW = inv.obsData[ii], inv.dataW[ii]
        invS.strModel = np.asarray(m, dtype=float).copy()
        meshS = copy.deepcopy(mesh)
        _, _, gI = O.compDataGradient(meshS, sub, invS, HMCPrior(), False)
        g = g + gI
    if len(it):
        _setup(mesh, sigma)
        if data.dataType == "Impedance":
            with tipper_rows_as_te():
                gT = O.compJacTMatVec(fwd.exTE, fwd.hxTM, wr[it], mesh, as_zxy(data, it), inv.activeIdx,
                                      fwd.AinvTE, fwd.AinvTM, False)
        else:
            J = tipper_jacobian(mesh, data, sigma, inv.activeIdx, fwd)[it]
            ni = n_imp(data)
            gT = np.zeros(len(m))
            for k, p in enumerate(it):
                c = data.dataComp[data.dtID[p] - 1]
                gT += (J[k].real if c == "RealTZY" else J[k].imag) * wr[p].real
        g = g + np.exp(m) * gT
    return pred, misfit, g


# ---------------------------------------------------------------------------------------------------------- problems
def tipper_problem(name, family="Impedance", with_impedance=True, mesh=None, rx_y=None, freqs=None):
    """(mesh, data, inv, m): config `name` (or the given mesh / receivers / frequencies) with a tipper layout, the start
    model of the tests, and observations = the reference's prediction at m perturbed by a few per cent (deterministic)."""
    if mesh is None:
        mesh, dz, _ = S.make_config(name)
        rx_y, freqs = dz.rxLoc[:, 0], dz.freqs
    data = S.make_tipper_layout(freqs, rx_y, family=family, with_impedance=with_impedance)
    ny, nz = mesh.gridSize
    nair = len(mesh.airLayer)
    mesh.sigma = np.concatenate([np.full(ny * nair, S.SIG_AIR), np.full(ny * (nz - nair), 0.01)])
    n = len(data.rxID)
    inv = I.setupInverseDataModel(mesh, [S.SIG_AIR], 0.0, 0.0, np.zeros(n, dtype=complex if family == "Impedance" else float),
                                  np.ones(n))
    m = S.rough_state(len(inv.strModel))
    pred, _ = forward(copy.deepcopy(mesh), data, sigma_of(inv, m))
    rng = np.random.default_rng(7)
    # (errors: 5 % of |pred| with a floor of 0.5 % of the largest datum -- without a floor the weights of tipper data near zero
    #  amplify the solver's error in T without bound)
    amp = np.abs(pred) + 0.1 * np.abs(pred).max()
    if family == "Impedance":
        obs = pred + 0.05 * amp * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    else:
        obs = pred + 0.05 * amp * rng.standard_normal(n)
    err = 0.05 * amp
    inv = I.setupInverseDataModel(mesh, [S.SIG_AIR], 0.0, 0.0, obs, err)
    return mesh, data, inv, m
