"""The explicit Jacobian's host side (hmcmt_jacobian / hmcmt_jacobian_device / hmcmt_sensitivity): the C declarations and exports,
the argument check that needs no device, the Python mirrors of the reference names, and the Rho_Pha reference Jacobian the GPU
tests compare against (tests/test_gpu_jacobian.py), itself checked against central differences of the oracle's forward."""
import ctypes
import os
import re

import numpy as np
import pytest

from hmcmt2d_amd import lib as L, synthetic as S, invsetup as I
from oracle import hmcmt_oracle as O
from tests.helpers import oracle_eval, rhophase_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAC_SYMBOLS = ("hmcmt_jacobian", "hmcmt_jacobian_device", "hmcmt_sensitivity")


def oracle_jacobian(mesh, data, inv, m):
    """oracle.compJacMat (DataType Impedance) at model m: (nData, nAC) complex, d Z / d sigma, data order."""
    oracle_eval(mesh, data, inv, m)                       # (sets mesh.sigma to m's conductivities)
    fwd = O.MT2DFwdSolver(mesh, data)[1]
    return O.compJacMat(mesh, data, inv.activeIdx, fwd)


def impedance_twin(mesh, data):
    """The Impedance data set (ZXY + ZYX, all data) on the frequencies and receivers of `data`, with its InvDataModel."""
    twin = S.make_data_layout(data.freqs, data.rxLoc[:, 0], data.rxLoc[0, 1])
    n = len(twin.rxID)
    return twin, I.setupInverseDataModel(mesh, [S.SIG_AIR], 0.0, 0.0, np.zeros(n, complex), np.ones(n))


def rhophase_rows(data, twin, Z, dZ):
    """Chain rule from the twin's impedances Z and their derivatives dZ (rows of the twin) to the rows of the Rho_Pha data set:
    rho_a (2/(w mu0)) Re(conj(Z) dZ), phase in degrees (180/pi) Im(conj(Z) dZ)/|Z|^2."""
    index = {(int(f), int(r), int(d)): k for k, (f, r, d) in enumerate(zip(twin.freqID, twin.rxID, twin.dtID))}
    J = np.empty((len(data.rxID),) + dZ.shape[1:])
    for k, (f, r, d) in enumerate(zip(data.freqID, data.rxID, data.dtID)):
        comp = data.dataComp[d - 1]
        t = index[(int(f), int(r), 1 if "XY" in comp else 2)]
        c = np.conj(Z[t]) * dZ[t]
        omega = 2 * np.pi * data.freqs[f - 1]
        J[k] = (2.0 / (omega * O.MU0)) * c.real if comp.startswith("Rho") else (180.0 / np.pi) * c.imag / abs(Z[t]) ** 2
    return J


def rhophase_jacobian(mesh, data, m):
    """Reference Jacobian of a Rho_Pha data set: rhophase_rows on oracle.compJacMat of its Impedance twin.  (nData, nAC) real."""
    twin, inv = impedance_twin(mesh, data)
    Jz = oracle_jacobian(mesh, twin, inv, m)
    Z, _ = O.MT2DFwdSolver(mesh, twin)
    return rhophase_rows(data, twin, Z, Jz)


def test_jacobian_symbols_are_declared_exported_and_listed():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hmcmt.h")).read(), flags=re.S)
    so = ctypes.CDLL(L.build_library())
    for name in JAC_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in include/hmcmt.h"
        assert hasattr(so, name), f"{name} not exported"
        assert name in L.PRODUCT_SYMBOLS
    assert re.search(r"#define\s+HMCMT_JAC_WRT_SIGMA\s+0\b", text) and re.search(r"#define\s+HMCMT_JAC_WRT_LNSIGMA\s+1\b", text)


def test_jacobian_null_context_is_einval():
    lib = L.load_library()
    m = np.zeros(4)
    J = np.zeros(16)
    assert lib.hmcmt_jacobian(None, L._dp(m), 0, 1, 0, L._dp(J), None) == -1
    assert lib.hmcmt_jacobian_device(None, None, 0, 1, 0, None, None) == -1
    assert lib.hmcmt_sensitivity(None, L._dp(m), 0, L._dp(J), None) == -1


def test_reference_name_mirrors_exist():
    import hmcmt2d_amd
    from hmcmt2d_amd import sampler
    assert hmcmt2d_amd.compJacMat is sampler.compJacMat and hmcmt2d_amd.compJacTMat is sampler.compJacTMat
    assert callable(L.HipContext.jacobian) and callable(L.HipContext.sensitivity)


def test_rhophase_reference_jacobian_matches_central_differences():
    """The chain rule of rhophase_jacobian against central differences of the oracle's Rho_Pha forward on interior earth cells
    of tiny, with the impedance derivative taken by the same central differences: the oracle's compJacMat itself differs from
    differences of its forward by ~1e-4 there (the reference's boundary-derivative terms are approximations: SURVEY section 4
    item 4, tests/test_oracle_kat.py), so that part is compared on its own, and only loosely."""
    mesh, data, inv, m, _ = rhophase_problem("tiny")
    J = rhophase_jacobian(mesh, data, m)
    twin, _ = impedance_twin(mesh, data)
    ny = mesh.gridSize[0]
    nair = len(mesh.airLayer)
    act = list(inv.activeIdx)
    sig = inv.bgModel.copy()
    sig[inv.activeIdx] += np.exp(m)
    mesh.sigma = sig
    Z, _ = O.MT2DFwdSolver(mesh, twin)
    for cell in ((nair + 1) * ny + 5, (nair + 2) * ny + 6, (nair + 1) * ny + 4):
        a = act.index(cell)
        h = 1e-6 * sig[cell]
        rp, zz = [], []
        for dh in (h, -h):
            s2 = sig.copy(); s2[cell] += dh
            mesh.sigma = s2
            rp.append(np.real(O.MT2DFwdSolver(mesh, data)[0]))
            zz.append(O.MT2DFwdSolver(mesh, twin)[0])
        fd = (rp[0] - rp[1]) / (2 * h)
        chain = rhophase_rows(data, twin, Z, ((zz[0] - zz[1]) / (2 * h))[:, None])[:, 0]
        assert np.abs(chain - fd).max() / np.abs(fd).max() < 1e-6, cell
        assert np.abs(J[:, a] - fd).max() / np.abs(fd).max() < 3e-2, cell


@pytest.mark.parametrize("wrt", ["x", 2])
def test_python_mirror_rejects_an_unknown_wrt(wrt):
    with pytest.raises(ValueError):
        L.HipContext._wrt(L.HipContext, wrt)
