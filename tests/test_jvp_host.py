"""The matrix-free Jacobian products' host side (hmcmt_linearize / hmcmt_jvp / hmcmt_jtvp / hmcmt_gn_hessvec): the C declarations
and exports, the argument check that needs no device, the Python mirrors, and the tangent-linear arithmetic and the free-u
adjoint of hmcmt_items.h, instantiated on the host (tests/emul/emul_jvp.cpp) and held against the oracle's compJacMat.

Error measure of a row k of J v: |(J v)_k - (Jo v)_k| / sum_a |Jo_ka| |v_a| -- the size the sum would have without
cancellation -- and of an entry a of J^T u: |.| / sum_k |Jo_ka| |u_k|.  The emulation is fp64 throughout and solves to 1e-12, so
what is left is the round-off of the two routes and the solves' stopping error."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from tests import tipper_ref as TR
from tests.helpers import make_problem, ragged_problem, rhophase_problem
from tests.test_jacobian_host import oracle_jacobian, rhophase_jacobian
from tests.emul.emul_jvp_py import EmulJvp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hmcmt_linearize", "hmcmt_jvp", "hmcmt_jtvp", "hmcmt_gn_hessvec")

# measured maxima (jvp, jtvp) of the error measure above per case of test_host_products_equal_the_oracle, on the build machine
# (g++ -O2, x86-64); asserted: ten times them, case by case (no looser anywhere than ten times the overall maximum)
MEASURED = {"tiny": (1.2e-10, 2.9e-10), "cfg2": (4.6e-1, 1.8e-1), "ragged": (1.6e-8, 2.6e-9), "rhophase": (2.4e-8, 8.6e-8),
            "tipper": (1.7e-11, 3.2e-11)}
SHALLOW_TOL, DEEP_TOL = 1e-7, 2e-6          # tests/test_gpu_jacobian.py


def test_symbols_are_declared_exported_and_listed():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hmcmt.h")).read(), flags=re.S)
    so = ctypes.CDLL(L.build_library())
    for base in SYMBOLS:
        for name in (base, base + "_device"):
            assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in include/hmcmt.h"
            assert hasattr(so, name), f"{name} not exported"
            assert name in L.PRODUCT_SYMBOLS


def test_null_context_is_einval():
    lib = L.load_library()
    x = np.zeros(8)
    assert lib.hmcmt_linearize(None, L._dp(x)) == -1
    assert lib.hmcmt_linearize_device(None, None) == -1
    for base in SYMBOLS[1:]:
        assert getattr(lib, base)(None, L._dp(x), 0, L._dp(x), None) == -1
        assert getattr(lib, base + "_device")(None, None, 0, None, None) == -1


def test_mirrors_exist():
    import hmcmt2d_amd
    from hmcmt2d_amd import sampler
    assert hmcmt2d_amd.compJacMatVec is sampler.compJacMatVec and hmcmt2d_amd.compJacTMatVec is sampler.compJacTMatVec
    for name in ("linearize", "jvp", "jtvp", "gn_hessvec", "linearize_device", "jvp_device", "jtvp_device", "gn_hessvec_device"):
        assert callable(getattr(L.HipContext, name))


def _case(name):
    """(mesh, data, inv, m, Jo): Jo in the library's row convention (complex, or real rows for real data)."""
    if name == "rhophase":
        mesh, data, inv, m, _ = rhophase_problem("tiny")
        return mesh, data, inv, m, rhophase_jacobian(mesh, data, m)
    if name == "tipper":
        mesh, data, inv, m = TR.tipper_problem("tiny", "Impedance", with_impedance=False)
        Jo = TR.tipper_row_values(data, TR.tipper_jacobian(copy.deepcopy(mesh), data, TR.sigma_of(inv, m), inv.activeIdx))
        return mesh, data, inv, m, Jo
    mesh, data, inv, m = ragged_problem(23, 17, 3, 3, 3, 4) if name == "ragged" else make_problem(name)
    return mesh, data, inv, m, oracle_jacobian(mesh, data, inv, m)


def _unit_cells(mesh, inv):
    """active indices of a side-column cell, a bottom-row cell and a receiver-layer cell: where the tangent of the side values,
    of the mean profile and the Q-term act alone"""
    ny, nt = mesh.gridSize
    nair = len(mesh.airLayer)
    act = list(inv.activeIdx)
    want = [(nair + 2) * ny + 0, (nt - 1) * ny + ny // 2, nair * ny + ny // 2]
    return [act.index(c) for c in want]


@pytest.mark.parametrize("name", ["tiny", "cfg2", "ragged", "rhophase", "tipper"])
def test_host_products_equal_the_oracle(name):
    """jvp(v) against Jo @ v and jtvp(u) against Re(Jo^T conj(u)), Jo = oracle.compJacMat (rhophase: its chain rule, tipper:
    tests/tipper_ref.py), for seeded random v, u and unit vectors (cells: side column, bottom row, receiver layer), both wrt.
    Measured maxima of the error measure of this file's docstring, (jvp, jtvp):
        tiny 1.1e-10 / 2.8e-10, ragged 1.5e-8 / 2.5e-9, rhophase 2.4e-8 / 8.6e-8, tipper 1.7e-11 / 3.1e-11, cfg2 4.5e-1 / 1.7e-1.
    They are not round-off everywhere: with a unit vector the scale sum_a |Jo_ka| |v_a| is the single entry |Jo_ka|, and the
    oracle's entries for bottom-row cells at the high frequencies are its own rounding noise (cfg2: 3.5e-26 where the row's maximum
    is 1e-5; the reference's bottom-boundary sensitivity row, MT1DSensitivity.jl:145-155) -- 0.45 of such an entry is the maximum on
    cfg2 (random v there: 2.4e-7).  So the same differences are also held to the GPU suite's ceiling, which scales with the row's
    maximum: |d|_k <= (1e-7 |v_shallow|_1 + 2e-6 |v_deep|_1) max_a |Jo_ka|; measured ratio to it: tiny 2.9e-4, cfg2 1.1e-1, ragged
    7.4e-4, rhophase 1.5e-2, tipper 2.3e-6."""
    mesh, data, inv, m, Jo = _case(name)
    em = EmulJvp(mesh, data, inv)
    em.linearize(m)
    rng = np.random.default_rng(5)
    nD, nA = Jo.shape
    real = not np.iscomplexobj(Jo)
    vs = [rng.standard_normal(nA)]
    for a in _unit_cells(mesh, inv):
        e = np.zeros(nA); e[a] = 1.0
        vs.append(e)
    us = [rng.standard_normal(nD) if real else rng.standard_normal(nD) + 1j * rng.standard_normal(nD)]
    for k in (0, nD // 2, nD - 1):
        e = np.zeros(nD, dtype=float if real else complex); e[k] = 1.0 if real else 1.0 - 0.5j
        us.append(e)
    ny, nt = mesh.gridSize
    deep = (inv.activeIdx // ny) >= nt - 5
    wj = wt = wc = 0.0
    for wrt, sc in (("sigma", np.ones(nA)), ("lnsigma", np.exp(m))):
        Jw = Jo * sc[None, :]
        for v in vs:
            got = em.jvp(v, wrt=wrt)
            d = np.abs(got - Jw @ v)
            wj = max(wj, float((d / (np.abs(Jw) @ np.abs(v))).max()))
            ceil = (SHALLOW_TOL * np.abs(v[~deep]).sum() + DEEP_TOL * np.abs(v[deep]).sum()) * np.abs(Jw).max(axis=1)
            wc = max(wc, float((d / ceil).max()))
        for u in us:
            got = em.jtvp(u, wrt=wrt)
            d = np.abs(got - np.real(Jw.T @ np.conj(u)))
            wt = max(wt, float((d / (np.abs(Jw).T @ np.abs(u))).max()))
    em.close()
    print(f"{name}: jvp {wj:.3e} jtvp {wt:.3e} jvp/ceiling {wc:.3e}")
    assert wj < 10 * MEASURED[name][0] and wt < 10 * MEASURED[name][1], (wj, wt)
    assert wc < 1.0, wc
