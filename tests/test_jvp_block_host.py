"""The block Jacobian products' host side (hmcmt_jvp_block / hmcmt_jtvp_block / hmcmt_gn_hessvec_block and their _device twins):
declarations, exports and prototypes against the ctypes argtypes and the Julia ccalls, the argument checks that need no device,
the Python wrappers' shape and dtype checks, and the premise of the solver route -- a problem whose frequency list is repeated k
times has, per repeated system, the operator and the pivots of the original system (host instantiation, tests/emul/emul.cpp).

The products' kernels (kernels_jvp.h: one family, launched with the count of directions) add no item function and change none:
they call the item functions of hmcmt_items.h on a View whose pointers are moved to a direction (dir_view), and the two dBC
contractions (k_dbc, k_contract) repeat the item functions' arithmetic per direction.  Neither has a host instantiation: the index
mapping of dir_view / blk_sv and the contractions are held to the oracle and to the single entry points only on the GPU
(tests/test_gpu_jvp.py, tests/test_gpu_jvp_block.py); the mapping sv(j, s) itself is the one checked here."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd import invsetup as I
from hmcmt2d_amd import synthetic as S
from tests.helpers import make_problem
from tests.test_abi import _c_prototypes, _JL_OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("hmcmt_jvp_block", "hmcmt_jtvp_block", "hmcmt_gn_hessvec_block")
SYMBOLS = tuple(n for b in BASES for n in (b, b + "_device"))


def test_symbols_are_declared_exported_and_listed():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hmcmt.h")).read(), flags=re.S)
    so = C.CDLL(L.build_library())
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in include/hmcmt.h"
        assert hasattr(so, name), f"{name} not exported"
        assert name in L.PRODUCT_SYMBOLS
    assert int(re.search(r"#define\s+HMCMT_BLOCK_MAX\s+(\d+)", text).group(1)) == L.BLOCK_MAX >= 16


def test_prototypes_argtypes_and_ccalls_agree():
    """header prototype == ctypes argtypes == Julia ccall, argument by argument (tests/test_abi.py's mechanics)."""
    protos = _c_prototypes()
    lib = L.load_library()
    src = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    vp, dp, st = C.c_void_p, L.c_double_p, C.POINTER(L.Stats)
    for name in SYMBOLS:
        ret, params = protos[name]
        dev = name.endswith("_device")
        assert ret == "int"
        assert [t for t, _ in params] == ["hmcmt_ctx*", "constdouble*", "int32_t", "int32_t", "double*", "hmcmt_stats*"], (name, params)
        assert [n for _, n in params][2:4] == ["nvec", "wrt"]
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == ([vp, vp, C.c_int32, C.c_int32, vp, st] if dev else [vp, dp, C.c_int32, C.c_int32, dp, st]), name
        m = re.search(r"ccall\(\(:%s, libhmcmt\),\s*(\w+),\s*\(" % name, src)
        assert m, f"{name}: no ccall in julia/HMCMTHip.jl"
        i = j = m.end(); depth = 1
        while depth:
            depth += src[j] == "("; depth -= src[j] == ")"; j += 1
        types = [t.strip() for t in re.split(r",(?![^{]*\})", src[i:j - 1]) if t.strip()]
        assert m.group(1) == "Cint" and len(types) == len(params), (name, types)
        for jt, (ct, pname) in zip(types, params):
            assert jt in _JL_OK[ct], f"{name}: {pname} is {ct} in C, {jt} in the ccall"


def test_null_context_is_einval():
    lib = L.load_library()
    x = np.zeros(8)
    for b in BASES:
        assert getattr(lib, b)(None, L._dp(x), 1, 0, L._dp(x), None) == -1
        assert getattr(lib, b + "_device")(None, None, 1, 0, None, None) == -1


def test_mirrors_exist():
    import hmcmt2d_amd
    from hmcmt2d_amd import sampler
    assert hmcmt2d_amd.compJacMatMat is sampler.compJacMatMat and hmcmt2d_amd.compJacTMatMat is sampler.compJacTMatMat
    for name in ("jvp_block", "jtvp_block", "gn_hessvec_block", "jvp_block_device", "jtvp_block_device", "gn_hessvec_block_device"):
        assert callable(getattr(L.HipContext, name))


def test_wrappers_reject_wrong_shapes_and_dtypes_without_a_device():
    chk = L.HipContext.block_input
    ok = chk(np.ones((3, 5), dtype=np.float32), 5, "jvp")
    assert ok.dtype == np.float64 and ok.shape == (3, 5) and ok.flags.c_contiguous
    assert chk(np.ones((7, 3)).T, 7, "jvp").flags.c_contiguous
    assert chk(np.ones((2, 4)), 4, "jtvp", complex_in=True).dtype == np.complex128
    with pytest.raises(ValueError, match="use jvp"):                   # 1-D: the single-direction method
        chk(np.ones(5), 5, "jvp")
    with pytest.raises(ValueError, match="use compJacTMatVec"):
        chk(np.ones(4), 4, "compJacTMatVec", complex_in=True)
    for bad in (np.ones((3, 4)), np.ones((2, 3, 5)), np.ones((0, 5)), np.ones((L.BLOCK_MAX + 1, 5))):
        with pytest.raises(ValueError):
            chk(bad, 5, "jvp")
    with pytest.raises(TypeError):                                     # a complex V would lose its imaginary part
        chk(np.ones((2, 5), dtype=np.complex128), 5, "jvp")
    with pytest.raises(TypeError):
        chk(np.array([["a"] * 5] * 2), 5, "jvp")
    with pytest.raises(TypeError):
        chk(np.ones((2, 5), dtype=object), 5, "jvp")


def _repeated(k):
    """the tiny problem, and the same with its frequency list repeated k times (every datum present, the same data per copy)"""
    mesh, data, inv, m = make_problem("tiny")
    rx = data.rxLoc[:, 0]
    dk = S.make_data_layout(np.tile(data.freqs, k), rx)
    nF, per = len(data.freqs), len(data.rxID) // len(data.freqs)
    obs, err = np.asarray(inv.obsData), 1.0 / np.asarray(inv.dataW)
    assert len(obs) == nF * per
    mk = copy.deepcopy(mesh)
    mk.sigma = mesh.sigma.copy()
    invk = I.setupInverseDataModel(mk, [S.SIG_AIR], 0.0, 0.0, np.tile(obs, k), np.tile(err, k))
    return (mesh, data, inv, m), (mk, dk, invk, m)


@pytest.mark.parametrize("k", [2, 3])
def test_repeated_frequency_list_repeats_operator_and_pivots(k):
    """The premise of the block solve: with the frequency list repeated k times, virtual system sv(j, s) -- j nFreq + s for TE,
    k nFreq + j nFreq + (s - nFreq) for TM -- has the stencil (A p), the FDM preconditioner (the tridiagonal pivots) and the
    smoothed preconditioner of system s, bit for bit, and the forward fields repeat."""
    from tests.emul.emul_py import Emul
    (mesh, data, inv, m), (mk, dk, invk, _) = _repeated(k)
    e1, ek = Emul(mesh, data, inv), Emul(mk, dk, invk)
    e1.grad(m, want_grad=False)
    ek.grad(m, want_grad=False)
    S1, nF = e1.S, e1.S // 2
    assert ek.S == k * S1 and (ek.NYP, ek.NZP) == (e1.NYP, e1.NZP)
    vs = e1.NYP * e1.NZP
    sv = lambda j, s: j * nF + s if s < nF else k * nF + j * nF + (s - nF)
    rng = np.random.default_rng(31)
    x1 = rng.standard_normal(S1 * vs) + 1j * rng.standard_normal(S1 * vs)
    xk = np.empty(k * S1 * vs, dtype=np.complex128)
    for j in range(k):
        for s in range(S1):
            xk[sv(j, s) * vs:(sv(j, s) + 1) * vs] = x1[s * vs:(s + 1) * vs]
    X1, Xk = e1.get("X"), ek.get("X")
    for which in ("spmv", "fdm", "jacobi", "fdmj"):
        y1, yk = e1.apply(which, x1), ek.apply(which, xk)
        assert np.abs(y1).max() > 0
        for j in range(k):
            for s in range(S1):
                a, b = yk[sv(j, s) * vs:(sv(j, s) + 1) * vs], y1[s * vs:(s + 1) * vs]
                assert np.array_equal(a.view(np.float64), b.view(np.float64)), (which, j, s)
    for j in range(k):
        for s in range(S1):
            assert np.array_equal(Xk[sv(j, s) * vs:(sv(j, s) + 1) * vs].view(np.float64), X1[s * vs:(s + 1) * vs].view(np.float64))
    e1.close(); ek.close()
