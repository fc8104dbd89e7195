"""ctypes front-end of the TEST-ONLY host instantiation of the warm-up adaptation's item functions (tests/emul/emul_adapt.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_adapt.so")
c_double_p = C.POINTER(C.c_double)
c_int64_p = C.POINTER(C.c_int64)


def build(force=False):
    src = os.path.join(HERE, "emul_adapt.cpp")
    hdrs = [os.path.join(HERE, "..", "..", "hmcmt2d_amd", "csrc", h) for h in ("hmcmt_math.h", "hmcmt_items.h")]
    newest = max(os.path.getmtime(f) for f in [src] + hdrs)
    if force or not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", SO])
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emuladapt_da.argtypes = [C.c_int64, c_double_p] + [C.c_double] * 7 + [c_double_p] * 3
        _lib.emuladapt_da.restype = None
        _lib.emuladapt_windows.argtypes = [C.c_int64] * 4 + [c_int64_p, C.c_int64]
        _lib.emuladapt_windows.restype = C.c_int64
        _lib.emuladapt_mass.argtypes = [C.c_int64, C.c_int64, c_double_p, c_double_p]
        _lib.emuladapt_mass.restype = None
    return _lib


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def dual_averaging(alpha, dt0, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, dt_min=0.0, dt_max=0.0):
    """(x, x_bar, dt) behind each of len(alpha) updates from a restart at dt0"""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    x, x_bar, dt = np.empty_like(alpha), np.empty_like(alpha), np.empty_like(alpha)
    lib().emuladapt_da(len(alpha), _dp(alpha), dt0, delta, gamma, t0, kappa, dt_min, dt_max, _dp(x), _dp(x_bar), _dp(dt))
    return x, x_bar, dt


def window_ends(nwarmup, init, term, base):
    """The window ends as steps completed (0-based last step + 1)"""
    ends = np.zeros(64, dtype=np.int64)
    k = lib().emuladapt_windows(nwarmup, init, term, base, ends.ctypes.data_as(c_int64_p), len(ends))
    assert k <= len(ends)
    return [int(e) + 1 for e in ends[:k]]


def window_mass(samples):
    """samples [ncell, n] (columns = samples) -> diag(M^-1) of that window"""
    rows = np.ascontiguousarray(np.asarray(samples, dtype=np.float64).T)
    ns, n = rows.shape
    invM = np.empty(n)
    lib().emuladapt_mass(n, ns, _dp(rows), _dp(invM))
    return invM
