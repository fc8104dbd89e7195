"""ctypes front-end of the TEST-ONLY host instantiation of the HMC chain's item functions (tests/emul/emul_chain.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_chain.so")
c_double_p = C.POINTER(C.c_double)


def build(force=False):
    src = os.path.join(HERE, "emul_chain.cpp")
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
        _lib.emulchain_layout.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.emulchain_momentum.argtypes = [C.c_int64, c_double_p, c_double_p, c_double_p]
        _lib.emulchain_momentum.restype = C.c_double
        _lib.emulchain_clip.argtypes = [C.c_int64, c_double_p, c_double_p]
        _lib.emulchain_clip.restype = None
        _lib.emulchain_kinetic.argtypes = [C.c_int64, c_double_p, c_double_p, c_double_p]
        _lib.emulchain_kinetic.restype = C.c_double
        _lib.emulchain_welford.argtypes = [C.c_int64, C.c_int64, C.c_int64, c_double_p, c_double_p, c_double_p]
        _lib.emulchain_welford.restype = C.c_int64
    return _lib


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _vec(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def layout():
    """(partial sums, threads per workgroup) of the chain's reductions"""
    nb, nt = C.c_int(), C.c_int()
    lib().emulchain_layout(C.byref(nb), C.byref(nt))
    return nb.value, nt.value


def momentum(z, invM):
    """(p, K): p = clip(z, +-2.5) / sqrt(invM), K = 0.5 p' invM p by the two-stage sum"""
    z, invM = _vec(z), _vec(invM)
    p = np.empty_like(z)
    K = lib().emulchain_momentum(len(z), _dp(z), _dp(invM), _dp(p))
    return p, K


def clip(z):
    z = _vec(z)
    out = np.empty_like(z)
    lib().emulchain_clip(len(z), _dp(z), _dp(out))
    return out


def kinetic(p, x=None, invM=None):
    p = _vec(p)
    x = None if x is None else _vec(x)
    invM = None if invM is None else _vec(invM)
    return lib().emulchain_kinetic(len(p), _dp(p), None if x is None else _dp(x), None if invM is None else _dp(invM))


def welford(samples, burnin):
    """samples [nparam, nsamples] (columns = samples, as hmcmodel) -> (count, mean, m2) of the columns behind the burn-in"""
    cols = np.ascontiguousarray(np.asarray(samples, dtype=np.float64).T)
    ns, n = cols.shape
    mean, m2 = np.empty(n), np.empty(n)
    count = lib().emulchain_welford(n, ns, int(burnin), _dp(cols), _dp(mean), _dp(m2))
    return int(count), mean, m2
