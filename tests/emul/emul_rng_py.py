"""ctypes front-end of the TEST-ONLY host instantiation of the random-number item functions (tests/emul/emul_rng.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_rng.so")
c_double_p = C.POINTER(C.c_double)
c_uint32_p = C.POINTER(C.c_uint32)


def build(force=False):
    src = os.path.join(HERE, "emul_rng.cpp")
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
        _lib.emulrng_philox.argtypes = [c_uint32_p] * 3
        _lib.emulrng_philox.restype = None
        _lib.emulrng_u52.argtypes = [C.c_uint32, C.c_uint32]
        _lib.emulrng_u52.restype = C.c_double
        _lib.emulrng_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int64, C.c_int64, c_double_p]
        _lib.emulrng_normals.restype = None
        _lib.emulrng_scalars.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_int32), c_double_p]
        _lib.emulrng_scalars.restype = None
        _lib.emulrng_momentum.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int64] + [c_double_p] * 6
        _lib.emulrng_momentum.restype = None
    return _lib


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def philox(c, k):
    cc, kk, out = (C.c_uint32 * 4)(*c), (C.c_uint32 * 2)(*k), (C.c_uint32 * 4)()
    lib().emulrng_philox(cc, kk, out)
    return tuple(int(x) for x in out)


def u52(hi, lo):
    return float(lib().emulrng_u52(hi, lo))


def normals(seed, stream, t, n, a0=0):
    z = np.empty(n)
    lib().emulrng_normals(seed, stream, t, a0, n, _dp(z))
    return z


def scalars(seed, stream, t, Lmin, Lmax):
    L, u = C.c_int32(), C.c_double()
    lib().emulrng_scalars(seed, stream, t, Lmin, Lmax, C.byref(L), C.byref(u))
    return int(L.value), float(u.value)


def momentum(seed, stream, t, invM):
    """(clipped normals, p drawn, p fed, terms drawn, terms fed) for the diagonal mass invM"""
    invM = np.ascontiguousarray(invM, dtype=np.float64)
    out = [np.empty(len(invM)) for _ in range(5)]
    lib().emulrng_momentum(seed, stream, t, len(invM), _dp(invM), *[_dp(a) for a in out])
    return out
