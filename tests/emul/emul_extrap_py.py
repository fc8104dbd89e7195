"""ctypes front-end of the TEST-ONLY host instantiation of the initial-guess extrapolation's weights (tests/emul/emul_extrap.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_extrap.so")
c_double_p = C.POINTER(C.c_double)


def build(force=False):
    src = os.path.join(HERE, "emul_extrap.cpp")
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
        _lib.emulext_weights.argtypes = [c_double_p, c_double_p, C.c_int32, C.c_int32]
        _lib.emulext_call.argtypes = [C.c_int64, c_double_p, c_double_p, c_double_p, C.c_int32, C.c_int32, c_double_p]
    return _lib


def constants():
    """points (EXT_NP), state_len (EXT_PART), nsums (EXT_NS) of hmcmt_items.h"""
    L = lib()
    return {"points": int(L.emulext_points()), "state_len": int(L.emulext_state_len()), "nsums": int(L.emulext_nsums())}


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _read(ext, keep):
    return {"weights": ext[:6].copy(), "keep": int(keep), "count": int(ext[7]), "head": int(ext[8]), "model_head": int(ext[9]),
            "npoints": int(np.flatnonzero(ext[:6]).max() + 1) if ext[:6].any() else 0}


class State:
    """The device state of one solve kind -- the model ring and {weights, keep, count, heads} -- as hmcmt_create leaves it (zeros)."""

    def __init__(self, n, adjoint=False, cap=6):
        k = constants()
        self.n, self.adjoint, self.cap = int(n), int(bool(adjoint)), int(cap)
        self.hist = np.zeros((k["points"] + 1, self.n))
        self.ext = np.zeros(k["state_len"])
        self.sums = np.zeros(k["nsums"])

    def reset(self):
        """the memset of a cold start: weights, flag, count and heads; the ring keeps its stale models"""
        self.ext[:] = 0.0

    def call(self, m):
        m = np.ascontiguousarray(m, dtype=np.float64)
        assert m.shape == (self.n,)
        keep = lib().emulext_call(self.n, _dp(m), _dp(self.hist), _dp(self.ext), self.cap, self.adjoint, _dp(self.sums))
        assert keep == int(self.ext[6])
        return _read(self.ext, keep)


def weights_from_sums(a, count, adjoint=False, cap=6):
    """extrap_weights on given sums a[12] with `count` models in the history"""
    k = constants()
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == (k["nsums"],)
    ext = np.zeros(k["state_len"])
    ext[7] = count
    keep = lib().emulext_weights(_dp(a), _dp(ext), int(cap), int(bool(adjoint)))
    return _read(ext, keep)
