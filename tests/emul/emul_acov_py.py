"""ctypes front-end of the TEST-ONLY host instantiation of the chain's autocovariance item functions (tests/emul/emul_acov.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_acov.so")
c_double_p = C.POINTER(C.c_double)


def build(force=False):
    src = os.path.join(HERE, "emul_acov.cpp")
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
        vp = C.c_void_p
        _lib.emulacov_accumulate.argtypes = [C.c_int64, C.c_int64, c_double_p, C.c_int64, vp, C.c_int32, vp, vp, vp, vp, vp]
        _lib.emulacov_accumulate.restype = None
        _lib.emulacov_out.argtypes = [C.c_int64, C.c_int32, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
        _lib.emulacov_out.restype = None
        _lib.emulacov_ess.argtypes = [C.c_int64, C.c_int32, C.c_int64, vp, vp, vp, vp]
        _lib.emulacov_ess.restype = None
    return _lib


def maxlag():
    return int(lib().emulacov_maxlag())


def run_length():
    return int(lib().emulacov_run())


def accumulate(samples, targets, K):
    """samples [nparam, nsamples] (columns = committed models), targets or None (every cell) -> the device's state as a dict:
    x0[ntarget], tot[ntarget], S, H, ring [K + 1, ntarget]"""
    cols = np.ascontiguousarray(np.asarray(samples, dtype=np.float64).T)
    ns, n = cols.shape
    t = None if targets is None else np.ascontiguousarray(targets, dtype=np.int64)
    nt = n if t is None else len(t)
    st = {"x0": np.zeros(nt), "tot": np.zeros(nt), "S": np.zeros((K + 1, nt)), "H": np.zeros((K + 1, nt)), "ring": np.zeros((K + 1, nt))}
    lib().emulacov_accumulate(n, ns, cols.ctypes.data_as(c_double_p), nt, None if t is None else t.ctypes.data, int(K),
                              *(st[k].ctypes.data for k in ("x0", "tot", "S", "H", "ring")))
    return st


def readout(st, N):
    """(mean[ntarget], acov[K + 1, ntarget]) of a state after N commits"""
    K, nt = st["S"].shape[0] - 1, st["S"].shape[1]
    mean, acov = np.empty(nt), np.empty((K + 1, nt))
    lib().emulacov_out(nt, K, int(N), *(st[k].ctypes.data for k in ("x0", "tot", "S", "H", "ring")), mean.ctypes.data, acov.ctypes.data)
    return mean, acov


def ess(acov, N):
    """(tau, ess, window) of acov[K + 1, ntarget]"""
    acov = np.ascontiguousarray(acov, dtype=np.float64)
    K, nt = acov.shape[0] - 1, acov.shape[1]
    tau, e, w = np.empty(nt), np.empty(nt), np.empty(nt, dtype=np.int32)
    lib().emulacov_ess(nt, K, int(N), acov.ctypes.data, tau.ctypes.data, e.ctypes.data, w.ctypes.data)
    return tau, e, w
