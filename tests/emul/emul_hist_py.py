"""ctypes front-end of the TEST-ONLY host instantiation of the chain's histogram item functions (tests/emul/emul_hist.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_hist.so")
c_double_p = C.POINTER(C.c_double)


def build(force=False):
    src = os.path.join(HERE, "emul_hist.cpp")
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
        _lib.emulhist_bins.argtypes = [C.c_int64, c_double_p, C.c_int32, C.c_double, C.c_double, vp]
        _lib.emulhist_bins.restype = None
        _lib.emulhist_accumulate.argtypes = [C.c_int64, C.c_int64, c_double_p, C.c_int64, vp, C.c_int32, C.c_double, C.c_double, vp]
        _lib.emulhist_accumulate.restype = None
        _lib.emulhist_quantiles.argtypes = [C.c_int64, C.c_int32, vp, C.c_int64, C.c_double, C.c_double, C.c_int32, c_double_p, vp, vp]
        _lib.emulhist_quantiles.restype = None
    return _lib


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def maxbins():
    return int(lib().emulhist_maxbins())


def bins(m, nbins, lo, hi):
    """the bin of every value of m"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    out = np.empty(len(m), dtype=np.int32)
    lib().emulhist_bins(len(m), _dp(m), int(nbins), float(lo), float(hi), out.ctypes.data)
    return out


def accumulate(samples, targets, nbins, lo, hi):
    """samples [nparam, nsamples] (columns = committed models) -> counts[ntarget, nbins] uint32"""
    cols = np.ascontiguousarray(np.asarray(samples, dtype=np.float64).T)
    ns, n = cols.shape
    t = np.ascontiguousarray(targets, dtype=np.int64)
    counts = np.empty((len(t), int(nbins)), dtype=np.uint32)
    lib().emulhist_accumulate(n, ns, _dp(cols), len(t), t.ctypes.data, int(nbins), float(lo), float(hi), counts.ctypes.data)
    return counts


def quantiles(counts, count, lo, hi, q):
    """(values[nq, ntarget], bins[nq, ntarget]) of target-major counts"""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    nt, nb = counts.shape
    out, b = np.empty((len(q), nt)), np.empty((len(q), nt), dtype=np.int32)
    lib().emulhist_quantiles(nt, nb, counts.ctypes.data, int(count), float(lo), float(hi), len(q), _dp(q), out.ctypes.data, b.ctypes.data)
    return out, b
