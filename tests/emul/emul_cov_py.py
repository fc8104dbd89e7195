"""ctypes front-end of the TEST-ONLY host instantiation of the chain's cross-moment item functions (tests/emul/emul_cov.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_cov.so")
c_double_p = C.POINTER(C.c_double)


def build(force=False):
    src = os.path.join(HERE, "emul_cov.cpp")
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
        _lib.emulcov_accumulate.argtypes = [C.c_int64, C.c_int64, C.c_int64, c_double_p, C.c_int64, vp, C.c_int32, vp, vp, vp, vp, vp,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int32, C.c_int32]
        _lib.emulcov_accumulate.restype = None
        _lib.emulcov_out.argtypes = [C.c_int64, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
        _lib.emulcov_out.restype = None
        _lib.emulcov_corr.argtypes = [C.c_int64, C.c_int64, vp, C.c_int64, vp, vp, vp, vp]
        _lib.emulcov_corr.restype = None
    return _lib


def constants():
    """batch_max, batch_default, tile_cols, tile_rows of hmcmt_items.h"""
    L = lib()
    return {"batch_max": int(L.emulcov_batch_max()), "batch_default": int(L.emulcov_batch_default()),
            "tile_cols": int(L.emulcov_tile_cols()), "tile_rows": int(L.emulcov_tile_rows())}


def begin(n, rows, batch):
    """the zeroed state of hmcmt_chain_cov_begin: rows or None (every cell)"""
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    nrow = n if r is None else len(r)
    B = int(batch) if batch else constants()["batch_default"]
    return {"n": int(n), "rows": r, "nrow": nrow, "B": B, "count": 0, "npend": C.c_int32(0), "nflush": C.c_int64(0),
            "x0": np.zeros(n), "tot": np.zeros(n), "q": np.zeros(n), "pend": np.zeros((B, n)), "S": np.zeros((nrow, n))}


def _rowptr(st):
    return None if st["rows"] is None else st["rows"].ctypes.data


def commit(st, samples, reverse=False, flush=False):
    """feeds samples [nparam, nsamples] (columns = committed models) to the state; flush: what a read-out does first"""
    cols = np.ascontiguousarray(np.asarray(samples, dtype=np.float64).T)
    ns = cols.shape[0]
    assert cols.shape[1] == st["n"]
    lib().emulcov_accumulate(st["n"], st["count"], st["count"] + ns, cols.ctypes.data_as(c_double_p), st["nrow"], _rowptr(st), st["B"],
                             *(st[k].ctypes.data for k in ("x0", "tot", "q", "pend", "S")), C.byref(st["npend"]), C.byref(st["nflush"]),
                             int(reverse), int(flush))
    st["count"] += ns
    return st


def accumulate(samples, rows, batch, reverse=False):
    """the state after all of samples [nparam, nsamples], its last batch flushed"""
    samples = np.asarray(samples, dtype=np.float64)
    return commit(begin(samples.shape[0], rows, batch), samples, reverse=reverse, flush=True)


def readout(st, cov=True):
    """(mean[n], var[n], cov[nrow, n]) of a flushed state after its count commits"""
    assert st["npend"].value == 0 and st["count"] >= 1
    n, nrow = st["n"], st["nrow"]
    mean, var, c = np.empty(n), np.empty(n), np.empty((nrow, n))
    lib().emulcov_out(n, nrow, _rowptr(st), st["count"], *(st[k].ctypes.data for k in ("x0", "tot", "q", "S")), mean.ctypes.data,
                      var.ctypes.data, c.ctypes.data if cov else None)
    return mean, var, (c if cov else None)


def corr(st):
    """corr[nrow, n] of a flushed state"""
    assert st["npend"].value == 0 and st["count"] >= 1
    out = np.empty((st["nrow"], st["n"]))
    lib().emulcov_corr(st["n"], st["nrow"], _rowptr(st), st["count"], *(st[k].ctypes.data for k in ("tot", "q", "S")), out.ctypes.data)
    return out
