"""ctypes front-end of the TEST-ONLY host instantiation of the low-rank mass's item functions (tests/emul/emul_mass_lowrank.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_mass_lowrank.so")


def build(force=False):
    src = os.path.join(HERE, "emul_mass_lowrank.cpp")
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
        _lib.emulmlr_project.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp]
        _lib.emulmlr_project.restype = None
        _lib.emulmlr_expand.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
        _lib.emulmlr_expand.restype = None
    return _lib


def constants():
    """rank_max, chunk, blocks of hmcmt_items.h"""
    L = lib()
    return {"rank_max": int(L.emulmlr_rank_max()), "chunk": int(L.emulmlr_chunk()), "blocks": int(L.emulmlr_blocks())}


def _arrays(invM, U, x):
    s = np.sqrt(np.ascontiguousarray(invM, dtype=np.float64))
    U = np.ascontiguousarray(U, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert U.ndim == 2 and U.shape[1] == len(s) == len(x) and 1 <= U.shape[0] <= constants()["rank_max"]
    return s, U, x


def project(invM, U, x, op):
    """part [rank, blocks] of k_mass_lr_project: op 0 (M^-1 x) or 1 (F x)"""
    s, U, x = _arrays(invM, U, x)
    part = np.zeros((U.shape[0], constants()["blocks"]))
    lib().emulmlr_project(len(s), U.shape[0], int(op), s.ctypes.data, U.ctypes.data, x.ctypes.data, part.ctypes.data)
    return part


def expand(invM, U, lam, x, part, op, in_place=False):
    """y of k_mass_lr_expand from the partial sums; in_place: y is written over (a copy of) x, as the kernel allows"""
    s, U, x = _arrays(invM, U, x)
    lam = np.asarray(lam, dtype=np.float64)
    c = np.ascontiguousarray(lam - 1.0 if op == 0 else 1.0 / np.sqrt(lam) - 1.0)
    part = np.ascontiguousarray(part, dtype=np.float64)
    x = x.copy()
    y = x if in_place else np.empty_like(x)
    lib().emulmlr_expand(len(s), U.shape[0], int(op), s.ctypes.data, U.ctypes.data, c.ctypes.data, part.ctypes.data, x.ctypes.data, y.ctypes.data)
    return y


def apply(invM, U, lam, x, op):
    return expand(invM, U, lam, x, project(invM, U, x, op), op)
