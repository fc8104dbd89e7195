"""ctypes front-end of the TEST-ONLY host instantiation of the No-U-turn sampler's item functions (tests/emul/emul_nuts.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_nuts.so")


def build(force=False):
    src = os.path.join(HERE, "emul_nuts.cpp")
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
        _lib.emulnuts_rng.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        _lib.emulnuts_rng.restype = None
        _lib.emulnuts_checkpoints.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _lib.emulnuts_checkpoints.restype = None
        _lib.emulnuts_leaf.argtypes = [C.c_int64] + [C.c_int32] * 5 + [vp] * 11
        _lib.emulnuts_leaf.restype = None
        _lib.emulnuts_sample.argtypes = [C.c_int32, vp, vp, C.c_double, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp]
        _lib.emulnuts_sample.restype = None
    return _lib


def constants():
    L = lib()
    return {"nq": int(L.emulnuts_nq()), "ck_max": int(L.emulnuts_ck_max()), "group": int(L.emulnuts_group()),
            "depth_max": int(L.emulnuts_depth_max())}


def rng(seed, stream, t, kind, index):
    f, u = C.c_int32(), C.c_double()
    lib().emulnuts_rng(seed, stream, t, kind, index, C.byref(f), C.byref(u))
    return int(f.value), float(u.value)


def checkpoints(i):
    """(slot, ndue) of leaf i: item_nuts_checkpoints"""
    s, d = C.c_int32(), C.c_int32()
    lib().emulnuts_checkpoints(int(i), C.byref(s), C.byref(d))
    return int(s.value), int(d.value)


def _ptr(a):
    return None if a is None else a.ctypes.data


def leaf(p, rho_s, x=None, inv_m=None, backward=False, first=False, ck_write=None, ck_due=(), merged=None):
    """One leaf's pass on host vectors (float64, contiguous; rho_s, ck_write and merged["rho_next"] are written in place), the
    arguments of HipContext.debug_nuts_leaf.  Returns the sums [nq]."""
    n = len(p)
    wr = (C.c_void_p * 3)(*([_ptr(v) for v in ck_write] if ck_write is not None else [None] * 3))
    flat = [_ptr(v) for trip in ck_due for v in trip]
    due = (C.c_void_p * max(len(flat), 1))(*flat)
    m = merged or {}
    sums = np.zeros(constants()["nq"])
    lib().emulnuts_leaf(n, int(bool(backward)), int(bool(m.get("other_backward", False))), int(bool(first)), int(merged is not None), len(ck_due),
                        _ptr(p), _ptr(x), _ptr(inv_m), _ptr(rho_s), C.addressof(wr), C.addressof(due), _ptr(m.get("rho")), _ptr(m.get("rho_next")),
                        _ptr(m.get("p_other")), _ptr(m.get("x_other")), _ptr(sums))
    return sums


def sample(A, inv_m, dt, max_depth, seed, stream, t, m, p0):
    """One sample on the Gaussian target (emulnuts_sample).  Returns (record dict, selected model, energies of the leaves taken)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    inv_m = np.ascontiguousarray(inv_m, dtype=np.float64)
    m = np.array(m, dtype=np.float64)
    p0 = np.ascontiguousarray(p0, dtype=np.float64)
    irec, drec = np.zeros(5, dtype=np.int64), np.zeros(3)
    energies = np.zeros(2 ** max_depth)
    lib().emulnuts_sample(len(m), A.ctypes.data, inv_m.ctypes.data, float(dt), int(max_depth), int(seed), int(stream), int(t), m.ctypes.data,
                          p0.ctypes.data, irec.ctypes.data, drec.ctypes.data, energies.ctypes.data)
    rec = dict(depth=int(irec[0]), nleaves=int(irec[1]), stop=int(irec[2]), dirs=int(irec[3]), selected=int(irec[4]), alpha=float(drec[0]),
               H0=float(drec[1]), Hsel=float(drec[2]))
    return rec, m, energies[:rec["nleaves"]]
