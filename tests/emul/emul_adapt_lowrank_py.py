"""ctypes front-end of the TEST-ONLY host instantiation of the low-rank mass adaptation's item functions
(tests/emul/emul_adapt_lowrank.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_adapt_lowrank.so")


def build(force=False):
    src = os.path.join(HERE, "emul_adapt_lowrank.cpp")
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
        _lib.emulalr_mean.argtypes = [C.c_int32, C.c_int64] + [vp] * 6
        _lib.emulalr_w.argtypes = [C.c_int32, C.c_int64] + [vp] * 4
        _lib.emulalr_gram.argtypes = [C.c_int32, C.c_int64] + [vp] * 4
        _lib.emulalr_lift.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, vp, C.c_int32, vp]
        _lib.emulalr_sign.argtypes = [C.c_int64, C.c_int32, vp]
        _lib.emulalr_jacobi.argtypes = [C.c_int32, vp, vp, vp]
        _lib.emulalr_estimate.argtypes = [C.c_int32, vp, C.c_int32, C.c_double, C.c_double, C.c_int32, vp, vp, vp, vp]
        _lib.emulalr_schedule.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
        for f in (_lib.emulalr_mean, _lib.emulalr_w, _lib.emulalr_gram, _lib.emulalr_lift, _lib.emulalr_sign, _lib.emulalr_estimate):
            f.restype = None
    return _lib


def constants():
    L = lib()
    return {"nmin": int(L.emulalr_nmin()), "nmax": int(L.emulalr_nmax()), "tile": int(L.emulalr_tile()), "strip": int(L.emulalr_strip())}


def _rows(X, G, invM):
    X, G = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(G, dtype=np.float64)
    invM = np.ascontiguousarray(invM, dtype=np.float64)
    assert X.ndim == 2 and X.shape == G.shape and X.shape[1] == len(invM)
    return X, G, invM


def w_rows(X, G, invM):
    X, G, invM = _rows(X, G, invM)
    W = np.zeros((2 * X.shape[0], X.shape[1]))
    lib().emulalr_w(X.shape[0], X.shape[1], X.ctypes.data, G.ctypes.data, invM.ctypes.data, W.ctypes.data)
    return W


def gram(X, G, invM):
    X, G, invM = _rows(X, G, invM)
    K = np.zeros((2 * X.shape[0], 2 * X.shape[0]))
    lib().emulalr_gram(X.shape[0], X.shape[1], X.ctypes.data, G.ctypes.data, invM.ctypes.data, K.ctypes.data)
    return K


def lift(X, G, invM, B, sign=False):
    X, G, invM = _rows(X, G, invM)
    B = np.ascontiguousarray(B, dtype=np.float64)
    assert B.shape[0] == 2 * X.shape[0]
    U = np.zeros((B.shape[1], X.shape[1]))
    lib().emulalr_lift(X.shape[0], X.shape[1], X.ctypes.data, G.ctypes.data, invM.ctypes.data, B.ctypes.data, B.shape[1], U.ctypes.data)
    if sign:
        lib().emulalr_sign(X.shape[1], B.shape[1], U.ctypes.data)
    return U


def sign(U):
    U = np.array(U, dtype=np.float64, order="C")
    lib().emulalr_sign(U.shape[1], U.shape[0], U.ctypes.data)
    return U


def jacobi(A):
    """(d ascending, V with the eigenvectors in its COLUMNS as numpy.linalg.eigh returns them, sweeps)"""
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    Vt, d = np.zeros((n, n)), np.zeros(n)
    sweeps = lib().emulalr_jacobi(n, A.ctypes.data, Vt.ctypes.data, d.ctypes.data)
    return d, Vt.T.copy(), int(sweeps)


def estimate_from_gram(K, n, rank=8, cutoff=2.0, gamma=1e-5, geometric=True):
    """dict(m, r, fallback, theta_all [m], theta [r], B [2n, r]) of item_adapt_lr_estimate"""
    K = np.ascontiguousarray(K, dtype=np.float64)
    assert K.shape == (2 * n, 2 * n)
    out = np.zeros(3, dtype=np.int32)
    thAll, th, B = np.zeros(2 * n), np.zeros(rank), np.zeros(2 * n * rank)
    lib().emulalr_estimate(n, K.ctypes.data, rank, cutoff, gamma, 1 if geometric else 0, out.ctypes.data, thAll.ctypes.data, th.ctypes.data,
                           B.ctypes.data)
    m, r = int(out[0]), int(out[1])
    return {"m": m, "r": r, "fallback": int(out[2]), "theta_all": thAll[:m].copy(), "theta": th[:r].copy(),
            "B": B[:2 * n * r].reshape(2 * n, r).copy()}


def estimate(X, G, invM, rank=8, cutoff=2.0, gamma=1e-5, geometric=True):
    """the product's window end without a device: (U [r, nAC] signed, lambda [r], the estimate's dict)"""
    E = estimate_from_gram(gram(X, G, invM), np.asarray(X).shape[0], rank, cutoff, gamma, geometric)
    U = lift(X, G, invM, E["B"], sign=True) if E["r"] else np.zeros((0, np.asarray(X).shape[1]))
    return U, E["theta"], E


def schedule(nwarmup, init_buffer, term_buffer, base_window, max_samples):
    """(slot [nwarmup] (-1: not stored), [(last step, stored, stride)] per closed window) of chain_adapt_step's bookkeeping"""
    slot = np.zeros(nwarmup, dtype=np.int32)
    end, stored, stride = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int64)
    nw = lib().emulalr_schedule(nwarmup, init_buffer, term_buffer, base_window, max_samples, slot.ctypes.data, end.ctypes.data,
                                stored.ctypes.data, stride.ctypes.data)
    return slot, [(int(end[w]), int(stored[w]), int(stride[w])) for w in range(nw)]
