"""ctypes front-end of the TEST-ONLY host instantiation of the row sketch's item functions (tests/emul/emul_sketch.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_sketch.so")


def build(force=False):
    src = os.path.join(HERE, "emul_sketch.cpp")
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
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, args, res in (("emulsk_commit", [i64, i64, i32, vp, vp, vp, vp, vp], None), ("emulsk_gram", [i64, i32, vp, vp, vp], None),
                                ("emulsk_shrink_T", [i32, vp, vp, C.POINTER(C.c_double)], i32), ("emulsk_apply", [i64, i32, vp, vp], None),
                                ("emulsk_mean", [i64, i64, vp, vp], None), ("emulsk_pca", [i32, vp, i32, vp, vp], i32),
                                ("emulsk_lift", [i64, i32, vp, vp, vp, i32, vp], None)):
            getattr(_lib, name).argtypes = args
            getattr(_lib, name).restype = res
    return _lib


def constants():
    L = lib()
    return {k: int(getattr(L, "emulsk_" + k)()) for k in ("ell_min", "ell_max", "ell_default", "cols", "sweeps_max")}


def begin(n, ell, pivot=None):
    """the zeroed state of hmcmt_chain_sketch_begin"""
    x0 = np.zeros(n) if pivot is None else np.array(pivot, dtype=np.float64)
    return {"n": int(n), "ell": int(ell), "fill": 0, "count": 0, "shrinks": 0, "Delta": 0.0, "pivot_given": int(pivot is not None),
            "x0": x0, "tot": np.zeros(n), "q": np.zeros(n), "B": np.zeros((2 * ell + 1, n)), "K": [], "T": [], "shrunk": []}


def gram(st, nrows, mean_row=False):
    nw = nrows + (1 if mean_row else 0)
    K = np.empty((nw, nw))
    lib().emulsk_gram(st["n"], nrows, st["B"].ctypes.data, st["B"][2 * st["ell"]].ctypes.data if mean_row else None, K.ctypes.data)
    return K


def shrink_T(ell, K):
    """(T[ell, 2 ell], delta) of the library's host code, or None where the eigensolver gave up"""
    K = np.ascontiguousarray(K, dtype=np.float64)
    T, delta = np.empty((ell, 2 * ell)), C.c_double()
    ok = lib().emulsk_shrink_T(ell, K.ctypes.data, T.ctypes.data, C.byref(delta))
    return (T, float(delta.value)) if ok else None


def apply_T(st, T):
    T = np.ascontiguousarray(T, dtype=np.float64)
    lib().emulsk_apply(st["n"], st["ell"], T.ctypes.data, st["B"].ctypes.data)


def commit(st, models, T_given=None):
    """feeds models [N, n] (rows = committed models) to the state, shrinking as hmcmt_chain_step does; T_given: a list of T, one per
    shrink from the state's shrink count on, used in place of the emulation's own (the library's, so that B is compared given T)"""
    X = np.ascontiguousarray(models, dtype=np.float64)
    assert X.ndim == 2 and X.shape[1] == st["n"]
    ell = st["ell"]
    for m in X:
        lib().emulsk_commit(st["n"], st["count"], st["pivot_given"], m.ctypes.data, st["x0"].ctypes.data, st["tot"].ctypes.data,
                            st["q"].ctypes.data, st["B"][st["fill"]].ctypes.data)
        st["count"] += 1
        st["fill"] += 1
        if st["fill"] == 2 * ell:
            K = gram(st, 2 * ell)
            T, delta = shrink_T(ell, K)
            st["K"].append(K)
            st["T"].append(T)
            apply_T(st, T if T_given is None else T_given[st["shrinks"]])
            st["shrunk"].append(st["B"][:ell].copy())
            st["Delta"] += delta
            st["shrinks"] += 1
            st["fill"] = ell
    return st


def as_sketch(st):
    """the state as a sketch dict (sampler.sketchOf's keys)"""
    N = float(max(st["count"], 1))
    out = {k: st[k] for k in ("count", "ell", "fill", "shrinks", "Delta", "pivot_given", "x0", "tot", "q")}
    out.update(mean=st["x0"] + st["tot"] / N, var=(st["q"] - st["tot"] * st["tot"] / N) / N, rows=st["B"][:st["fill"]].copy())
    return out


def pca(st, rank):
    """(lam[r], U[r, n], err, G, coef) of hmcmt_chain_pca on the state (its mean row is written, nothing else)"""
    n, N, fill = st["n"], st["count"], st["fill"]
    lib().emulsk_mean(n, N, st["tot"].ctypes.data, st["B"][2 * st["ell"]].ctypes.data)
    G = gram(st, fill, True)
    theta, coef = np.zeros(rank), np.zeros((fill + 1) * rank)
    r = lib().emulsk_pca(fill + 1, G.ctypes.data, rank, theta.ctypes.data, coef.ctypes.data)
    assert r >= 0
    coef = np.ascontiguousarray(coef[:(fill + 1) * r].reshape(fill + 1, r)) if r else np.zeros((fill + 1, 0))
    U = np.zeros((r, n))
    if r:
        lib().emulsk_lift(n, fill, st["B"].ctypes.data, st["B"][2 * st["ell"]].ctypes.data, coef.ctypes.data, r, U.ctypes.data)
    return theta[:r] / float(N), U, st["Delta"] / float(N), G, coef
