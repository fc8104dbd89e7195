"""ctypes front-end of the TEST-ONLY host instantiation of the Jacobian products (tests/emul/emul_jvp.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

from hmcmt2d_amd.marshal import CreateArgs, CREATE_ARGTYPES, c_double_p

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_jvp.so")
WRT = {"sigma": 0, "lnsigma": 1}


def build(force=False):
    srcs = [os.path.join(HERE, f) for f in ("emul_jvp.cpp", "emul.cpp")]
    hdrs = [os.path.join(HERE, "..", "..", "hmcmt2d_amd", "csrc", h) for h in ("hmcmt_math.h", "hmcmt_items.h", "hmcmt_host.h")]
    newest = max(os.path.getmtime(f) for f in srcs + hdrs)
    if force or not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", srcs[0], "-o", SO])
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emuljvp_create.restype = C.c_void_p
        _lib.emuljvp_create.argtypes = CREATE_ARGTYPES + [C.c_char_p, C.c_int]
        _lib.emuljvp_destroy.argtypes = [C.c_void_p]
        _lib.emuljvp_linearize.argtypes = [C.c_void_p, c_double_p, C.c_int, C.c_double, C.c_int]
        for name in ("emuljvp_jvp", "emuljvp_jtvp"):
            getattr(_lib, name).argtypes = [C.c_void_p, c_double_p, C.c_int, C.c_int, C.c_double, C.c_int, c_double_p]
    return _lib


class EmulJvp:
    """linearize(m), then jvp(v) / jtvp(u): fp64 throughout, every solve to `tol` with the emulation's own COCG."""

    def __init__(self, mtMesh, mtData, invParam, precond=2, tol=1e-12, maxit=20000):
        self.args = CreateArgs(mtMesh, mtData, invParam)
        err = C.create_string_buffer(512)
        self.h = lib().emuljvp_create(*self.args.as_tuple(), err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())
        self.solver = (int(precond), float(tol), int(maxit))

    def linearize(self, m):
        m = np.ascontiguousarray(m, dtype=np.float64)
        lib().emuljvp_linearize(self.h, m.ctypes.data_as(c_double_p), *self.solver)

    def jvp(self, v, wrt="sigma"):
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = np.zeros(self.args.nData, dtype=np.complex128)
        rc = lib().emuljvp_jvp(self.h, v.ctypes.data_as(c_double_p), WRT[wrt], *self.solver, out.ctypes.data_as(c_double_p))
        if rc:
            raise RuntimeError("jvp before linearize")
        return out.real.copy() if self.args.real_data else out

    def jtvp(self, u, wrt="sigma"):
        u = np.ascontiguousarray(u, dtype=np.complex128)
        out = np.zeros(self.args.nAC)
        rc = lib().emuljvp_jtvp(self.h, u.ctypes.data_as(c_double_p), WRT[wrt], *self.solver, out.ctypes.data_as(c_double_p))
        if rc:
            raise RuntimeError("jtvp before linearize")
        return out

    def close(self):
        if self.h:
            lib().emuljvp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
