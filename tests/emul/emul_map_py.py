"""ctypes front-end of the TEST-ONLY host instantiation of the MAP optimiser's item functions (tests/emul/emul_map.cpp), and the
library's host logic (hmcmt2d_amd/csrc/host_map.h: hmcmt_map_begin / hmcmt_map_step) over them for any callable objective."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_build", "libhmcmt_emul_map.so")
MC_GAMMA, MC_FLAG, MC_GTD, MC_PGINF, MC_PG2, MC_NB, MC_USED, MC_A, MC_W, MAP_COEF = 0, 1, 2, 3, 4, 5, 6, 8, 40, 72
RUNNING, CONVERGED, STALLED = 0, 1, 2
DEFAULTS = dict(history=8, max_backtracks=10, c1=1e-4, shrink=0.5, curv_eps=1e-10, gtol=1e-5)


def build(force=False):
    src = os.path.join(HERE, "emul_map.cpp")
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
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        _lib.emulmap_project.argtypes = [i64, i32, i32, i32, vp, vp, vp, dbl, dbl, vp, vp]
        _lib.emulmap_coef.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
        _lib.emulmap_expand.argtypes = [i64, i32, i32, i32, vp, vp, vp, vp, vp, dbl, dbl, dbl, vp, vp]
        _lib.emulmap_clip.argtypes = [i64, vp, vp, dbl, dbl, dbl, vp]
        _lib.emulmap_trial.argtypes = [i64, vp, vp, vp, vp, dbl, dbl, vp]
        _lib.emulmap_pair.argtypes = [i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, dbl, dbl, vp, vp]
        for f in (_lib.emulmap_project, _lib.emulmap_coef, _lib.emulmap_expand, _lib.emulmap_clip, _lib.emulmap_trial, _lib.emulmap_pair):
            f.restype = None
    return _lib


def constants():
    L = lib()
    return {"history_max": int(L.emulmap_history_max()), "part_rows": int(L.emulmap_part_rows()), "coef": int(L.emulmap_coef_len())}


def _v(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data


def direction(rows, head, count, sy, yy, m, g, lo, hi, alpha=1.0):
    """k_map_project, k_map_coef, k_map_expand: dict(pg, d, mt, coef [72], proj [2 count]).  rows [2 H, n] (None with count = 0)."""
    m, g = _v(m), _v(g)
    n = len(m)
    if rows is None:
        H, rows, sy, yy = 1, np.zeros((2, n)), np.zeros((1, 1)), np.zeros((1, 1))
    rows, sy, yy = _v(rows), _v(sy), _v(yy)
    H = rows.shape[0] // 2
    assert rows.shape == (2 * H, n) and sy.shape == (H, H) and yy.shape == (H, H) and 0 <= count <= H and 0 <= head < H
    L = lib()
    pg, d, mt = np.empty(n), np.empty(n), np.empty(n)
    part, coef, proj = np.zeros(L.emulmap_part_rows() * 64), np.zeros(MAP_COEF), np.zeros(64)
    L.emulmap_project(n, H, head, count, _p(rows), _p(m), _p(g), lo, hi, _p(pg), _p(part))
    L.emulmap_coef(H, head, count, _p(sy), _p(yy), _p(part), _p(coef), _p(proj))
    L.emulmap_expand(n, H, head, count, _p(rows), _p(coef), _p(pg), _p(m), _p(g), lo, hi, alpha, _p(d), _p(mt))
    return {"pg": pg, "d": d, "mt": mt, "coef": coef, "proj": proj[:2 * count].copy()}


def clip(m, d, alpha, lo, hi):
    m, d = _v(m), _v(d)
    mt = np.empty(len(m))
    lib().emulmap_clip(len(m), _p(m), _p(d), alpha, lo, hi, _p(mt))
    return mt


def trial(m0, g0, m1, g1, lo, hi):
    """dict(gTs, sTy, sTs, yTy, pg2, pginf, nbound) of a trial's pass (m0, g0 None: no state yet)."""
    m1, g1 = _v(m1), _v(g1)
    m0 = None if m0 is None else _v(m0)
    g0 = None if g0 is None else _v(g0)
    out = np.zeros(7)
    lib().emulmap_trial(len(m1), _p(m0), _p(g0), _p(m1), _p(g1), lo, hi, _p(out))
    return dict(zip(("gTs", "sTy", "sTs", "yTy", "pg2", "pginf", "nbound"), out.tolist()))


def pair(rows, head, count, slot, m0, g0, m1, g1, sTy, yTy, sy, yy):
    """k_map_pair + k_map_pair_final in place on rows, sy, yy (float64, C-ordered): (head, count) the pairs that stay."""
    H = rows.shape[0] // 2
    for a in (rows, sy, yy):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    m0, g0, m1, g1 = _v(m0), _v(g0), _v(m1), _v(g1)
    lib().emulmap_pair(len(m0), H, head, count, slot, _p(rows), _p(m0), _p(g0), _p(m1), _p(g1), sTy, yTy, _p(sy), _p(yy))


class EmulMAP:
    """hmcmt_map_begin / hmcmt_map_step of host_map.h over the host instantiation, for a callable f(m) -> (Phi, g) with Phi the whole
    objective and g its full gradient.  Records are dicts with the library's fields (D = Phi, M = 0)."""

    def __init__(self, f, m_start, lo, hi, **opts):
        self.f, self.lo, self.hi = f, float(lo), float(hi)
        self.o = dict(DEFAULTS, **opts)
        H = self.o["history"]
        self.m = np.clip(_v(m_start), lo, hi)
        n = len(self.m)
        self.rows, self.sy, self.yy = np.zeros((2 * H, n)), np.zeros((H, H)), np.zeros((H, H))
        self.head = self.count = self.iter = 0
        self.phi, self.g = f(self.m)
        self.g = _v(self.g)
        t = trial(None, None, self.m, self.g, self.lo, self.hi)
        self.pg2, self.pginf, self.nbound = t["pg2"], t["pginf"], int(t["nbound"])
        self.pginf0 = self.pginf
        self.status = CONVERGED if self.pginf <= self.o["gtol"] * max(1.0, self.pginf0) else RUNNING

    def _record(self, rec):
        rec.update(iter=self.iter, status=self.status, npairs=self.count, nbound=self.nbound, phi=self.phi, pg_inf=self.pginf,
                   pg_2=float(np.sqrt(self.pg2)))
        return rec

    def _round(self, rec):
        o = self.o
        D = direction(self.rows, self.head, self.count, self.sy, self.yy, self.m, self.g, self.lo, self.hi, 1.0)
        alpha, mt = 1.0, D["mt"]
        rec["phi_trial"] = np.full(16, np.nan)
        rec["d"] = D["d"]
        for k in range(o["max_backtracks"] + 1):
            if k > 0:
                alpha *= o["shrink"]
                mt = clip(self.m, D["d"], alpha, self.lo, self.hi)
            phi_t, g_t = self.f(mt)
            g_t = _v(g_t)
            rec["nfevals"] += 1
            t = trial(self.m, self.g, mt, g_t, self.lo, self.hi)
            rec["phi_trial"][k] = phi_t
            rec.update(backtracks=k, alpha=alpha, gamma=float(D["coef"][MC_GAMMA]), gTd=float(D["coef"][MC_GTD]))
            fell = D["coef"][MC_FLAG] != 0.0
            if np.isfinite(phi_t) and np.isfinite(t["pg2"]) and phi_t <= self.phi + o["c1"] * t["gTs"]:
                return True, fell, (mt, g_t, phi_t, t)
        return False, fell, None

    def step(self):
        assert self.status == RUNNING
        rec = dict(nfevals=0, backtracks=0, resets=0, pair_stored=0, alpha=0.0, gamma=0.0, gTd=0.0, sTy=0.0)
        while True:
            had = self.count > 0
            ok, fell, got = self._round(rec)
            used = had
            if had and fell:
                rec["resets"] += 1; self.head = self.count = 0; used = False
            if ok or not used:
                break
            rec["resets"] += 1; self.head = self.count = 0
        if not ok:
            self.status = STALLED
            rec["alpha"] = 0.0
            return self._record(rec)
        mt, g_t, phi_t, t = got
        H = self.o["history"]
        rec["sTy"] = t["sTy"]
        if t["sTy"] > self.o["curv_eps"] * np.sqrt(t["sTs"]) * np.sqrt(t["yTy"]):
            if self.count == H:
                self.head = (self.head + 1) % H; self.count -= 1
            slot = (self.head + self.count) % H
            pair(self.rows, self.head, self.count, slot, self.m, self.g, mt, g_t, t["sTy"], t["yTy"], self.sy, self.yy)
            self.count += 1
            rec["pair_stored"] = 1
        self.m, self.g, self.phi = mt, g_t, phi_t
        self.pg2, self.pginf, self.nbound = t["pg2"], t["pginf"], int(t["nbound"])
        self.iter += 1
        if self.pginf <= self.o["gtol"] * max(1.0, self.pginf0):
            self.status = CONVERGED
        return self._record(rec)

    def run(self, maxiter):
        recs = []
        while self.status == RUNNING and len(recs) < maxiter:
            recs.append(self.step())
        return recs
