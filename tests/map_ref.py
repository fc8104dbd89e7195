"""Reference of the MAP optimiser (include/hmcmt.h: hmcmt_map_*): projected L-BFGS whose direction comes from the TWO-LOOP recursion in
numpy.longdouble -- the independent form; the library and its host instantiation (tests/emul/emul_map.cpp) use the compact one --
and the iteration as a driver over any callable m -> (Phi, D, g).  Plain numpy, no library code."""
import numpy as np

LD = np.longdouble
RUNNING, CONVERGED, STALLED = 0, 1, 2
DEFAULTS = dict(history=8, max_backtracks=10, c1=1e-4, shrink=0.5, curv_eps=1e-10, gtol=1e-5)


def active_set(m, g, lo, hi):
    return ((m <= lo) & (g > 0)) | ((m >= hi) & (g < 0))


def two_loop(v, pairs):
    """H v in longdouble: pairs [(s, y)] oldest first, H0 = gamma I with gamma = s'y / y'y of the newest (Nocedal & Wright, alg. 7.4)."""
    q = np.asarray(v, dtype=LD).copy()
    P = [(np.asarray(s, dtype=LD), np.asarray(y, dtype=LD)) for s, y in pairs]
    rho = [1 / (s @ y) for s, y in P]
    al = [None] * len(P)
    for i in range(len(P) - 1, -1, -1):
        al[i] = rho[i] * (P[i][0] @ q)
        q -= al[i] * P[i][1]
    s, y = P[-1]
    r = (s @ y) / (y @ y) * q
    for i in range(len(P)):
        be = rho[i] * (P[i][1] @ r)
        r += (al[i] - be) * P[i][0]
    return r


def direction(m, g, lo, hi, pairs):
    """dict(d [longdouble], pg, B, gamma, gTd, flag): steps 1 and 2 of the iteration; flag: the pairs did not give a descent direction
    and d is the direction without them."""
    m, g = np.asarray(m, dtype=float), np.asarray(g, dtype=float)
    B = active_set(m, g, lo, hi)
    pg = np.where(B, 0.0, g)
    pginf = float(np.abs(pg).max())
    flag = False
    d = None
    if pairs:
        s, y = pairs[-1]
        gamma = float((np.asarray(s, dtype=LD) @ np.asarray(y, dtype=LD)) / (np.asarray(y, dtype=LD) @ np.asarray(y, dtype=LD)))
        d = -two_loop(pg, pairs)
        d[B] = 0
        gTd = float(np.asarray(g, dtype=LD) @ d)
        if not gTd < 0:
            flag, d = True, None
    if d is None:
        gamma = min(1.0, 1.0 / pginf) if pginf > 0 else 1.0
        d = -np.asarray(pg, dtype=LD) * LD(gamma)
        gTd = float(np.asarray(g, dtype=LD) @ d)
    return {"d": d, "pg": pg, "B": B, "gamma": gamma, "gTd": gTd, "flag": flag, "pginf": pginf}


def trial_model(m, d, alpha, lo, hi):
    return np.clip(m + alpha * np.asarray(d, dtype=float), lo, hi)


def pair_test(s, y, curv_eps):
    sTy = float(s @ y)
    return sTy > curv_eps * np.sqrt(float(s @ s)) * np.sqrt(float(y @ y)), sTy


class RefMAP:
    """The iteration over f(m) -> (Phi, D, g), g the full gradient.  step() returns a dict with the library's record fields."""

    def __init__(self, f, m_start, lo, hi, **opts):
        self.f, self.lo, self.hi, self.o = f, float(lo), float(hi), dict(DEFAULTS, **opts)
        self.m = np.clip(np.asarray(m_start, dtype=float), lo, hi)
        self.phi, self.D, self.g = f(self.m)
        self.pairs, self.iter, self.nfevals = [], 0, 1
        self._measure()
        self.pginf0 = self.pginf
        self.status = CONVERGED if self.pginf <= self.o["gtol"] * max(1.0, self.pginf0) else RUNNING

    def _measure(self):
        B = active_set(self.m, self.g, self.lo, self.hi)
        pg = np.where(B, 0.0, self.g)
        self.pginf, self.pg2, self.nbound = float(np.abs(pg).max()), float(np.sqrt(pg @ pg)), int(B.sum())

    def _record(self, rec):
        rec.update(iter=self.iter, status=self.status, npairs=len(self.pairs), nbound=self.nbound, phi=self.phi, D=self.D,
                   M=self.phi - self.D, pg_inf=self.pginf, pg_2=self.pg2)
        return rec

    def step(self):
        assert self.status == RUNNING
        o = self.o
        rec = dict(nfevals=0, backtracks=0, resets=0, pair_stored=0, alpha=0.0, gamma=0.0, gTd=0.0, sTy=0.0)
        got = None
        while True:
            had = bool(self.pairs)
            D = direction(self.m, self.g, self.lo, self.hi, self.pairs)
            if D["flag"]:
                rec["resets"] += 1; self.pairs = []; had = False
            rec.update(gamma=D["gamma"], gTd=D["gTd"], phi_trial=np.full(16, np.nan), decided_by=[])
            alpha = 1.0
            for k in range(o["max_backtracks"] + 1):
                if k > 0:
                    alpha *= o["shrink"]
                mt = trial_model(self.m, D["d"], alpha, self.lo, self.hi)
                phi_t, D_t, g_t = self.f(mt)
                rec["nfevals"] += 1
                rec["phi_trial"][k] = phi_t
                rec.update(backtracks=k, alpha=alpha)
                bound = self.phi + o["c1"] * float(self.g @ (mt - self.m))
                rec["decided_by"].append(abs(phi_t - bound) / abs(self.phi))
                if np.isfinite(phi_t) and phi_t <= bound:
                    got = (mt, phi_t, D_t, np.asarray(g_t, dtype=float))
                    break
            if got or not had:
                break
            rec["resets"] += 1; self.pairs = []
        self.nfevals += rec["nfevals"]
        if not got:
            self.status = STALLED
            rec["alpha"] = 0.0
            return self._record(rec)
        mt, phi_t, D_t, g_t = got
        s, y = mt - self.m, g_t - self.g
        keep, rec["sTy"] = pair_test(s, y, o["curv_eps"])
        if keep:
            self.pairs = (self.pairs + [(s, y)])[-o["history"]:]
            rec["pair_stored"] = 1
        self.m, self.g, self.phi, self.D = mt, g_t, phi_t, D_t
        self.iter += 1
        self._measure()
        if self.pginf <= o["gtol"] * max(1.0, self.pginf0):
            self.status = CONVERGED
        return self._record(rec)

    def run(self, maxiter):
        recs = []
        while self.status == RUNNING and len(recs) < maxiter:
            recs.append(self.step())
        return recs


def replay_step(m, g, phi, pairs, lo, hi, phi_trial, m_new, g_new, resets=0, **opts):
    """One step of the reference on a GIVEN state (m, g, phi, pairs oldest first), fed the Phi of the trials instead of evaluating
    (field-replay manner: no error accumulates): which trial passes the Armijo test, and -- with the state the step under test
    returned, m_new and g_new -- the pair decision and the new active set.  resets: what the record under test counted; a reset after
    a failed first round cannot be replayed from the last round's trials and is taken from it.  Returns dict(alpha, backtracks,
    accepted, flag, d, gamma, gTd, pair_stored, sTy, nbound, npairs)."""
    o = dict(DEFAULTS, **opts)
    D = direction(m, g, lo, hi, pairs)
    used = list(pairs)
    if D["flag"]:
        used = []
    elif resets > 0 and pairs:
        used = []
        D = direction(m, g, lo, hi, [])
    out = {"flag": D["flag"], "d": np.asarray(D["d"], dtype=float), "gamma": D["gamma"], "gTd": D["gTd"], "accepted": False, "alpha": 0.0,
           "backtracks": 0, "pair_stored": 0, "sTy": 0.0, "npairs": len(used)}
    alpha = 1.0
    for k in range(o["max_backtracks"] + 1):
        if k > 0:
            alpha *= o["shrink"]
        mt = trial_model(m, D["d"], alpha, lo, hi)
        out["backtracks"] = k
        if np.isfinite(phi_trial[k]) and phi_trial[k] <= phi + o["c1"] * float(g @ (mt - m)):
            out.update(accepted=True, alpha=alpha, mt=mt)
            break
    if out["accepted"]:
        keep, out["sTy"] = pair_test(m_new - m, g_new - g, o["curv_eps"])
        out["pair_stored"] = int(keep)
        out["npairs"] = min(len(used) + int(keep), o["history"])
        out["nbound"] = int(active_set(m_new, g_new, lo, hi).sum())
    else:
        out["nbound"] = int(active_set(m, g, lo, hi).sum())
    return out
