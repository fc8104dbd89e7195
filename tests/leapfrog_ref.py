"""A plain reference of one leapfrog trajectory (proposeLeapfrog / checkParameterBound, HMCSampler.jl:206-269, 515-559): numpy,
every value in np.longdouble, no GPU, no ctypes and nothing of the library's.  The step is dm = dt M^-1 p; if max|dm| > 3 every
element is scaled by 3 / max|dm|; the model is reflected at the ln-sigma bounds and the momentum flipped with it.

M^-1 is one of three operators (DiagonalMass, WmMass, LowRankMass: inv, mul and absinv, the last for the bars); the data gradient
comes from a callback.  trajectory() returns, per step, everything a test needs to say WHERE an implementation went wrong: p before
the position update, x = M^-1 p, mx = max|dt x|, whether it clamped, the clamp factor, the reflection count per element, the model,
p after the momentum update, and the absolute-summand totals of the momentum; bars() turns those into float64 rounding bounds.

With `models` the trajectory is a REPLAY: each step's momentum update, and the step behind it, start from the model the
implementation under test returned for that step, so that its model error reaches the momentum through neither the gradient nor Wm.

tests/test_leapfrog_host.py holds this file to oracle.proposeLeapfrog, tests/test_gpu_leapfrog_updates.py holds the kernels to it."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MAX_STEP = 3.0                                 # maxStepSize, HMCSampler.jl:236
MAX_REFLECT = 500


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


class Rows:
    """a sparse (scipy, anything with tocoo()) or dense matrix as long-double triplets: A d and |A| |d| by rows"""

    def __init__(self, A):
        if hasattr(A, "tocoo"):
            coo = A.tocoo()
            self.row, self.col, val = np.asarray(coo.row), np.asarray(coo.col), np.asarray(coo.data, dtype=np.float64)
            self.n = coo.shape[0]
        else:
            dense = np.asarray(A, dtype=np.float64)
            self.row, self.col = np.nonzero(dense)
            val = dense[self.row, self.col]
            self.n = dense.shape[0]
        self.val = val.astype(LD)
        self.rownnz = int(np.bincount(self.row, minlength=self.n).max()) if len(self.row) else 0

    def _sum(self, terms):
        out = np.zeros(self.n, dtype=LD)
        np.add.at(out, self.row, terms)
        return out

    def mul(self, d):
        return self._sum(self.val * d[self.col])

    def absmul(self, d):
        return self._sum(np.abs(self.val) * np.abs(d[self.col]))


# ---- the mass operators: inv(p) = M^-1 p, mul(x) = M x in long double; absinv(b) = |M^-1| b (entrywise absolute values: how an
# error bound b on p reaches x), float64 --------------------------------------------------------------------------------------------
class DiagonalMass:
    def __init__(self, invM):
        self.w = _ld(invM)

    def inv(self, p):
        return self.w * p

    def mul(self, x):
        return x / self.w

    def absinv(self, b):
        return np.asarray(self.w, dtype=np.float64) * b


class WmMass:
    """M = Wm: scipy's sparse LU with long-double residuals (three rounds of refinement: the correction falls below 1e-18 relative
    for the matrices of the tests, condition 1e3 .. 1e6)"""
    DENSE_MAX = 1024

    def __init__(self, Wm):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        self.A = Rows(Wm)
        self.lu = spla.splu(sp.csc_matrix(Wm))
        self._abs = np.abs(np.linalg.inv(sp.csr_matrix(Wm).toarray())) if self.A.n <= self.DENSE_MAX else None

    def inv(self, p):
        x = self.lu.solve(np.asarray(p, dtype=np.float64)).astype(LD)
        for _ in range(3):
            r = p - self.A.mul(x)
            x = x + self.lu.solve(np.asarray(r, dtype=np.float64)).astype(LD)
        return x

    def mul(self, x):
        return self.A.mul(x)

    def absinv(self, b):
        if self._abs is None:
            raise ValueError("absinv: the dense inverse is formed up to DENSE_MAX rows only")
        return self._abs @ b


class LowRankMass:
    """M^-1 = S (I + U' (Lambda - I) U) S, M = S^-1 (I + U' (Lambda^-1 - I) U) S^-1; S = diag(sqrt(invM)), U [rank, n] with
    orthonormal rows, Lambda = diag(lam) (hmcmt_set_mass_lowrank; tests/mass_lowrank_ref.py has the float64 forms)"""
    DENSE_MAX = 1024

    def __init__(self, invM, U, lam):
        self.s, self.U, self.lam = np.sqrt(_ld(invM)), _ld(U), _ld(lam)

    def _core(self, y, c):
        return y + self.U.T @ (c * (self.U @ y))

    def inv(self, p):
        return self.s * self._core(self.s * p, self.lam - 1)

    def mul(self, x):
        return self._core(x / self.s, 1 / self.lam - 1) / self.s

    def absinv(self, b):
        n = len(self.s)
        if n > self.DENSE_MAX:
            raise ValueError("absinv: the dense inverse is formed up to DENSE_MAX rows only")
        A = self.s[:, None] * (np.eye(n, dtype=LD) + self.U.T @ ((self.lam - 1)[:, None] * self.U)) * self.s[None, :]
        return np.abs(np.asarray(A, dtype=np.float64)) @ b


def reflect(m, p, lo, hi):
    """checkParameterBound: (m, p, count, margin) with count the reflections per element and margin the smallest distance by which
    an element was outside a bound when it was reflected (inf where it never was): how far the decision is from going the other way"""
    m, p = m.copy(), p.copy()
    count = np.zeros(len(m), dtype=np.int64)
    margin = np.full(len(m), np.inf)
    for _ in range(MAX_REFLECT):
        if not np.any((m < lo) | (m > hi)):
            break
        below = m < lo
        margin[below] = np.minimum(margin[below], np.asarray(lo - m[below], dtype=np.float64))
        m[below] = 2 * lo - m[below]; p[below] = -p[below]; count[below] += 1
        above = m > hi
        margin[above] = np.minimum(margin[above], np.asarray(m[above] - hi, dtype=np.float64))
        m[above] = 2 * hi - m[above]; p[above] = -p[above]; count[above] += 1
    else:
        raise FloatingPointError("an element is still outside the bounds after 500 reflections")
    return m, p, count, margin


def trajectory(m0, p0, dt, L, lam, mref, Wm, lo, hi, mass, grad, models=None):
    """One trajectory of L steps.  grad(k, m): the DATA gradient (float64 [n]) at the float64 model m of step k (k = 0: the start).
    models: None, or the L models the implementation under test returned behind its position updates (see the module's text).
    Returns a dict: m, p (float64), nfevals, T (the absolute-summand total of p, per element) and steps, one dict per step with
    p_before, x, mx, clamped, factor, dm, start (the model the step started from), count, margin, m, p_position (p behind the
    reflection), model (the model of the momentum update), gtot, c, p, T -- long double unless said otherwise."""
    W = Rows(Wm)
    m, p = _ld(m0), _ld(p0)
    mref, lo, hi, dt, lam = _ld(mref), LD(lo), LD(hi), LD(dt), LD(lam)
    if models is not None and len(models) != L:
        raise ValueError("trajectory: one model per step")

    def total_gradient(k, model):
        g = _ld(grad(k, np.asarray(model, dtype=np.float64)))
        d = model - mref
        return g + lam * W.mul(d), np.abs(g) + abs(lam) * W.absmul(d)

    g, ga = total_gradient(0, m)
    nfevals = 1
    p = p - LD(0.5) * dt * g
    T = np.abs(_ld(p0)) + LD(0.5) * dt * ga
    half = dict(p=p.copy(), T=np.asarray(T, dtype=np.float64), gtot=g)
    steps = []
    for k in range(1, L + 1):
        s = dict(p_before=p.copy(), start=m.copy())
        x = mass.inv(p)
        dm = dt * x
        mx = np.abs(dm).max()
        clamped = bool(mx > MAX_STEP)
        factor = LD(MAX_STEP) / mx if clamped else LD(1)
        if clamped:
            dm = dm / mx * LD(MAX_STEP)
        mk, p, count, margin = reflect(m + dm, p, lo, hi)
        s.update(x=x, mx=float(mx), imax=int(np.abs(dt * x).argmax()), clamped=clamped, factor=float(factor), dm=dm, count=count,
                 margin=margin, m=mk.copy(), p_position=p.copy())
        m = mk if models is None else _ld(models[k - 1])
        g, ga = total_gradient(k, m)
        nfevals += 1
        c = LD(1.0 if k < L else 0.5)
        p = p - c * dt * g
        T = T + c * dt * ga
        s.update(model=m.copy(), gtot=g, c=float(c), p=p.copy(), T=np.asarray(T, dtype=np.float64))
        steps.append(s)
    return dict(m=np.asarray(steps[-1]["m"], dtype=np.float64), p=np.asarray(p, dtype=np.float64), nfevals=nfevals,
                T=np.asarray(T, dtype=np.float64), half=half, steps=steps, replay=models is not None,
                dt=float(dt), lam=float(lam), lo=float(lo), hi=float(hi), rownnz=W.rownnz, W=W)


def bars(traj, mass, solve_rel=0.0, lipschitz=0.0):
    """Float64 rounding bounds on an implementation of `traj`, per element: (bm, bp), lists with one entry per step, on the model
    behind the position update and on the momentum behind the momentum update.

    Momentum: every update p - c dt (g + lam Wm (m - mref)) is a row of Wm plus a handful of operations, each rounding a partial sum
    that the absolute-summand total T bounds: (row nonzeros + 8) eps T, T running over the whole trajectory.
    Model, first step: dt x, / mx * 3, the sum, and two operations per reflection, on values within |m| + |dm| + max(|lo|, |hi|):
    (8 + 2 reflections) eps (|m| + |dm| + max(|lo|, |hi|)); a solver for x that is good to solve_rel of max|x| adds
    dt factor solve_rel max|x|.
    Later steps add what the momentum's bound does to them: factor dt |M^-1| bp, and |dm| times the relative error of mx when clamped.
    Without a replay the model's error goes on into the next step, and into the momentum through Wm and through a data gradient
    with the Lipschitz constant `lipschitz` (per element, on the maximum norm of the model's error)."""
    dt, lam, W = traj["dt"], traj["lam"], traj["W"]
    B = max(abs(traj["lo"]), abs(traj["hi"]))
    c_p = (traj["rownnz"] + 8) * EPS
    bp = c_p * traj["half"]["T"]
    T_prev = traj["half"]["T"]
    carried = np.zeros_like(bp)
    bm_all, bp_all = [], []
    for k, s in enumerate(traj["steps"]):
        dm = np.abs(np.asarray(s["dm"], dtype=np.float64))
        start = np.abs(np.asarray(s["start"], dtype=np.float64))
        xmax = float(np.abs(np.asarray(s["x"], dtype=np.float64)).max())
        bm = (8 + 2 * s["count"]) * EPS * (start + dm + B) + dt * s["factor"] * solve_rel * xmax
        if k > 0:
            dx = mass.absinv(bp)
            bm = bm + s["factor"] * dt * dx
            if s["clamped"]:
                bm = bm + dm * (dt * float(dx.max()) / s["mx"])
        bm = bm + carried
        bm_all.append(bm)
        if not traj["replay"]:
            carried = bm
        dT = s["T"] - T_prev
        T_prev = s["T"]
        bp = bp + c_p * dT
        if not traj["replay"]:
            bp = bp + s["c"] * dt * (lipschitz * float(bm.max()) + abs(lam) * np.asarray(W.absmul(bm.astype(LD)), dtype=np.float64))
        bp_all.append(bp)
    return bm_all, bp_all
