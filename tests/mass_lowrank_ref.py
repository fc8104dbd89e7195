"""numpy reference of the low-rank-plus-diagonal mass (hmcmt_set_mass_lowrank):

    M^-1 = S (I + U' (Lambda - I) U) S,    M = F F',    F = S^-1 (I + U' (Lambda^-1/2 - I) U)

with S = diag(sqrt(invM)), U [rank, n] with orthonormal ROWS (the library's layout: one direction per row), Lambda = diag(lam).
Two forms: the dense matrices (dense_inv, dense_sqrt), and the two steps of one application in the order the kernels
k_mass_lr_project / k_mass_lr_expand take them through the item functions of hmcmt_items.h (project, expand) -- with an fma that is
exact, so the host instantiation of those functions (tests/emul/emul_mass_lowrank.cpp) must give the same bits."""
import numpy as np

OP_INV, OP_SQRT = 0, 1
NB, NT, WAVE = 64, 256, 64            # LFNB workgroups of 256 threads, waves of 64 lanes
CHUNK = 8


def dense_inv(invM, U, lam):
    s = np.sqrt(np.asarray(invM, dtype=np.float64))
    U = np.asarray(U, dtype=np.float64)
    core = np.eye(len(s)) + U.T @ ((np.asarray(lam) - 1.0)[:, None] * U)
    return s[:, None] * core * s[None, :]


def dense_sqrt(invM, U, lam):
    s = np.sqrt(np.asarray(invM, dtype=np.float64))
    U = np.asarray(U, dtype=np.float64)
    core = np.eye(len(s)) + U.T @ ((1.0 / np.sqrt(np.asarray(lam)) - 1.0)[:, None] * U)
    return core / s[:, None]


DENSE_MAX = 4096                      # above it the dense matrix is not formed (20000 cells: 3.2 GB)


def apply_dense(invM, U, lam, x, op):
    """M^-1 x (OP_INV) or F x (OP_SQRT): with the dense matrix up to DENSE_MAX cells; above, the same product factored and carried in
    longdouble (its own error is below 1e-18 relative, so it stands in for the exact value)"""
    n = len(invM)
    if n <= DENSE_MAX:
        return (dense_inv if op == OP_INV else dense_sqrt)(invM, U, lam) @ np.asarray(x, dtype=np.float64)
    ld = np.longdouble
    s, lam = np.sqrt(np.asarray(invM, dtype=ld)), np.asarray(lam, dtype=ld)
    c = lam - 1 if op == OP_INV else 1 / np.sqrt(lam) - 1
    Ul = np.asarray(U, dtype=ld)
    xp = np.asarray(x, dtype=ld) * (s if op == OP_INV else 1)
    core = xp + Ul.T @ (c * (Ul @ xp))
    return np.asarray(core * s if op == OP_INV else core / s, dtype=np.float64)


class Inverse:
    """invM of oracle.proposeLeapfrog as an operator (as WmInverse in tests/test_gpu_mass.py): p -> M^-1 p by apply_dense"""

    def __init__(self, invM, U, lam):
        self.args = (invM, U, lam)
        self.A = dense_inv(invM, U, lam) if len(invM) <= DENSE_MAX else None

    def __mul__(self, p):
        p = np.asarray(p, dtype=np.float64)
        return self.A @ p if self.A is not None else apply_dense(*self.args, p, OP_INV)


def problem(n, rank, seed=None):
    """(invM, U[rank, n], lam, x): scales from uniform(0.25, 4), lam from 16 down to 0.25 -- on both sides of 1 --, U from numpy's QR"""
    rng = np.random.default_rng(1000 * rank + n if seed is None else seed)
    invM = rng.uniform(0.25, 4.0, n)
    lam = np.array([16.0]) if rank == 1 else np.geomspace(16.0, 0.25, rank)
    U = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((n, rank)))[0].T)
    return invM, U, lam, rng.standard_normal(n)


# ---- an exact fma on arrays (Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums", IEEE TC 2008: the product's two
# halves, the low parts added with rounding to odd, one final rounding to nearest).  Exact while nothing over- or underflows.
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    split = 134217729.0                                    # 2^27 + 1 (Veltkamp)
    ca, cb = split * a, split * b
    ah = ca - (ca - a); al = a - ah
    bh = cb - (cb - b); bl = b - bh
    p = a * b
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_odd(a, b):
    """a + b rounded to odd: where the sum is inexact and its last bit is even, the neighbour on the error's side"""
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0.0) & even
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def fma(a, b, c):
    a, b, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), np.broadcast(a, b, c).shape)) for v in (a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    return vh + _add_odd(tl, vl)


# ---- the order of the kernels ------------------------------------------------------------------------------------------------
def wave_sum(v):
    """v [..., 64] -> [...]: the lanes' tree of wave_sum (kernels_cocg.h): pairs, quads, the row of 16 by two rotations, then
    (row 0 + row 1) + (row 2 + row 3)"""
    v = np.asarray(v, dtype=np.float64)
    q = (v[..., 0::4] + v[..., 1::4]) + (v[..., 2::4] + v[..., 3::4])              # [..., 16] quads
    q = q.reshape(q.shape[:-1] + (4, 4))                                            # [..., row, quad]
    rows = (q[..., 0] + q[..., 3]) + (q[..., 2] + q[..., 1])                        # lane 0 of each row
    return (rows[..., 0] + rows[..., 1]) + (rows[..., 2] + rows[..., 3])


def pre(invM, x, op):
    return np.sqrt(invM) * x if op == OP_INV else np.array(x, dtype=np.float64)


def project(invM, U, x, op):
    """part [rank, NB]: k_mass_lr_project's partial sums of U x'"""
    rank, n = U.shape
    xp = pre(invM, x, op)
    stride = NB * NT
    passes = -(-n // stride)
    acc = np.zeros((rank, stride))
    for j in range(passes):                                                        # a thread walks its cells upwards
        lo, hi = j * stride, min(n, (j + 1) * stride)
        acc[:, :hi - lo] = fma(U[:, lo:hi], xp[None, lo:hi], acc[:, :hi - lo])
    w = wave_sum(acc.reshape(rank, NB, NT // WAVE, WAVE))                           # [rank, NB, 4]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def total(part):
    """the workgroups' partial sums in index order (item_chain_total)"""
    t = np.zeros(part.shape[0])
    for b in range(part.shape[1]):
        t = t + part[:, b]
    return t


def expand(invM, U, lam, x, part, op):
    s = np.sqrt(invM)
    c = (np.asarray(lam) - 1.0) if op == OP_INV else (1.0 / np.sqrt(np.asarray(lam)) - 1.0)
    w = c * total(part)
    acc = pre(invM, x, op)
    for k in range(U.shape[0]):
        acc = fma(U[k], w[k], acc)
    return s * acc if op == OP_INV else acc / s


def apply(invM, U, lam, x, op):
    return expand(invM, U, lam, x, project(invM, U, x, op), op)
