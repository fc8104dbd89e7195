"""Reference side of the MUMPS-symbol tests (tests/test_gpu_mumps.py, tests/test_mumps_host.py): no GPU, no library.

  true_relres   ||b - A x||_2 / ||b||_2 per column, accumulated in extended precision from the COO triplets -- the
                independent measure every solve of the GPU tests is held to
  builders      the matrices that reach each kernel instantiation of csrc/mumps_shim.hip (lanes per row are chosen by
                nnz / n <= 12), seeded
  jacobi_cocg   a plain numpy twin of the library's algorithm (Jacobi preconditioner, unconjugated inner products),
                used only to size the end-to-end bars of the replay test
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


# ---- the measure ----------------------------------------------------------------------------------------------------
def true_relres(A, x, b, ord=2):
    """Per-column ||b - A x|| / ||b|| (float64 array, one entry per column; of length 1 for 1-D b) in the 2-norm, or
    the 1-norm with ord = 1.  The residual is summed in np.longdouble / np.clongdouble over the COO triplets, not
    with an fp64 matvec."""
    A = sp.coo_matrix(A)
    b = np.asarray(b)
    x = np.asarray(x).reshape(b.shape)
    cm = np.iscomplexobj(A.data) or np.iscomplexobj(x) or np.iscomplexobj(b)
    dt = np.clongdouble if cm else np.longdouble
    B = b.reshape(b.shape[0], -1).astype(dt)
    X = x.reshape(b.shape[0], -1).astype(dt)
    R = B.copy()
    np.add.at(R, A.row, -(A.data.astype(dt)[:, None] * X[A.col, :]))
    if ord == 1:
        nr, nb = np.abs(R).sum(axis=0), np.abs(B).sum(axis=0)
    else:
        nr, nb = np.sqrt((np.abs(R) ** 2).sum(axis=0)), np.sqrt((np.abs(B) ** 2).sum(axis=0))
    return np.asarray(nr / nb, dtype=np.float64)


def kappa1(A, lu=None):
    """1-norm condition number: from the dense inverse up to n = 1000, from onenormest above (with the SuperLU
    factors `lu` of A when the caller has them)."""
    A = sp.csc_matrix(A)
    n = A.shape[0]
    if n <= 1000:
        D = A.toarray()
        return float(np.linalg.norm(D, 1) * np.linalg.norm(np.linalg.inv(D), 1))
    lu = spla.splu(A) if lu is None else lu
    dt = A.dtype
    inv = spla.LinearOperator((n, n), dtype=dt, matvec=lambda v: lu.solve(np.asarray(v, dtype=dt).reshape(-1)),
                              rmatvec=lambda v: lu.solve(np.asarray(v, dtype=dt).reshape(-1), "H"))
    return float(spla.onenormest(A) * spla.onenormest(inv))


# ---- the matrices ---------------------------------------------------------------------------------------------------
def tridiag(n, off=1.0, diag=4.0):
    d = np.full(n, diag) if np.isscalar(diag) else np.asarray(diag, dtype=float)
    if n == 1:
        return sp.csc_matrix(d.reshape(1, 1))
    return sp.diags([np.full(n - 1, off), d, np.full(n - 1, off)], [-1, 0, 1], format="csc")


def pentadiag(n):
    return sp.diags([np.full(n - 2, 1.0), np.full(n - 1, 2.0), np.full(n, 6.0), np.full(n - 1, 2.0), np.full(n - 2, 1.0)],
                    [-2, -1, 0, 1, 2], format="csc")


def K27():
    """kron(T, T, T), T = tridiag(1, 4, 1) of size 21: n = 9261, 24.5 per row -> 16 lanes, a second grid-stride pass
    (n > 512 * 16), last block 13 of 16 rows."""
    T = tridiag(21)
    return sp.kron(T, sp.kron(T, T)).tocsc()


def P25():
    """kron(P[:13, :13], P), P = pentadiag(1, 2, 6, 2, 1) of size 14: n = 182, 20.7 per row -> 16 lanes, one pass,
    ragged last block (182 = 11 * 16 + 6)."""
    P = pentadiag(14)
    return sp.kron(P[:13, :13], P).tocsc()


def MIX(seed=0):
    """blockdiag(band of half-width 20 with entries 1 / (1 + |k|) plus 8 I (601 rows), diag(1 + U) (299 rows)):
    n = 900, 27.2 per row -> 16 lanes; rows of one entry beside rows of 21 .. 41."""
    rng = np.random.default_rng(seed)
    ks = np.arange(-20, 21)
    band = sp.diags([np.full(601 - abs(k), 1.0 / (1 + abs(k))) for k in ks], ks, format="csc") + 8.0 * sp.identity(601)
    return sp.block_diag([band, sp.diags(1.0 + rng.random(299))], format="csc")


def ARROW(seed=0, n=3000):
    """tridiag(1, 4 + U, 1) + 1e-3 in row / column 0: n = 3000, 5.0 per row -> 4 lanes, one row of 3000 entries."""
    rng = np.random.default_rng(seed)
    A = tridiag(n, 1.0, 4.0 + rng.random(n)).tolil()
    A[0, :] = A[0, :].toarray() + 1e-3
    A[1:, 0] = A[1:, 0].toarray() + 1e-3
    return A.tocsc()


def TRI(n):
    return tridiag(n)


def circulant(n, offsets, diag=16.0):
    rows = np.repeat(np.arange(n), len(offsets))
    cols = (rows + np.tile(np.asarray(offsets), n)) % n
    vals = np.where(rows == cols, diag, 1.0)
    return sp.csc_matrix((vals, (rows, cols)), shape=(n, n))


def C12():
    """symmetric circulant, n = 256, offsets {0, +-1 .. +-5, 128}: exactly 12.0 per row -> 4 lanes"""
    return circulant(256, [0, 128] + [s * k for k in range(1, 6) for s in (1, -1)])


def C14():
    """the same plus +-6: exactly 14.0 per row -> 16 lanes"""
    return circulant(256, [0, 128] + [s * k for k in range(1, 7) for s in (1, -1)])


def complexify(A, seed=0):
    """A + i diag(20 U(0, 1))"""
    rng = np.random.default_rng(seed + 1000)
    return (sp.csc_matrix(A) + 1j * sp.diags(20.0 * rng.random(A.shape[0]))).tocsc()


def make_rhs(n, ncol, cmplx, seed=0):
    rng = np.random.default_rng(seed + 2000)
    shape = (n,) if ncol == 0 else (n, ncol)
    b = rng.standard_normal(shape)
    return b + 1j * rng.standard_normal(shape) if cmplx else b


PART_B = {"K27": K27, "P25": P25, "MIX": MIX, "ARROW": ARROW, "TRI1": lambda: TRI(1), "TRI2": lambda: TRI(2),
          "TRI63": lambda: TRI(63), "TRI64": lambda: TRI(64), "TRI65": lambda: TRI(65), "C12": C12, "C14": C14}


def lanes_per_row(A):
    """the rule of factor_impl (csrc/mumps_shim.hip): 4 lanes up to 12 entries per row on average, else 16"""
    return 4 if A.nnz / A.shape[0] <= 12.0 else 16


# ---- the twin -------------------------------------------------------------------------------------------------------
def jacobi_cocg(A, b, tol, maxit=None):
    """Jacobi-preconditioned conjugate-orthogonal CG (unconjugated inner products; plain PCG for real SPD matrices),
    x0 = 0, stopped on ||r|| <= tol ||b|| of the recurrence residual.  b is 1-D or 2-D (columns are independent
    solves run side by side).  Returns (x, iterations of the slowest column, converged: bool per column)."""
    A = sp.csr_matrix(A)
    b = np.asarray(b)
    B = b.reshape(b.shape[0], -1)
    n, m = B.shape
    dt = np.result_type(A.dtype, B.dtype, np.float64)
    dinv = (1.0 / A.diagonal()).astype(dt)[:, None]
    maxit = max(2000, 20 * n) if maxit is None else maxit
    x = np.zeros((n, m), dtype=dt)
    r = B.astype(dt).copy()
    bb = (np.abs(B) ** 2).sum(axis=0)
    live = bb > 0.0
    done = ~live
    z = dinv * r
    p = z.copy()
    rz = (r * z).sum(axis=0)
    it = 0
    while it < maxit:
        rr = (np.abs(r) ** 2).sum(axis=0)
        done = done | (live & (rr <= tol * tol * bb))
        live = live & ~done
        if not live.any():
            break
        q = A @ p
        pq = (p * q).sum(axis=0)
        live = live & (np.abs(pq) > 0.0)             # breakdown: the column stops where it is
        if not live.any():
            break
        alpha = np.where(live, rz / np.where(live, pq, 1.0), 0.0)
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        rz_new = (r * z).sum(axis=0)
        ok = live & (np.abs(rz) > 0.0)
        beta = np.where(ok, rz_new / np.where(ok, rz, 1.0), 0.0)
        live = ok
        rz = rz_new
        p = z + beta * p
        it += 1
    return x.reshape(b.shape), it, (done if b.ndim > 1 else bool(done[0]))
