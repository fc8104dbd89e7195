"""The reference's own MUMPS-wrapper tests (MUMPS/test/testDivGrad.jl, testTwoSystem.jl, testDestroyMUMPS.jl)
replayed against the eight Fortran-convention symbols of include/hmcmt_mumps.h, plus the MT systems of the path.

Tolerance: the reference's direct solver is held to ||Ax - b||/||b|| < 1e-14; the GPU solver behind these symbols is
iterative (Jacobi-COCG + refinement on the true fp64 residual) and is held to 1e-13 on the well-conditioned div-grad
systems and 1e-11 on the MT systems (cells from 100 m to 100 km, air at 1e-8 S/m)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from hmcmt2d_amd import mumps as M
from tests import mumps_ref as R
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu


def ddx(n):
    return sp.diags([-np.ones(n), np.ones(n)], [0, 1], shape=(n, n + 1), format="csc")


def getDivGrad(n1, n2, n3):
    """MUMPS/test/getDivGrad.jl:3-13."""
    e = lambda n: sp.identity(n, format="csc")
    D1 = sp.kron(e(n3), sp.kron(e(n2), ddx(n1)))
    D2 = sp.kron(e(n3), sp.kron(ddx(n2), e(n1)))
    D3 = sp.kron(ddx(n3), sp.kron(e(n2), e(n1)))
    Div = sp.hstack([D1, D2, D3]).tocsc()
    return (Div @ Div.T).tocsc()


def relres(A, x, b):
    x = x.reshape(b.shape)
    if b.ndim == 1:
        return np.linalg.norm(A @ x - b) / np.linalg.norm(b)
    return max(np.linalg.norm(A @ x[:, i] - b[:, i]) / np.linalg.norm(b[:, i]) for i in range(b.shape[1]))


def test_div_grad_real_and_complex_single_and_multiple_rhs():
    """testDivGrad.jl:9-59."""
    rng = np.random.default_rng(0)
    A = getDivGrad(32, 32, 16)
    n = A.shape[0]
    rhs = rng.standard_normal(n)
    x = M.solveMUMPS(A, rhs, 1)
    assert x.dtype == np.float64 and relres(A, x, rhs) < 1e-13
    rhs = rng.standard_normal((n, 10))
    x = M.solveMUMPS(A, rhs, 1)
    assert x.dtype == np.float64 and relres(A, x, rhs) < 1e-13
    Ac = (A + 1j * sp.diags(rng.random(n))).tocsc()
    rhs = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x = M.solveMUMPS(Ac, rhs, 1)
    assert x.dtype == np.complex128 and relres(Ac, x, rhs) < 1e-13
    rhs = rng.standard_normal((n, 10)) + 1j * rng.standard_normal((n, 10))
    x = M.solveMUMPS(Ac, rhs, 2)
    assert x.dtype == np.complex128 and relres(Ac, x, rhs) < 1e-13


def test_two_systems_alive_and_destroy_loop():
    """testTwoSystem.jl:12-51 (a complex and a real factorization alive at once), testDestroyMUMPS.jl:28-35
    (factor/destroy in a loop: nothing leaks, nothing dangles), sparse right-hand sides (MUMPSfuncs.jl:111-146)."""
    rng = np.random.default_rng(1)
    A = getDivGrad(24, 23, 25)
    A2 = getDivGrad(34, 32, 36)
    n, n2 = A.shape[0], A2.shape[0]
    A = (A + 1j * sp.diags(rng.random(n))).tocsc()
    rhs = rng.standard_normal((n, 10)) + 1j * rng.standard_normal((n, 10))
    rhs2 = rng.standard_normal((n2, 10))
    F1 = M.factorMUMPS(A, 1)
    F2 = M.factorMUMPS(A2, 1)
    x = M.applyMUMPS(F1, rhs)
    x2 = M.applyMUMPS(F2, rhs2)
    assert relres(A, x, rhs) < 1e-13 and relres(A2, x2, rhs2) < 1e-13
    S = sp.random(n2, 3, density=5e-4, random_state=3, format="csc")
    xs = M.applyMUMPS(F2, S)
    assert relres(A2, xs, S.toarray()) < 1e-13
    M.destroyMUMPS(F1)
    M.destroyMUMPS(F2)
    assert F1.ptr == -1 and F2.ptr == -1
    Ar = getDivGrad(12, 13, 11)
    for _ in range(100):
        M.destroyMUMPS(M.factorMUMPS(Ar, 1))


def test_mt_systems_of_the_path_match_a_direct_solver():
    """The calls the reference makes on the path (mt2DTE.jl:51-53, compJacTMatVec.jl:224): factorMUMPS(Aii, 1) on the
    complex-symmetric TE / TM systems, forward right-hand side and a second (adjoint-like) one, against SuperLU."""
    from tests.helpers import oracle_eval
    mesh, data, inv, m = make_problem("tiny")
    keep = {}
    oracle_eval(mesh, data, inv, m, keep=keep)
    mats = keep["Aii"]                                     # {(mode, freq): Aii} as the reference assembles them
    assert len(mats) == 2 * len(data.freqs)
    rng = np.random.default_rng(2)
    for key in sorted(mats):
        A = sp.csc_matrix(mats[key])
        n = A.shape[0]
        rhs = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
        F = M.factorMUMPS(A, 1)
        x = M.applyMUMPS(F, rhs)
        st = M.lastSolveStats(F)
        M.destroyMUMPS(F)
        xd = spla.splu(A).solve(rhs)
        assert st["relres"] < 1e-11 and np.abs(x - xd).max() / np.abs(xd).max() < 1e-8


def test_error_codes():
    """MUMPSfuncs.jl:59-73: stat < 0 after factor raises; zero diagonal -> -10 (numerically singular)."""
    A = sp.csc_matrix(np.array([[0.0, 1.0], [1.0, 2.0]]))
    with pytest.raises(RuntimeError, match="singular"):
        M.factorMUMPS(A, 1)
    with pytest.raises(RuntimeError, match="error"):
        M.factorMUMPS(getDivGrad(4, 4, 4), 0)          # unsymmetric mode is not offered


# ======================================================================================================================
# Every kernel instantiation, the interface's contracts and the reference's own call sequence, through the exported
# symbols.  The measure is tests/mumps_ref.py: true_relres (extended-precision residual from the COO triplets) and
# SuperLU; kappa_1 sizes the forward-error bar, nothing here is tuned to what the library returns.
# ======================================================================================================================
_i64p, _dp = M._i64p, M._dp
BAR_B = 1e-13            # well-conditioned systems (the bar of the div-grad tests above)
BAR_MT = 1e-11           # MT systems (the bar of test_mt_systems_of_the_path_match_a_direct_solver)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def nan_array(shape, dt, order="F"):
    """every double of it NaN (real and imaginary parts)"""
    return np.full(shape, complex(np.nan, np.nan) if dt == np.complex128 else np.nan, dtype=dt, order=order)


def all_nan(x):
    return bool(np.isnan(x.real).all() and (not np.iscomplexobj(x) or np.isnan(x.imag).all()))


def assert_truthful(A, b, rc, x):
    """The contract of the return code, checked on every raw solve of this file: 0 => every non-zero column has a
    true residual <= 1e-10 and x is finite; -10 => x is finite.  Nothing else is ever returned for a valid call."""
    assert rc in (0, -10), rc
    assert np.isfinite(x).all(), "non-finite x"
    if rc == 0:
        B, X = b.reshape(b.shape[0], -1), x.reshape(b.shape[0], -1)
        nz = np.abs(B).max(axis=0) > 0
        if nz.any():
            rr = R.true_relres(A, X[:, nz], B[:, nz])
            assert (rr <= 1e-10).all(), f"return code 0 with true residual {rr.max():.3e}"


def raw_solve(F, A, b, kind=None):
    """solve_mumps_[cmplx_] on a NaN-prefilled x -> (return code, x); `kind` picks the symbol regardless of the handle"""
    cm = F.cmplx if kind is None else kind == "complex"
    dt = np.complex128 if cm else np.float64
    nrhs = 1 if b.ndim == 1 else b.shape[1]
    rf = np.asfortranarray(b.reshape(F.n, nrhs), dtype=dt)
    x = nan_array((F.n, nrhs), dt)
    so = M._so()
    f = so.solve_mumps_cmplx_ if cm else so.solve_mumps_
    rc = int(f(M._ref(F.ptr), M._ref(nrhs), M._ptr(rf, _dp), M._ptr(x, _dp), M._ref(0)))
    x = x[:, 0] if b.ndim == 1 else x
    if kind is None:
        assert_truthful(A, b, rc, x)
    return rc, x


def raw_solve_sparse(F, S, kind=None):
    """solve_mumps_[cmplx_]sparse_rhs_ (void) on a NaN-prefilled x -> x"""
    cm = F.cmplx if kind is None else kind == "complex"
    dt = np.complex128 if cm else np.float64
    S = sp.csc_matrix(S).astype(dt)
    S.sort_indices()
    nz = np.ascontiguousarray(S.data)
    rowval = np.ascontiguousarray(S.indices, dtype=np.int64) + 1
    colptr = np.ascontiguousarray(S.indptr, dtype=np.int64) + 1
    x = nan_array((F.n, S.shape[1]), dt)
    so = M._so()
    f = so.solve_mumps_cmplx_sparse_rhs_ if cm else so.solve_mumps_sparse_rhs_
    f(M._ref(F.ptr), M._ref(S.nnz), M._ref(S.shape[1]), M._ptr(nz, _dp), M._ptr(rowval, _i64p), M._ptr(colptr, _i64p),
      M._ptr(x, _dp), M._ref(0))
    return x


@functools.lru_cache(maxsize=None)
def reference(name, cmplx):
    """(A, SuperLU factors, kappa_1) of a part-B matrix: computed once, shared, never modified"""
    A = R.PART_B[name]()
    if cmplx:
        A = R.complexify(A)
    lu = spla.splu(A)
    return A, lu, R.kappa1(A, lu)


def assert_bar_b(tag, A, lu, kappa, F, b, rc, x, cols=None):
    """The bar of part B on the columns `cols` (default: all) of one solve; prints every figure before asserting.

      true_relres < 1e-13 per column; the library's reported residual is the true one (0.1 relative + 1e-15);
      return code 0; x within the textbook forward-error bound of SuperLU's solution x_d in the 1-norm:
      |x - x*| / |x*| <= kappa_1 |b - A x| / |b| for the exact x*, all norms the 1-norm (a 2-norm residual in a 1-norm
      bound is off by the vectors' shape, which shows at n = 2), applied to both solutions -- SuperLU's own residual is
      of the same size as the library's -- and referred to |x_d| instead of |x*|."""
    B, X = b.reshape(b.shape[0], -1), x.reshape(b.shape[0], -1)
    cols = list(range(B.shape[1])) if cols is None else cols
    B, X = B[:, cols], X[:, cols]
    rr = R.true_relres(A, X, B)
    st = M.lastSolveStats(F)
    XD = lu.solve(B)
    r1, d1 = R.true_relres(A, X, B, ord=1), R.true_relres(A, XD, B, ord=1)
    bound = kappa * (r1 + d1) / (1.0 - kappa * d1)
    err = np.abs(X - XD).sum(axis=0) / np.abs(XD).sum(axis=0)
    print(f"{tag}: n {A.shape[0]} rc {rc} true_relres {rr.max():.2e} reported {st['relres']:.2e} iters {st['iterations']} "
          f"passes {st['refinement_passes']} fwd err {err.max():.2e} of bound {bound.min():.2e} kappa1 {kappa:.1f}")
    assert rc == 0
    assert (rr < BAR_B).all(), rr
    assert abs(st["relres"] - rr.max()) <= 0.1 * rr.max() + 1e-15, (st["relres"], rr.max())
    assert (err <= bound).all(), (err, bound)
    return float(rr.max())


# ---- B. every kernel instantiation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cmplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name", list(R.PART_B))
def test_every_kernel_instantiation_against_the_direct_solver(name, cmplx):
    """k_sp_resid / k_sp_dir with 4 and 16 lanes per row, real and complex, at the shapes where they can go wrong:
    K27 (16 lanes, second grid-stride pass, last block 13 of 16 rows), P25 (16 lanes, one pass, ragged last block), MIX
    (16 lanes, rows of 1 beside rows of 21..41), ARROW (4 lanes, one row of 3000), TRI (4 lanes, n = 1, 2 and around one
    64-row block), C12 / C14 (the two sides of the lane rule on nearly the same matrix, same right-hand side).  One
    right-hand side and a block of three."""
    A, lu, kappa = reference(name, cmplx)
    n = A.shape[0]
    assert R.lanes_per_row(A) == {"K27": 16, "P25": 16, "MIX": 16, "C14": 16}.get(name, 4)
    F = M.factorMUMPS(A, 1)
    try:
        for ncol in (0, 3):
            b = R.make_rhs(n, ncol, cmplx)
            rc, x = raw_solve(F, A, b)
            assert_bar_b(f"B {name} {'complex' if cmplx else 'real'} nrhs {max(ncol, 1)}", A, lu, kappa, F, b, rc, x)
    finally:
        M.destroyMUMPS(F)


# ---- C. contracts of the interface ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cmplx", [("K27", True), ("ARROW", False)], ids=["K27-complex", "ARROW-real"])
def test_block_equals_alone_sparse_equals_dense_and_repeats_bitwise(name, cmplx):
    """C1: nothing is carried from one right-hand side to the next (p0 / p1 / rho / flag / partial sums), and the
    kernels reduce in a fixed order: column j of a block == the same column alone == a repeat == the sparse-rhs call
    on the same numbers, bit for bit."""
    A, lu, kappa = reference(name, cmplx)
    n = A.shape[0]
    b = R.make_rhs(n, 3, cmplx, seed=7)
    b[:: 3, 1] = 0.0                                    # (a genuinely sparse middle column)
    F = M.factorMUMPS(A, 1)
    try:
        rc, X = raw_solve(F, A, b)
        assert rc == 0
        for j in (2, 0, 1):                             # (not in the block's order)
            rcj, xj = raw_solve(F, A, b[:, j].copy())
            assert rcj == 0 and np.array_equal(bits(xj), bits(X[:, j])), f"column {j} alone differs from the block"
        rc2, X2 = raw_solve(F, A, b)
        assert rc2 == 0 and np.array_equal(bits(X2), bits(X)), "a repeat differs"
        S = sp.csc_matrix(b)
        assert S.nnz < b.size
        XS = raw_solve_sparse(F, S)
        assert np.array_equal(bits(XS), bits(X)), "sparse right-hand side differs from the dense one"
    finally:
        M.destroyMUMPS(F)


@pytest.mark.parametrize("name,cmplx", [("P25", True), ("TRI65", False)], ids=["P25-complex", "TRI65-real"])
def test_zero_column_gives_exact_zero_and_x_argument_is_filled(name, cmplx):
    """C2: a block whose middle column is zero, x prefilled with NaN through the raw symbol: the middle column of x is
    exactly 0, the outer ones meet the bar, return code 0; the same for a sparse right-hand side with an empty
    column; applyMUMPS(x=...) fills and returns the caller's array."""
    A, lu, kappa = reference(name, cmplx)
    n = A.shape[0]
    b = R.make_rhs(n, 3, cmplx, seed=11)
    b[:, 1] = 0.0
    F = M.factorMUMPS(A, 1)
    try:
        rc, X = raw_solve(F, A, b)
        assert (bits(X[:, 1]) == 0).all(), "zero right-hand side: x is not exactly +0"
        assert_bar_b(f"C2 {name} dense", A, lu, kappa, F, b, rc, X, cols=[0, 2])
        S = sp.csc_matrix(b)
        assert S.indptr[1] == S.indptr[2]                                   # (an empty column)
        XS = raw_solve_sparse(F, S)
        assert (bits(XS[:, 1]) == 0).all() and np.array_equal(bits(XS), bits(X))
        assert_bar_b(f"C2 {name} sparse", A, lu, kappa, F, b, 0, XS, cols=[0, 2])
        dt = X.dtype
        for x in (nan_array((n, 3), dt, "F"), nan_array((n, 3), dt, "C")):
            out = M.applyMUMPS(F, b, x)
            assert out is x and np.array_equal(bits(x), bits(X))
        x1 = nan_array(n, dt)
        assert M.applyMUMPS(F, b[:, 2], x1) is x1 and np.array_equal(bits(x1), bits(X[:, 2]))
        xs = nan_array((n, 3), dt)
        assert M.applyMUMPS(F, S, xs) is xs and np.array_equal(bits(xs), bits(X))
        assert np.array_equal(bits(M.applyMUMPS(F, b, np.zeros(0))), bits(X))   # (an empty x is replaced)
        with pytest.raises(ValueError, match="wrong size of x"):
            M.applyMUMPS(F, b, np.zeros((n, 2), dtype=dt))
    finally:
        M.destroyMUMPS(F)


@pytest.mark.parametrize("cmplx", [False, True], ids=["real", "complex"])
def test_scaling_the_system_or_the_right_hand_side_changes_nothing(cmplx):
    """C3: b * 2^+-200 and A * 2^+-100 on P25, each held to the bar against its own right-hand side: no absolute
    threshold hides in a kernel or in the refinement loop (kappa_1 does not change with the scale)."""
    A, lu, kappa = reference("P25", cmplx)
    n = A.shape[0]
    b = R.make_rhs(n, 3, cmplx, seed=13)
    F = M.factorMUMPS(A, 1)
    try:
        for e in (200, -200):
            bs = b * 2.0 ** e
            rc, x = raw_solve(F, A, bs)
            assert_bar_b(f"C3 b*2^{e}", A, lu, kappa, F, bs, rc, x)
    finally:
        M.destroyMUMPS(F)
    for e in (100, -100):
        As = (A * 2.0 ** e).tocsc()
        F = M.factorMUMPS(As, 1)
        try:
            rc, x = raw_solve(F, As, b)
            assert_bar_b(f"C3 A*2^{e}", As, spla.splu(As), kappa, F, b, rc, x)
        finally:
            M.destroyMUMPS(F)


def test_return_code_is_truthful_on_breakdown():
    """C4: arithmetic breakdowns of COCG end in a status code, never in a wrong or non-finite x.

      [[1,1],[1,1]] x = (1,-1), real     p'q = 0 on the first step           -> -10, x = 0, reported residual 1
      [[1,1],[1,1]] x = (1, 1)           consistent                          ->   0, x = (1/2, 1/2)
      [[2,i],[i,2]] x = (1, i), complex  b' D^-1 b = 0: first step length 0,
                                         the next beta is 0 / 0              -> -10, x finite, reported residual 1
                                         (perfectly conditioned: a direct solver succeeds)
      the same A, b = (1, 0)                                                 ->   0, the bar of part B
      blockdiag(K, -K), K = tridiag(-1, 4, -1) of size 50, sym = 2 (real indefinite): only the contract of the code"""
    S2 = sp.csc_matrix(np.array([[1.0, 1.0], [1.0, 1.0]]))
    F = M.factorMUMPS(S2, 1)
    try:
        rc, x = raw_solve(F, S2, np.array([1.0, -1.0]))
        st = M.lastSolveStats(F)
        print(f"C4 singular inconsistent: rc {rc} x {x} reported {st['relres']} iters {st['iterations']}")
        assert rc == -10 and (x == 0).all() and st["relres"] == 1.0
        rc, x = raw_solve(F, S2, np.array([1.0, 1.0]))
        print(f"C4 singular consistent: rc {rc} x {x}")
        assert rc == 0 and np.abs(x - 0.5).max() <= 1e-15
    finally:
        M.destroyMUMPS(F)
    Ci = sp.csc_matrix(np.array([[2.0, 1j], [1j, 2.0]]))
    F = M.factorMUMPS(Ci, 1)
    try:
        rc, x = raw_solve(F, Ci, np.array([1.0, 1j]))
        st = M.lastSolveStats(F)
        print(f"C4 complex breakdown: rc {rc} x {x} reported {st['relres']} iters {st['iterations']}")
        assert rc == -10 and np.isfinite(x).all() and st["relres"] == 1.0
        b = np.array([1.0 + 0j, 0.0])
        rc, x = raw_solve(F, Ci, b)
        assert_bar_b("C4 complex (1,0)", Ci, spla.splu(Ci), R.kappa1(Ci), F, b, rc, x)
    finally:
        M.destroyMUMPS(F)
    K = R.tridiag(50, -1.0, 4.0)
    Ind = sp.block_diag([K, -K], format="csc")
    F = M.factorMUMPS(Ind, 2)
    try:
        for ncol in (0, 3):
            b = R.make_rhs(100, ncol, False, seed=17)
            rc, x = raw_solve(F, Ind, b)                    # (asserts the contract)
            st = M.lastSolveStats(F)
            print(f"C4 indefinite nrhs {max(ncol, 1)}: rc {rc} true_relres {R.true_relres(Ind, x, b).max():.2e} "
                  f"reported {st['relres']:.2e} iters {st['iterations']}")
    finally:
        M.destroyMUMPS(F)


def test_solve_of_the_wrong_kind_is_refused_and_leaves_x_alone():
    """C5: solve_mumps_ on a complex handle and solve_mumps_cmplx_ on a real one return -1 and leave the NaN-prefilled
    x untouched; the sparse variants return without touching x.  (Buffers are sized for the larger kind.)"""
    A = R.TRI(65)
    Fr, Fc = M.factorMUMPS(A, 1), M.factorMUMPS(R.complexify(A), 1)
    try:
        b = R.make_rhs(65, 3, True)
        for F, kind in ((Fr, "complex"), (Fc, "real")):
            bb = b if kind == "complex" else np.concatenate([b.real, b.imag])          # 2 n doubles per column either way
            F2 = M.MUMPSfactorization(F.ptr, bb.shape[0], F.cmplx)
            rc, x = raw_solve(F2, None, bb, kind=kind)
            assert rc == -1 and all_nan(x)
            xs = raw_solve_sparse(F2, sp.csc_matrix(bb), kind=kind)
            assert all_nan(xs)
        rc, x = raw_solve(Fr, A, b.real.copy())                                        # both handles still work
        assert rc == 0
        rc, x = raw_solve(Fc, R.complexify(A), b)
        assert rc == 0
    finally:
        M.destroyMUMPS(Fr)
        M.destroyMUMPS(Fc)


# ---- D. the reference's own call sequence ---------------------------------------------------------------------------
class _Factors:
    """What `lu(Aii)` / `factorMUMPS(Aii, 1)` returns to the oracle: .solve(b) for 1-D and 2-D b, every call counted."""

    def __init__(self, log, A):
        self.A, self.log = sp.csc_matrix(A), log
        log["factor"] += 1

    def solve(self, b):
        self.log["solve"].append(np.shape(b))
        return self._solve(np.asarray(b))


class _SuperLU(_Factors):
    def __init__(self, log, A):
        super().__init__(log, A)
        self.lu = spla.splu(self.A)

    def _solve(self, b):
        return self.lu.solve(b)


class _Twin(_Factors):
    def _solve(self, b):
        x, it, ok = R.jacobi_cocg(self.A, b, BAR_MT)
        assert np.all(ok)
        return x


class _Mumps(_Factors):
    """mt2DTE.jl:51-53: Ainv = factorMUMPS(Aii, 1), applyMUMPS(Ainv, rhs); the handle stays alive until the test
    destroys it (HMCSampler.jl:312-325)."""

    def __init__(self, log, A):
        super().__init__(log, A)
        self.F = M.factorMUMPS(self.A, 1)
        log["handles"].append(self.F)

    def _solve(self, b):
        x = M.applyMUMPS(self.F, b)
        st = M.lastSolveStats(self.F)
        rr = R.true_relres(self.A, x, b)
        self.log["relres"] = max(self.log["relres"], float(rr.max()))
        self.log["iters"] = max(self.log["iters"], st["iterations"])       # (of a block: its last column's)
        assert x.shape == b.shape and (rr <= BAR_MT).all(), f"true residual {rr.max():.3e} (reported {st['relres']:.3e})"
        return x


class _Proxy:
    """scipy.sparse.linalg with `splu` replaced, for the oracle module only"""

    def __init__(self, kind):
        self.log = {"factor": 0, "solve": [], "handles": [], "relres": 0.0, "iters": 0}
        self._kind = kind

    def __getattr__(self, name):
        return getattr(spla, name)

    def splu(self, A):
        return self._kind(self.log, A)


def _replay(monkeypatch, kind, problem, jac):
    from oracle import hmcmt_oracle as O
    from hmcmt2d_amd.structs import HMCPrior
    mesh, data, inv, m = problem()
    proxy = _Proxy(kind)
    monkeypatch.setattr(O, "spla", proxy)
    out = {}
    try:
        if not mesh.setup:
            O.setupTensorMesh2D(mesh)
        inv.strModel = np.asarray(m, dtype=float).copy()
        out["pred"], out["misfit"], out["grad"] = O.compDataGradient(mesh, data, inv, HMCPrior(), False)
        nsys = len(data.freqs) * (int(bool(data.compTE)) + int(bool(data.compTM)))
        assert proxy.log["factor"] == nsys
        if kind is _Mumps:                                   # all handles of the evaluation alive at once, all distinct
            assert len({F.ptr for F in proxy.log["handles"]}) == nsys and all(F.ptr > 0 for F in proxy.log["handles"])
        out["calls"] = (proxy.log["factor"], list(proxy.log["solve"]))
        if jac:                                              # compJacMat.jl:211,286: a dense block per system
            handles, proxy.log["handles"] = proxy.log["handles"], []
            for F in handles:
                M.destroyMUMPS(F)
            pred, fwd = O.MT2DFwdSolver(mesh, data)
            out["J"] = O.compJacMat(mesh, data, inv.activeIdx, fwd)
            out["calls_jac"] = (proxy.log["factor"], list(proxy.log["solve"]))
    finally:
        handles = proxy.log["handles"]
        for F in handles:                                    # HMCSampler.jl:312-325
            M.destroyMUMPS(F)
        monkeypatch.setattr(O, "spla", spla)
    assert all(F.ptr == -1 for F in handles) and (kind is not _Mumps or len(handles) == nsys)
    out["mesh"], out["inv"], out["log"] = mesh, inv, proxy.log
    return out


def _replay_errors(run, ref):
    from tests.helpers import gerr_split, relmax
    e = {"pred": relmax(run["pred"], ref["pred"]), "misfit": abs(run["misfit"] - ref["misfit"]) / abs(ref["misfit"])}
    e["grad shallow"], e["grad deep"] = gerr_split(run["grad"], ref["grad"], ref["inv"], ref["mesh"])
    if "J" in ref:
        e["J"] = relmax(run["J"], ref["J"])
    return e


def _problems():
    from tests.helpers import ragged_problem, rhophase_problem
    return {"tiny": lambda: make_problem("tiny"), "ragged": lambda: ragged_problem(17, 9, 1, 3, 3, 2),
            "rhophase": lambda: rhophase_problem("tiny")[:4], "cfg2": lambda: make_problem("cfg2")}


@pytest.mark.parametrize("name", ["tiny", "ragged", "rhophase", "cfg2"])
def test_reference_call_sequence_through_the_mumps_symbols(name, monkeypatch):
    """INTEGRATION section 6's claim: the oracle's compDataGradient (and, on tiny, compJacMat) with its direct solves
    replaced by factorMUMPS(Aii, 1) / applyMUMPS exactly as mt2DTE.jl:51-53, compJacTMatVec.jl:224,295 and
    compJacMat.jl:211,286 call them -- all 2 nFreq handles alive at once, forward solves, adjoint solves on the stored
    handles, dense blocks, destroyMUMPS on each.  Every solve is held to true_relres <= 1e-11.

    Parity with the SuperLU oracle (predicted data, misfit, gradient shallow / deep, J): how far a residual moves the
    data depends on each system's conditioning, so the bars are made at run time from the reference side -- the same
    replay with the numpy twin of the algorithm stopped at 1e-11; the GPU replay's errors must be within 4x the twin's
    (the 4 covers the dependence on the residual's direction)."""
    problem, jac = _problems()[name], name == "tiny"
    ref = _replay(monkeypatch, _SuperLU, problem, jac)
    twin = _replay(monkeypatch, _Twin, problem, jac)
    gpu = _replay(monkeypatch, _Mumps, problem, jac)
    assert gpu["calls"] == ref["calls"] == twin["calls"]
    if jac:
        assert gpu["calls_jac"] == ref["calls_jac"] and any(len(s) == 2 and s[1] > 50 for s in ref["calls_jac"][1])
    bars, errs = _replay_errors(twin, ref), _replay_errors(gpu, ref)
    print(f"D {name}: systems {ref['calls'][0]} solves {len(ref['calls'][1])} worst true_relres {gpu['log']['relres']:.2e} "
          f"most iterations of one solve {gpu['log']['iters']:.0f}")
    for k in bars:
        print(f"D {name}: {k}: error {errs[k]:.2e}, twin at 1e-11 {bars[k]:.2e}")
    for k in bars:
        assert errs[k] <= 4.0 * bars[k], (k, errs[k], bars[k])
