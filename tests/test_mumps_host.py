"""The MUMPS-wrapper symbols (include/hmcmt_mumps.h) without a device: everything factor_mumps_[cmplx_] checks before its
first HIP call, the handle-taking entry points on a null handle, the wrapper's `x` argument, and the reference module
of the GPU tests (tests/mumps_ref.py) against SuperLU.

No call here passes a non-zero handle: a destroyed or invented one would be a wild pointer, not a test."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from hmcmt2d_amd import mumps as M
from tests import mumps_ref as R

_i64p, _dp = M._i64p, M._dp
NAN = float("nan")


def _raw_factor(cmplx, n, sym, nz, rowval, colptr, with_stat=True):
    """factor_mumps_[cmplx_] with exactly these arrays (1-based, as the caller states them) -> (handle, stat[0])"""
    so = M._so()
    nz = np.ascontiguousarray(nz, dtype=np.complex128 if cmplx else np.float64)
    rowval = np.ascontiguousarray(rowval, dtype=np.int64)
    colptr = np.ascontiguousarray(colptr, dtype=np.int64)
    stat = np.full(1, 77, dtype=np.int64)
    f = so.factor_mumps_cmplx_ if cmplx else so.factor_mumps_
    h = f(M._ref(n), M._ref(sym), M._ref(0), M._ptr(nz, _dp), M._ptr(rowval, _i64p), M._ptr(colptr, _i64p),
          M._ptr(stat, _i64p) if with_stat else None)
    return int(h), int(stat[0])


# a valid 3 x 3 tridiagonal system in 1-based CSC: every case below spoils exactly one thing of it
N3 = 3
NZ3 = [4.0, 1.0, 1.0, 4.0, 1.0, 1.0, 4.0]
ROW3 = [1, 2, 1, 2, 3, 2, 3]
COL3 = [1, 3, 6, 8]

CASES = {
    "n = 0": (dict(n=0), -1),
    "n = 2^31": (dict(n=2 ** 31), -1),
    "sym = 0": (dict(sym=0), -1),
    "sym = 3": (dict(sym=3), -1),
    "0-based colptr": (dict(colptr=[0, 2, 5, 7]), -1),
    "non-monotone colptr": (dict(colptr=[1, 6, 3, 8]), -1),
    "nnz < n": (dict(colptr=[1, 2, 3, 3]), -1),
    "row index 0": (dict(rowval=[1, 2, 0, 2, 3, 2, 3]), -1),
    "row index n + 1": (dict(rowval=[1, 2, 1, 2, 4, 2, 3]), -1),
    "stored zero on the diagonal": (dict(nz=[4.0, 1.0, 1.0, 0.0, 1.0, 1.0, 4.0]), -10),
    "column without a diagonal entry": (dict(rowval=[1, 2, 1, 3, 3, 2, 3]), -10),
}


@pytest.mark.parametrize("cmplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("case", list(CASES))
def test_factor_refuses_bad_input_before_the_device(case, cmplx, capfd):
    """Every check of factor_impl (csrc/mumps_shim.hip) that runs before hipGetDeviceCount: handle 0, the stated
    stat[0], a line on stderr."""
    spoil, want = CASES[case]
    a = dict(n=N3, sym=1, nz=NZ3, rowval=ROW3, colptr=COL3)
    a.update(spoil)
    h, stat = _raw_factor(cmplx, **a)
    assert h == 0 and stat == want, (case, h, stat)
    assert "factor failed" in capfd.readouterr().err


@pytest.mark.parametrize("cmplx", [False, True], ids=["real", "complex"])
def test_factor_with_a_null_stat_returns_zero_without_writing(cmplx):
    h, stat = _raw_factor(cmplx, N3, 1, NZ3, ROW3, COL3, with_stat=False)
    assert h == 0 and stat == 77


@pytest.mark.parametrize("cmplx", [False, True], ids=["real", "complex"])
def test_null_handle_is_refused_by_every_entry_point(cmplx):
    """*handle == 0 (what a failed factor returns): solve / destroy / last_solve return -1, the sparse solves (void)
    return without touching x."""
    so = M._so()
    sfx = "cmplx_" if cmplx else ""
    w = 2 if cmplx else 1
    rhs = np.ones(N3 * w)
    x = np.full(N3 * w, NAN)
    zero = M._ref(0)
    assert getattr(so, f"solve_mumps_{sfx}")(zero, M._ref(1), M._ptr(rhs, _dp), M._ptr(x, _dp), M._ref(0)) == -1
    assert np.isnan(x).all()
    nz = np.ones(w)
    rowval, colptr = np.array([1], dtype=np.int64), np.array([1, 2], dtype=np.int64)
    getattr(so, f"solve_mumps_{sfx}sparse_rhs_")(zero, M._ref(1), M._ref(1), M._ptr(nz, _dp), M._ptr(rowval, _i64p),
                                                  M._ptr(colptr, _i64p), M._ptr(x, _dp), M._ref(0))
    assert np.isnan(x).all()
    assert getattr(so, f"destroy_mumps_{sfx}")(zero) == -1
    out = np.full(3, NAN)
    assert so.hmcmt_mumps_last_solve(zero, M._ptr(out, _dp)) == -1 and np.isnan(out).all()


def test_apply_refuses_an_x_of_the_wrong_size():
    """MUMPSfuncs.jl:89-95: a non-empty x whose size is not the right-hand side's is an error (checked before any call
    into the library, so a factorization object that was never factored serves)."""
    F = M.MUMPSfactorization(0, 5, False)
    with pytest.raises(ValueError, match=r"applyMUMPS: wrong size of x, size\(A\)=5, size\(rhs\)=\(5, 2\), size\(x\)=\(5, 3\) provided"):
        M.applyMUMPS(F, np.ones((5, 2)), np.zeros((5, 3)))
    with pytest.raises(ValueError, match="wrong size of x"):
        M.applyMUMPS(F, np.ones(5), np.zeros((5, 1)))
    with pytest.raises(ValueError, match="wrong size of x"):
        M.applyMUMPS(F, sp.identity(5, format="csc"), np.zeros((5, 4)))
    with pytest.raises(ValueError, match="wrong size of rhs"):
        M.applyMUMPS(F, np.ones(4), np.zeros(4))
    with pytest.raises(TypeError):
        M.applyMUMPS(M.MUMPSfactorization(0, 5, True), np.ones(5), np.zeros(5))


# ---- the reference module itself ------------------------------------------------------------------------------------
def _variants():
    for name, make in R.PART_B.items():
        A = make()
        yield name + "-real", A
        yield name + "-complex", R.complexify(A)


def test_part_b_matrices_are_what_the_cases_say():
    """sizes, fill and the lane count each matrix selects (nnz / n <= 12 -> 4 lanes, else 16), symmetry"""
    want = {"K27": (9261, 24.5, 16), "P25": (182, 20.7, 16), "MIX": (900, 27.2, 16), "ARROW": (3000, 5.0, 4),
            "TRI1": (1, 1.0, 4), "TRI2": (2, 2.0, 4), "TRI63": (63, 2.97, 4), "TRI64": (64, 2.97, 4), "TRI65": (65, 2.97, 4),
            "C12": (256, 12.0, 4), "C14": (256, 14.0, 16)}
    for name, make in R.PART_B.items():
        A = make()
        n, fill, lanes = want[name]
        assert A.shape == (n, n) and abs(A.nnz / n - fill) < 0.05 and R.lanes_per_row(A) == lanes, name
        assert abs(A - A.T).max() == 0.0 and (A.diagonal() != 0).all()
    assert R.C12().nnz == 12 * 256 and R.C14().nnz == 14 * 256           # exactly on / above the threshold
    rows = np.diff(sp.csr_matrix(R.MIX()).indptr)
    assert rows.min() == 1 and rows.max() == 41 and ((rows > 16) & (rows <= 32)).any() and (rows > 32).any()
    assert np.diff(sp.csr_matrix(R.ARROW()).indptr).max() == 3000


def test_true_relres_against_superlu_and_by_hand():
    """true_relres of a SuperLU solution is at rounding level (<= 1e-15 kappa_1); of a solution spoilt by a known
    amount, that amount; per column."""
    assert R.true_relres(sp.csc_matrix([[2.0, 1.0], [1.0, 2.0]]), [1.0, 1.0], [3.0, 3.5]) == pytest.approx(0.5 / np.sqrt(21.25), rel=1e-15)
    for name, A in _variants():
        n = A.shape[0]
        cm = np.iscomplexobj(A.data)
        b = R.make_rhs(n, 3, cm)
        lu = spla.splu(A)
        x = lu.solve(b)
        rr = R.true_relres(A, x, b)
        assert rr.shape == (3,) and (rr <= 1e-15 * R.kappa1(A, lu)).all(), (name, rr)
        assert R.true_relres(A, x[:, 1], b[:, 1])[0] == rr[1]
        d = np.zeros_like(x); d[n // 2, 1] = 1e-6
        want = 1e-6 * np.linalg.norm(A[:, [n // 2]].toarray()) / np.linalg.norm(b[:, 1])
        rr2 = R.true_relres(A, x + d, b)
        assert rr2[0] == rr[0] and rr2[2] == rr[2] and rr2[1] == pytest.approx(want, rel=1e-6)


def test_kappa1_estimate_agrees_with_the_dense_one():
    """onenormest bounds the 1-norm from below (so the forward-error bar it sizes is never wider than the textbook
    one) and is close to it"""
    A = R.complexify(R.P25())
    big = sp.block_diag([A] * 6, format="csc")                             # n = 1092 > 1000: the onenormest branch
    exact = R.kappa1(A)
    assert 0.5 * exact <= R.kappa1(big) <= exact * (1 + 1e-12)


def test_twin_reaches_1e14_on_every_part_b_matrix():
    """jacobi_cocg stopped at 1e-14 converges on every matrix of part B, real and complex, well inside the iteration
    cap (none of the GPU cases is slow or marginal), and its solution's true residual is at that level."""
    for name, A in _variants():
        n = A.shape[0]
        b = R.make_rhs(n, 3, np.iscomplexobj(A.data))
        x, it, ok = R.jacobi_cocg(A, b, 1e-14)
        assert ok.all() and it <= 100, (name, it)
        assert (R.true_relres(A, x, b) <= 1e-13).all(), name
        x1, it1, ok1 = R.jacobi_cocg(A, b[:, 2], 1e-14)
        assert ok1 and np.linalg.norm(x1 - x[:, 2]) <= 1e-12 * np.linalg.norm(x1)     # (columns of a block are independent solves)


def test_twin_breaks_down_where_the_products_vanish():
    """the cases of the breakdown test: p'q = 0 on the first step (real), b' D^-1 b = 0 (complex symmetric)"""
    x, it, ok = R.jacobi_cocg(sp.csc_matrix([[1.0, 1.0], [1.0, 1.0]]), np.array([1.0, -1.0]), 1e-14)
    assert not ok and it == 0 and (x == 0).all()
    x, it, ok = R.jacobi_cocg(sp.csc_matrix([[2.0, 1j], [1j, 2.0]]), np.array([1.0, 1j]), 1e-14)
    assert not ok and np.isfinite(x).all()
    x, it, ok = R.jacobi_cocg(sp.csc_matrix([[2.0, 1j], [1j, 2.0]]), np.array([1.0, 0.0]), 1e-14)
    assert ok and R.true_relres(sp.csc_matrix([[2.0, 1j], [1j, 2.0]]), x, np.array([1.0, 0.0]))[0] < 1e-14
