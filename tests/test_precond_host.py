"""The independent reference of the operator and the preconditioner (tests/precond_ref.py: the oracle's assembled matrix, a sparse
LU of the separable background) against itself and against the host instantiation of the kernel bodies (tests/emul),
at every shape tests/test_gpu_precond.py runs on the device.  No GPU involved.

Bars: q = A p to 16 eps componentwise, |dq_i| <= 16 eps (|A| |p|)_i -- derived: a row is five complex multiply-adds, and the two
sides assemble the coefficients in different orders.  Everything else: four times the largest value measured on the host
(the table in DESIGN 4.2; the factor covers another libm or BLAS), never above 1e-9."""
import numpy as np
import pytest

from tests.emul.emul_py import Emul
from tests import precond_ref as R

SHAPE_NAMES = list(R.SHAPES)

# measured (host column), largest over systems and the three vectors; the assertions allow four times as much
MEASURED = {
    #          F_modal(V_lib)  emul fdm   emul fdmj  backward error  M-orthonormality  eigen-residual
    #          vs F_exact      vs ref     vs ref     of emul fdm     of V              of (V, lam)
    "cfg2":   (1.45e-12, 5.94e-12, 5.87e-12, 1.59e-14, 2.00e-15, 2.42e-16),
    "w301":   (2.08e-13, 2.51e-13, 2.51e-13, 2.85e-14, 3.55e-15, 5.42e-16),
    "w100":   (1.93e-13, 2.49e-13, 2.48e-13, 1.54e-14, 3.00e-15, 3.01e-16),
    "w200":   (1.24e-13, 1.60e-13, 1.60e-13, 2.74e-14, 2.66e-15, 4.10e-16),
    "w405":   (3.58e-13, 3.99e-13, 3.97e-13, 8.91e-15, 3.66e-15, 3.21e-16),
    "w270":   (2.21e-13, 2.65e-13, 2.61e-13, 9.80e-15, 3.33e-15, 1.76e-16),
    "slab16": (8.76e-14, 1.06e-13, 1.06e-13, 1.77e-15, 2.00e-15, 1.12e-16),
}


def bar(name, col):
    return min(4.0 * MEASURED[name][col], 1e-9)


_cache = {}


def setup(name):
    """(ref, emulation at the model, V of the emulation [node][mode], the three vectors, interior views): once per shape"""
    if name not in _cache:
        mesh, data, inv, m, ref = R.reference(name)
        E = Emul(mesh, data, inv)
        E.grad(m, False, 2, 1e-12, 1)                                    # (sets the model's coefficients and pivots; one iteration)
        ny, nz = ref.ny, ref.nz
        V = E.get("Vpad").reshape(E.NYP, E.NYP)[1:ny, :ny - 1].copy()
        rows, cols = R.seams(ny, nz, E.NYP)
        vecs = R.make_vectors(E.S, E.NZP, E.NYP, ny, nz, rows, cols)
        _cache[name] = (ref, E, V, vecs)
    return _cache[name]


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_modal_form_with_the_librarys_basis_is_the_exact_fdm_stage(name):
    """F_modal(V_lib) -- Rayleigh quotients of the library's eigenvectors, one LAPACK tridiagonal solve per mode -- against the
    sparse LU of P: two routes to P^-1 that share nothing but the mesh."""
    ref, E, V, vecs = setup(name)
    worst = 0.0
    for s in range(ref.S):
        Fm, Fe = ref.F_modal(s, V), ref.F_exact(s)
        for v in vecs.values():
            t = ref.interior(v[s])
            worst = max(worst, R.relmax(Fm(t), Fe(t)))
    print(f"[host] {name}: F_modal(V_lib) vs F_exact {worst:.2e}")
    assert worst < bar(name, 0)


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_emulated_operator_is_the_oracles_matrix(name):
    ref, E, V, vecs = setup(name)
    worst = 0.0
    for v in vecs.values():
        q = E.apply("spmv", v).reshape(v.shape)
        for s in range(ref.S):
            p = ref.interior(v[s])
            worst = max(worst, ref.spmv_error(s, p, ref.interior(q[s])))
        assert np.isfinite(q).all()
        outside = q.copy()
        outside[:, 1:ref.nz, 1:ref.ny] = 0
        assert not outside.any()
    print(f"[host] {name}: spmv componentwise {worst:.2f} eps")
    assert worst <= 16.0


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_emulated_preconditioners_are_the_references(name):
    """`fdm` (F alone) and `fdmj` (one damped Jacobi sweep on each side) of the emulation -- the item code the kernels inline: the
    geometric row means, the twisted pivots, the host's eigenbasis -- against the reference; and the backward error of `fdm`."""
    ref, E, V, vecs = setup(name)
    worst = [0.0, 0.0, 0.0]
    for v in vecs.values():
        zf, zj = E.apply("fdm", v).reshape(v.shape), E.apply("fdmj", v).reshape(v.shape)
        assert np.isfinite(zf).all() and np.isfinite(zj).all()              # (a NaN would drop out of the max below)
        for s in range(ref.S):
            r = ref.interior(v[s])
            F = ref.F_exact(s)
            worst[0] = max(worst[0], R.relmax(ref.interior(zf[s]), ref.precond(s, r, F, 0)))
            worst[1] = max(worst[1], R.relmax(ref.interior(zj[s]), ref.precond(s, r, F, 1)))
            worst[2] = max(worst[2], ref.backward_error(s, ref.interior(zf[s]), r))
    print(f"[host] {name}: fdm {worst[0]:.2e} fdmj {worst[1]:.2e} backward error of fdm {worst[2]:.2e}")
    assert worst[0] < bar(name, 1) and worst[1] < bar(name, 2) and worst[2] < bar(name, 3)


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_eigenbasis_at_every_width(name):
    """tests/test_kernel_math.py::test_fdm_eigenbasis's two assertions -- V' My V = I, Ty V = My V diag(lam) -- at every width used
    here (the host's implicit-QL iteration up to 404 modes), and the library's eigenvalues against the Rayleigh quotients the
    reference uses in their place."""
    ref, E, V, vecs = setup(name)
    n = ref.ny - 1
    lam = E.get("lam")[:n]
    Ty, my = ref.Ty.toarray(), ref.my
    ortho = float(np.abs(V.T @ (my[:, None] * V) - np.eye(n)).max())
    resid = float(np.abs(Ty @ V - (my[:, None] * V) * lam).max() / np.abs(Ty).max())
    rq = float(np.abs(ref.rayleigh(V) / lam - 1).max())
    print(f"[host] {name}: {n} modes, M-orthonormality {ortho:.2e} eigen-residual {resid:.2e} Rayleigh quotients vs lam {rq:.2e}")
    assert ortho < bar(name, 4) and resid < bar(name, 5)
    assert ortho < 1e-12 and resid < 1e-12                       # (the bars of test_fdm_eigenbasis)


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_rounding_the_basis_to_bf16_moves_the_fdm_stage_by_parts_per_thousand(name):
    """The premise of the modelled reference tests/test_gpu_precond.py holds the mixed-precision kernels to: bf16(V) in place of V,
    everything else exact, moves F by 1e-4 .. 1e-2 (the range tests/test_gpu_parity.py asserts for the transform alone) -- far
    above the fp32-class rounding of the kernels, so a reference with the exact V could hold them at the per-cent level only."""
    ref, E, V, vecs = setup(name)
    d = R.bf16_distance(ref, V, vecs["random"])
    print(f"[host] {name}: bf16(V) vs V, F stage, per system {' '.join(f'{x:.2e}' for x in d)}")
    assert 1e-4 < min(d) and max(d) < 1e-2
