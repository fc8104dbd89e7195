"""The solve's operator q = A p and preconditioner z = P^-1 r, every kernel variant, against the independent reference of
tests/precond_ref.py (the oracle's assembled matrix; a sparse LU of the separable background) -- the anchor of the chain
of sibling comparisons in tests/test_gpu_parity.py, test_gpu_sweeps.py and test_gpu_persist.py, which compare the kernels with each
other and with the host instantiation of the same item source.

  a. hmcmt_debug_spmv against the oracle's Aii: 16 eps componentwise (five complex multiply-adds per row, coefficients assembled in
     another order) -- the stencil that options.verify's true residual is formed with.
  b. the fp64 FDM path (plain FDM, one and two sweeps per side) against the exact reference F_exact.
  c. the mixed-precision launch-per-phase path, fused and separate kernels, narrow and wide meshes,
  d. every variant of the persistent kernel through hmcmt_debug_persist_precond,
     against the MODELLED reference F_modal(bf16(V_lib)): the kernels round the eigenvector matrix to bfloat16 by design, which moves
     the operator by 2e-3 .. 3e-3 (tests/test_precond_host.py); with that one approximation in the reference too, what is left is
     their fp32-class arithmetic (split-bf16 operands with ~16 bits, complex64 tridiagonals, complex64 smoother in the persistent
     kernel) and can be held a hundred times tighter than the approximation itself.

Bars of b, c, d: four times the value measured on an MI355X (the tables below and in DESIGN 4.2), and -- a condition, not a
measurement -- for c and d never above a tenth of the shape's bf16(V)-against-V distance; for b never above 1e-9.  Every test says
from persist_info / persist_width / dims which kernel it measured and fails if that is not the intended one."""
import numpy as np
import pytest

from hmcmt2d_amd.lib import HipContext, persist_envelope
from tests import precond_ref as R

pytestmark = pytest.mark.gpu

_ENV = ("HMCMT_PERSIST", "HMCMT_SWEEPS", "HMCMT_PERSIST_CS", "HMCMT_PERSIST_WIDTHK", "HMCMT_PERSIST_STRIPS", "HMCMT_FUSED_FWD",
        "HMCMT_FUSED_BACK", "HMCMT_TWIST", "HMCMT_JACOBI_W", "HMCMT_VLO")


def _open(monkeypatch, name, env=None, sweeps=None, **kw):
    """a context on shape `name` with the launch-per-phase loop for its evaluations (the persistent kernel's preconditioner is reached
    through its own hook), one forward evaluation at the shape's model"""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HMCMT_PERSIST", "0")
    if sweeps:
        monkeypatch.setenv("HMCMT_SWEEPS", str(sweeps))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    mesh, data, inv, m, ref = R.reference(name)
    ctx = HipContext(mesh, data, inv, **kw)
    ctx.forward(m)
    assert (ctx.ny, ctx.nz, ctx.S) == (ref.ny, ref.nz, ref.S)
    return ctx, ref, m


def _lib_V(ctx):
    """the library's eigenvector matrix [node][mode]: the rows of the identity through the fp64 transform kernel"""
    rows = ctx.S * ctx.NZP
    Vpad = np.zeros((ctx.NYP, ctx.NYP))
    for k0 in range(0, ctx.NYP, rows):
        A = np.zeros((rows, ctx.NYP), complex)
        n = min(rows, ctx.NYP - k0)
        A[np.arange(n), k0 + np.arange(n)] = 1.0
        C = ctx.debug_transform(0, A).reshape(rows, ctx.NYP)
        assert not C.imag.any()
        Vpad[k0:k0 + n] = C[:n].real
    return Vpad[1:ctx.ny, :ctx.ny - 1].copy()


def _vectors(ctx, info):
    cs = info["column_parts"]
    blocks = info["workgroups_per_system"] // max(cs, 1) if cs else None
    if blocks is not None:
        assert blocks == -(-(ctx.nz - 1) // R.PS_OWN), info                      # (the row blocks the seams are computed from)
    rows, cols = R.seams(ctx.ny, ctx.nz, ctx.NYP, blocks, cs) if blocks else R.seams(ctx.ny, ctx.nz, ctx.NYP)
    vecs = R.make_vectors(ctx.S, ctx.NZP, ctx.NYP, ctx.ny, ctx.nz, rows, cols)
    return vecs, R.seam_mask(ctx.NZP, ctx.NYP, ctx.ny, ctx.nz, blocks, cs)


def _nothing_outside(ctx, z):
    """finite everywhere (a NaN would drop out of every max below), zero on boundary and padding nodes"""
    if not np.isfinite(z).all():
        return False
    out = np.array(z, copy=True)
    out[:, 1:ctx.nz, 1:ctx.ny] = 0
    return not out.any()


# ---- a. the operator ----

@pytest.mark.parametrize("name", ["cfg2", "w405", "w270"])
def test_operator_is_the_oracles_matrix(monkeypatch, name):
    ctx, ref, m = _open(monkeypatch, name)
    try:
        vecs, _ = _vectors(ctx, ctx.persist_info())
        shape = (ctx.S, ctx.NZP, ctx.NYP)
        worst = 0.0
        for v in vecs.values():
            q = ctx.debug_spmv(v).reshape(shape)
            assert _nothing_outside(ctx, q)
            for s in range(ctx.S):
                p = ref.interior(v[s])
                worst = max(worst, ref.spmv_error(s, p, ref.interior(q[s])))
    finally:
        ctx.close()
    print(f"[gpu] spmv {name}: {worst:.2f} eps componentwise")
    assert worst <= 16.0


# ---- b. the fp64 FDM path against the exact reference ----

# measured on an MI355X: (largest relmax over systems and vectors, backward error of plain FDM or None)
MEASURED_FP64 = {
    ("cfg2", "fdm"): (3.86e-12, 1.41e-14), ("cfg2", "fdmj1"): (3.85e-12, None), ("cfg2", "fdmj2"): (3.84e-12, None),
    ("w100", "fdm"): (2.47e-13, 1.54e-14), ("w100", "fdmj1"): (2.47e-13, None), ("w100", "fdmj2"): (2.46e-13, None),
    ("w200", "fdm"): (1.62e-13, 2.74e-14), ("w200", "fdmj1"): (1.63e-13, None), ("w200", "fdmj2"): (1.62e-13, None),
    ("w405", "fdm"): (4.00e-13, 8.88e-15), ("w405", "fdmj1"): (3.97e-13, None), ("w405", "fdmj2"): (3.98e-13, None),
}


@pytest.mark.parametrize("name,kind", list(MEASURED_FP64))
def test_fp64_preconditioner_is_the_exact_reference(monkeypatch, name, kind):
    """fdm_precision = fp64 on the launch-per-phase loop: plain FDM (k_transform, k_thomas), one sweep per side (k_pre, k_mid,
    k_post), two (k_sweep_exp) -- against F_exact wrapped in the reference's own smoother.  405 + 1 <= 448 nodes: the widest mesh
    the fp64 transform holds is covered."""
    sweeps = {"fdm": 0, "fdmj1": 1, "fdmj2": 2}[kind]
    ctx, ref, m = _open(monkeypatch, name, sweeps=max(sweeps, 1), fdm_precision="fp64", precond="fdm" if sweeps == 0 else "fdmj")
    try:
        vecs, _ = _vectors(ctx, ctx.persist_info())
        shape = (ctx.S, ctx.NZP, ctx.NYP)
        worst, back = 0.0, 0.0
        for v in vecs.values():
            z = ctx.debug_precond(v).reshape(shape)
            assert _nothing_outside(ctx, z)
            for s in range(ctx.S):
                r = ref.interior(v[s])
                worst = max(worst, R.relmax(ref.interior(z[s]), ref.precond(s, r, ref.F_exact(s), sweeps)))
                if sweeps == 0:
                    back = max(back, ref.backward_error(s, ref.interior(z[s]), r))
    finally:
        ctx.close()
    print(f"[gpu] fp64 {name} {kind}: relmax {worst:.2e}" + (f" backward error {back:.2e}" if sweeps == 0 else ""))
    meas, mback = MEASURED_FP64[(name, kind)]
    assert worst < min(4 * meas, 1e-9)
    if sweeps == 0:
        assert back < min(4 * mback, 1e-9)


# ---- c, d. the mixed-precision kernels against the modelled reference ----

def _compare_mixed(ctx, ref, name, apply, sweeps, label, measured):
    """apply(v) -> z for the three vectors, against precond(F_modal(bf16(V_lib))); per system kind (TE, TM) the largest relmax"""
    info = ctx.persist_info()
    vecs, mask = _vectors(ctx, info)
    shape = (ctx.S, ctx.NZP, ctx.NYP)
    V = _lib_V(ctx)
    Vb = R.bf16(V)
    ceiling = 0.1 * min(R.bf16_distance(ref, V, vecs["random"]))
    F = [ref.F_modal(s, Vb, V) for s in range(ctx.S)]
    worst, seam, where = [0.0, 0.0], [0.0, 0.0], ["", ""]
    for vn, v in vecs.items():
        z = apply(v).reshape(shape)
        assert _nothing_outside(ctx, z)
        for s in range(ctx.S):
            zr = ref.pack(ref.precond(s, ref.interior(v[s]), F[s], sweeps)[None], ctx.NZP, ctx.NYP)[0]
            k = int(s >= ctx.nFreq)
            e = R.relmax(z[s], zr)
            if e > worst[k]:
                worst[k], where[k] = e, f"system {s} vector {vn}"
            seam[k] = max(seam[k], R.relmax_seams(z[s], zr, mask))
    print(f"[gpu] mixed {label} sweeps {sweeps}: TE {worst[0]:.2e} TM {worst[1]:.2e} | at the seams TE {seam[0]:.2e} TM {seam[1]:.2e} "
          f"| ceiling {ceiling:.2e}")
    for k, kind in enumerate(("TE", "TM")):
        bar = 4 * measured[k]
        assert bar <= ceiling, f"{label} {kind}: the bar {bar:.2e} is above a tenth of the bf16(V) distance, {ceiling:.2e}"
        assert worst[k] < bar, f"{label} sweeps {sweeps} {kind}: {worst[k]:.2e} at {where[k]} (at the seams {seam[k]:.2e}), bar {bar:.2e}"


# measured on an MI355X: (TE, TM) largest relmax over the systems of the kind and the three vectors
LPP = {
    "cfg2":            ("cfg2", {}),
    "cfg2-fwd-apart":  ("cfg2", {"HMCMT_FUSED_FWD": "0"}),
    "cfg2-back-apart": ("cfg2", {"HMCMT_FUSED_BACK": "0"}),
    "w270-wide":       ("w270", {}),
}
MEASURED_LPP = {
    ("cfg2", 1): (3.59e-06, 2.87e-06), ("cfg2", 2): (2.50e-06, 3.75e-06),
    ("cfg2-fwd-apart", 1): (3.59e-06, 2.86e-06), ("cfg2-fwd-apart", 2): (2.92e-06, 3.76e-06),
    ("cfg2-back-apart", 1): (3.56e-06, 2.87e-06), ("cfg2-back-apart", 2): (2.52e-06, 3.75e-06),
    ("w270-wide", 1): (4.17e-06, 2.16e-06), ("w270-wide", 2): (1.88e-06, 2.52e-06),
}


@pytest.mark.parametrize("variant,sweeps", list(MEASURED_LPP))
def test_mixed_launch_per_phase_preconditioner_is_the_modelled_reference(monkeypatch, variant, sweeps):
    """The default precision on the launch-per-phase loop: the fused forward (k_fdm_fwd) and back (k_back_post) kernels, each of
    them replaced by its separate kernels, and the wide path of meshes beyond 256 padded nodes (k_transform_lp, k_thomas32, k_post,
    k_post_w2)."""
    name, env = LPP[variant]
    ctx, ref, m = _open(monkeypatch, name, env, sweeps)
    try:
        assert ctx.stats()["smoother_sweeps"] // 10 == sweeps
        assert (ctx.NYP > 256) == (variant == "w270-wide"), ctx.NYP
        _compare_mixed(ctx, ref, name, ctx.debug_precond, sweeps, f"launch-per-phase {variant}", MEASURED_LPP[(variant, sweeps)])
    finally:
        ctx.close()


# variant -> (shape, environment, expected strips, column parts, slab modes, workgroups per system, width-specialised kernel)
PERSIST = {
    "cfg2-3wg":      ("cfg2", {}, 2, 1, 32, 3, 0),
    "cfg2-forced2":  ("cfg2", {"HMCMT_PERSIST_CS": "2"}, 2, 2, 16, 6, 0),
    "w301-generic2": ("w301", {"HMCMT_PERSIST_WIDTHK": "0"}, 2, 2, 16, 4, 0),
    "w100-k112":     ("w100", {}, 2, 1, None, 2, 112),
    "w200-k208":     ("w200", {}, 2, 1, None, 2, 208),
    "w405-k416":     ("w405", {}, 2, 2, 16, 4, 416),
    "cfg2-strips4":  ("cfg2", {"HMCMT_PERSIST_STRIPS": "4"}, 4, 1, 32, 3, 0),
    "slab16":        ("slab16", {}, 2, 1, 16, 3, 0),
}
MEASURED_PERSIST = {
    ("cfg2-3wg", 1): (3.56e-06, 3.03e-06), ("cfg2-3wg", 2): (2.51e-06, 3.67e-06),
    ("cfg2-forced2", 1): (3.65e-06, 3.02e-06), ("cfg2-forced2", 2): (2.87e-06, 3.67e-06),
    ("w301-generic2", 1): (2.41e-06, 2.68e-06), ("w301-generic2", 2): (1.94e-06, 1.73e-06),
    ("w100-k112", 1): (2.49e-06, 2.52e-06), ("w100-k112", 2): (2.12e-06, 1.85e-06),
    ("w200-k208", 1): (2.43e-06, 2.28e-06), ("w200-k208", 2): (2.04e-06, 1.70e-06),
    ("w405-k416", 1): (2.59e-06, 2.15e-06), ("w405-k416", 2): (1.67e-06, 1.56e-06),
    ("cfg2-strips4", 1): (3.59e-06, 2.90e-06), ("cfg2-strips4", 2): (2.95e-06, 3.67e-06),
    ("slab16", 1): (2.45e-06, 2.95e-06), ("slab16", 2): (2.12e-06, 1.56e-06),
}


@pytest.mark.parametrize("variant,sweeps", list(MEASURED_PERSIST))
def test_persistent_preconditioner_is_the_modelled_reference(monkeypatch, variant, sweeps):
    """Every variant of the persistent kernel, through its first preconditioner application: three workgroups per system with a
    short last one; two column parts forced onto a mesh one tile would hold, and chosen by the kernel on a 301-wide mesh (generic
    instantiation); the width-specialised instantiations 112 / 208 / 416; four strips; 16-mode slabs with one column part (four
    slabs on three workgroups: precond_ref.SLAB16 says how the mesh was picked with hmcmt_persist_envelope)."""
    name, env, strips, parts, slab, wgs, width = PERSIST[variant]
    ctx, ref, m = _open(monkeypatch, name, env, sweeps)
    try:
        info = ctx.persist_info()
        got = (info["strips"], info["column_parts"], info["workgroups_per_system"], ctx.persist_width())
        assert got == (strips, parts, wgs, width), (variant, got, info)
        if slab is not None:
            assert info["slab_modes"] == slab, info
        if variant == "slab16":
            env16 = persist_envelope(ref.ny, ref.nz, 32, ctx.S)
            assert env16["slab_modes"] == 16 and env16["column_parts"] == 1 and persist_envelope(ref.ny, ref.nz - 1, 32, ctx.S)["slab_modes"] == 32
        _compare_mixed(ctx, ref, name, lambda v: ctx.debug_persist_precond(v, sweeps), sweeps, f"persistent {variant}",
                       MEASURED_PERSIST[(variant, sweeps)])
    finally:
        ctx.close()
