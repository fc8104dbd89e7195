"""Matrix-free Jacobian products on the GPU (hmcmt_linearize / hmcmt_jvp / hmcmt_jtvp / hmcmt_gn_hessvec): against the reference's
definition (oracle.compJacMat @ v), against the parent's own routes (the explicit Jacobian, the production gradient), the adjoint
identity, differences of the forward, a matrix-free Gauss-Newton step, and the state rules (validity of the linearisation point,
isolation of the products, repeatability, statistics).

Ceilings: against the oracle, what tests/test_gpu_jacobian.py holds every entry of J to (SHALLOW_TOL 1e-7 / DEEP_TOL 2e-6 of the
row's maximum, deep = the five deepest cell rows), summed over the entries of v; between two routes through the library's own
solves, the 1e-9 of the parent's identity tests."""
import copy

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import tipper_ref as TR
from tests.helpers import make_problem, ragged_problem, rhophase_problem, relmax
from tests.test_jacobian_host import oracle_jacobian, rhophase_jacobian
from tests.test_gpu_jacobian import SHALLOW_TOL, DEEP_TOL, _ran_the_persistent_kernel

pytestmark = pytest.mark.gpu

ROUTES_TOL = 1e-9


def _deep(mesh, inv):
    ny, nt = mesh.gridSize
    return (inv.activeIdx // ny) >= nt - 5


def _case(name):
    if name == "rhophase_tiny" or name == "rhophase_cfg1":
        mesh, data, inv, m, _ = rhophase_problem(name.split("_")[1])
        return mesh, data, inv, m, rhophase_jacobian(mesh, data, m)
    if name == "tipper":
        mesh, data, inv, m = TR.tipper_problem("tiny", "Impedance", with_impedance=False)
        Jo = TR.tipper_row_values(data, TR.tipper_jacobian(copy.deepcopy(mesh), data, TR.sigma_of(inv, m), inv.activeIdx))
        return mesh, data, inv, m, Jo
    mesh, data, inv, m = ragged_problem(23, 17, 3, 3, 3, 4) if name == "ragged" else make_problem(name)
    return mesh, data, inv, m, oracle_jacobian(mesh, data, inv, m)


@pytest.mark.parametrize("name", ["tiny", "cfg2", "ragged", "rhophase_tiny", "rhophase_cfg1", "tipper"])
def test_jvp_equals_the_oracle_jacobian_times_v(name):
    """|Jv - Jo v|_k <= (1e-7 |v_shallow|_1 + 2e-6 |v_deep|_1) max_a |Jo_ka|, both wrt, a seeded random v and a unit vector on a
    side-column cell.  The measured ratio to the ceiling is printed."""
    mesh, data, inv, m, Jo = _case(name)
    deep = _deep(mesh, inv)
    rng = np.random.default_rng(5)
    nA = len(m)
    e = np.zeros(nA)
    e[list(inv.activeIdx).index((len(mesh.airLayer) + 2) * mesh.gridSize[0])] = 1.0
    ctx = HipContext(mesh, data, inv)
    ctx.linearize(m)
    worst = 0.0
    for wrt, sc in (("sigma", np.ones(nA)), ("lnsigma", np.exp(m))):
        Jw = Jo * sc[None, :]
        for v in (rng.standard_normal(nA), e):
            got = ctx.jvp(v, wrt=wrt)
            assert ctx.jvp_stats["status"] == 0 and ctx.jvp_stats["fallback_solves"] == 0
            ceil = (SHALLOW_TOL * np.abs(v[~deep]).sum() + DEEP_TOL * np.abs(v[deep]).sum()) * np.abs(Jw).max(axis=1)
            worst = max(worst, float((np.abs(got - Jw @ v) / ceil).max()))
    ctx.close()
    print(f"jvp/oracle {name}: ratio to the ceiling {worst:.3e}")
    assert worst <= 1.0, worst


def _routes(ctx, m, inv, rng):
    J = ctx.jacobian(m)
    pred, _, g = ctx.grad(m)
    ctx.linearize(m)
    v = rng.standard_normal(len(m))
    ejv = relmax(ctx.jvp(v), J @ v)
    u = inv.dataW * (inv.dataW * (pred - inv.obsData))
    ejt = relmax(np.exp(m) * ctx.jtvp(u), g)
    return ejv, ejt


@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_products_equal_the_parents_routes(name):
    """jvp(v) against ctx.jacobian(m) @ v, and exp(m) jtvp(W^2 (pred - obs)) against ctx.grad(m)[2]: 1e-9 (relmax)."""
    mesh, data, inv, m = make_problem(name)
    ctx = HipContext(mesh, data, inv)
    s0 = ctx.persist_info()["solves"]
    ejv, ejt = _routes(ctx, m, inv, np.random.default_rng(9))
    if name == "cfg3":
        _ran_the_persistent_kernel(ctx)
        assert ctx.persist_info()["solves"] - s0 >= 42 + 2 + 1 + 2      # Jacobian, gradient, linearize, the two products
    ctx.close()
    print(f"routes {name}: jvp {ejv:.3e} jtvp {ejt:.3e}")
    assert ejv < ROUTES_TOL and ejt < ROUTES_TOL, (ejv, ejt)


def test_products_equal_the_parents_routes_cfg5_device():
    """The cfg5 mesh through the _device entry points: jvp against J @ v accumulated from row blocks of hmcmt_jacobian_device, jtvp
    against the production gradient."""
    import torch
    mesh, data, inv, m = make_problem("cfg5")
    ctx = HipContext(mesh, data, inv)
    pred, _, g = ctx.grad(m)
    rng = np.random.default_rng(9)
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    dv = torch.tensor(rng.standard_normal(ctx.nAC), dtype=torch.float64, device="cuda")
    ref = torch.zeros(ctx.nData, dtype=torch.complex128, device="cuda")
    blk = 648
    buf = torch.empty((blk, ctx.nAC), dtype=torch.complex128, device="cuda")
    for r0 in range(0, ctx.nData, blk):
        n = min(blk, ctx.nData - r0)
        ctx.jacobian_device(dm.data_ptr(), r0, n, buf.data_ptr())
        ref[r0:r0 + n] = buf[:n] @ dv.to(torch.complex128)
    ctx.linearize_device(dm.data_ptr())
    djv = torch.zeros(ctx.nData, dtype=torch.complex128, device="cuda")
    ctx.jvp_device(dv.data_ptr(), djv.data_ptr())
    du = torch.tensor(inv.dataW * (inv.dataW * (pred - inv.obsData)), dtype=torch.complex128, device="cuda")
    dg = torch.zeros(ctx.nAC, dtype=torch.float64, device="cuda")
    ctx.jtvp_device(du.data_ptr(), dg.data_ptr())
    torch.cuda.synchronize()
    _ran_the_persistent_kernel(ctx)
    ejv = relmax(djv.cpu().numpy(), ref.cpu().numpy())
    ejt = relmax(np.exp(m) * dg.cpu().numpy(), g)
    ctx.close()
    print(f"routes cfg5: jvp {ejv:.3e} jtvp {ejt:.3e}")
    assert ejv < ROUTES_TOL and ejt < ROUTES_TOL, (ejv, ejt)


@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_adjoint_identity_and_gauss_newton_product(name):
    """Re(u^H jvp(v)) = v^T jtvp(u) relative to |u| |jvp(v)| for seeded random real v and complex u, at options.tol 1e-11 and 1e-13;
    gn_hessvec symmetric (w^T H v = v^T H w), v^T H v = |W jvp(v)|^2 >= 0, and equal to jtvp(W^2 jvp(v)) composed on the host.
    Ceiling 1e-9 (two routes through solves stopped at tol).  Measured on MI355X, worst of the four residuals: cfg2 6.5e-13 at tol
    1e-11 (v^T H v against |W jvp(v)|^2; the adjoint identity itself 3.7e-13) and 1.1e-13 at 1e-13; cfg3 3.9e-13 and 4.4e-15; the
    composed product equals gn_hessvec bit for bit.  Asserted: ten times the worse, 6.5e-12."""
    mesh, data, inv, m = make_problem(name)
    rng = np.random.default_rng(13)
    v, w = rng.standard_normal(len(m)), rng.standard_normal(len(m))
    u = rng.standard_normal(len(inv.dataW)) + 1j * rng.standard_normal(len(inv.dataW))
    worst = 0.0
    for tol in (1e-11, 1e-13):
        ctx = HipContext(mesh, data, inv, tol=tol)
        ctx.linearize(m)
        jv, jtu = ctx.jvp(v, wrt="lnsigma"), ctx.jtvp(u, wrt="lnsigma")
        res = abs(np.real(np.vdot(u, jv)) - v @ jtu) / (np.linalg.norm(u) * np.linalg.norm(jv))
        Hv, Hw = ctx.gn_hessvec(v, wrt="lnsigma"), ctx.gn_hessvec(w, wrt="lnsigma")
        st = ctx.jvp_stats
        assert st["status"] == 0 and st["iters_fwd_sum"] > 0 and st["iters_adj_sum"] > 0 and st["fallback_solves"] == 0, st
        sym = abs(w @ Hv - v @ Hw) / (np.linalg.norm(w) * np.linalg.norm(Hv))
        q = float(np.sum(np.abs(inv.dataW * jv) ** 2))
        pos = abs(v @ Hv - q) / q
        comp = relmax(Hv, ctx.jtvp(inv.dataW ** 2 * jv, wrt="lnsigma"))
        ctx.close()
        print(f"identity {name} tol {tol:g}: adjoint {res:.3e} symmetry {sym:.3e} vHv {pos:.3e} composed {comp:.3e}")
        assert v @ Hv > 0
        worst = max(worst, res, sym, pos, comp)
    assert worst < min(ROUTES_TOL, 10 * 6.5e-13), worst


def test_linearisation_against_differences_of_the_forward_cfg2():
    """jvp(dm, wrt="lnsigma") against central differences of hmcmt_forward (test_gpu_jacobian's perturbation and its 1e-5)."""
    mesh, data, inv, m = make_problem("cfg2")
    ny, nt = mesh.gridSize
    nair = len(mesh.airLayer)
    ky, kz = inv.activeIdx % ny, inv.activeIdx // ny
    yc, zc = (ny - 1) / 2.0, nair + (nt - nair) / 3.0
    dm = np.exp(-((ky - yc) / (ny / 8.0)) ** 2 - ((kz - zc) / ((nt - nair) / 8.0)) ** 2)
    dm[(ky < 8) | (ky >= ny - 8) | (kz >= nt - 6)] = 0.0
    ctx = HipContext(mesh, data, inv, tol=1e-13)
    ctx.linearize(m)
    jv = ctx.jvp(dm, wrt="lnsigma")
    h = 1e-4
    pp, _ = ctx.forward(m + h * dm)
    pm, _ = ctx.forward(m - h * dm)
    ctx.close()
    assert relmax(jv, (pp - pm) / (2 * h)) < 1e-5


def test_gauss_newton_step_matrix_free_cfg2():
    """CG on (H + lambda Wm) d = -(g + lambda Wm (m - mref)) with gn_hessvec (wrt ln sigma) as the only access to H, against the dense
    solve with Jo from the oracle; lambda = 1, Wm = inv.Wm, the same right-hand side on both sides.  CG stops at a relative residual
    tau = 1e-8 of the right-hand side; it is preconditioned with lambda Wm (sparse LU), so that its iteration count is bounded by the
    number of distinct eigenvalues H adds to the identity (measured: 356 iterations, |d' - d|_A / |d|_A = 4.3e-7 where the bound
    is 9.4e-2; printed, and asserted below the cap of 600).
    Bound, derived: A d = b (dense), (A + E) d' = b + rho with |rho| <= tau |b|, so d' - d = A^-1 (rho - E d') and, in the energy
    norm of A, |d' - d|_A = |rho - E d'|_{A^-1} <= (tau |b|_2 + |E d'|_2) / sqrt(lambda_min(A)).  E = H_gpu - H_o to first order is
    Jo^H W^2 dJ + dJ^H W^2 Jo with |dJ_ka| <= t_a r_k, t_a = 1e-7 (2e-6 in the five deepest rows), r_k = max_a |Jo_ka| -- what test 1
    of this file holds J v to --, hence |E d'| <= |Jo|^T W^2 (r (t.|d'|)) + t ((r W^2) . |Jo d'|), entry by entry."""
    mesh, data, inv, m = make_problem("cfg2")
    Jm = oracle_jacobian(mesh, data, inv, m) * np.exp(m)[None, :]
    Wm = inv.Wm.tocsr()
    mref = inv.refModel if inv.refModel is not None else np.full(len(m), np.log(0.01))
    from scipy.sparse.linalg import splu
    lam, tau, cap = 1.0, 1e-8, 600
    Minv = splu((lam * Wm).tocsc()).solve
    W2 = inv.dataW ** 2
    ctx = HipContext(mesh, data, inv)
    _, _, g = ctx.grad(m)
    b = -(g + lam * (Wm @ (m - mref)))
    ctx.linearize(m)
    A = lambda x: ctx.gn_hessvec(x, wrt="lnsigma") + lam * (Wm @ x)
    d = np.zeros(len(m)); r = b.copy(); z = Minv(r); p = z.copy(); rz = r @ z
    its = 0
    while np.linalg.norm(r) > tau * np.linalg.norm(b) and its < cap:
        Ap = A(p)
        al = rz / (p @ Ap)
        d += al * p; r -= al * Ap
        z = Minv(r)
        rn = r @ z
        p = z + (rn / rz) * p; rz = rn
        its += 1
    ctx.close()
    Ad = np.real(Jm.conj().T @ (W2[:, None] * Jm)) + lam * Wm.toarray()
    dd = np.linalg.solve(Ad, b)
    lmin = float(np.linalg.eigvalsh(Ad)[0])
    t = np.where(_deep(mesh, inv), DEEP_TOL, SHALLOW_TOL)
    rk = np.abs(Jm).max(axis=1)
    Eb = np.abs(Jm).T @ (W2 * rk * (t @ np.abs(d))) + t * ((rk * W2) @ np.abs(Jm @ d))
    bound = (tau * np.linalg.norm(b) + np.linalg.norm(Eb)) / np.sqrt(lmin)
    err = float(np.sqrt((d - dd) @ (Ad @ (d - dd))))
    ref = float(np.sqrt(dd @ (Ad @ dd)))
    print(f"gauss-newton cfg2: {its} CG iterations, |d - dd|_A / |dd|_A = {err / ref:.3e}, bound {bound / ref:.3e}")
    assert its < cap and lmin > 0
    assert err <= bound, (err, bound)


def _chain(ctx, m0, p0, products):
    import torch
    dm = torch.tensor(m0, dtype=torch.float64, device="cuda")
    dp = torch.tensor(p0, dtype=torch.float64, device="cuda")
    pred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device="cuda")
    mis = torch.zeros(1, dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(1)
    out = []
    start = 0
    for accept in (True, False, True, True):
        mstart = dm.clone()
        ctx.leapfrog_device(dm.data_ptr(), dp.data_ptr(), 0.02, 3, 1.0, np.log(1e-4), 0.0, start_grad=start,
                            d_pred=pred.data_ptr(), d_misfit=mis.data_ptr())
        ctx.wait()
        out += [dm.cpu().numpy().copy(), dp.cpu().numpy().copy(), pred.cpu().numpy().copy(), mis.cpu().numpy().copy()]
        if not accept:
            dm.copy_(mstart)
        start = 1 if accept else 2
        ctx.linearize(dm.cpu().numpy())
        if products:
            st0, it0 = ctx.stats(), ctx.iters()
            ctx.jvp(rng.standard_normal(ctx.nAC))
            ctx.jtvp(rng.standard_normal(ctx.nData) + 0j, wrt="lnsigma")
            ctx.gn_hessvec(rng.standard_normal(ctx.nAC))
            assert ctx.stats() == st0 and np.array_equal(ctx.iters(), it0)
    return out


def test_isolation_of_the_context_state():
    """A chain of device trajectories with linearize between them is bit for bit the same chain with linearize + products there."""
    mesh, data, inv, m = make_problem("cfg2")
    p0 = np.random.default_rng(3).standard_normal(len(m))
    runs = []
    for products in (False, True):
        ctx = HipContext(mesh, data, inv)
        ctx.set_prior(inv.refModel if inv.refModel is not None else m, inv.Wm, np.ones(len(m)))
        runs.append(_chain(ctx, m, p0, products))
        ctx.close()
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


def test_state_rules_repeatability_and_statistics():
    import torch
    mesh, data, inv, m = make_problem("tiny")
    ctx = HipContext(mesh, data, inv)
    _, _, g0 = ctx.grad(m)
    v = np.random.default_rng(2).standard_normal(ctx.nAC)
    u = np.random.default_rng(4).standard_normal(ctx.nData) + 1j
    with pytest.raises(HmcmtError, match="linearisation point"):       # before linearize
        ctx.jvp(v)
    ctx.linearize(m)
    a, b = ctx.jvp(v), ctx.jvp(v)
    assert np.array_equal(a.view(np.float64), b.view(np.float64))     # same call twice: same bits
    st = ctx.jvp_stats
    assert st["status"] == 0 and st["iters_fwd_sum"] > 0 and st["iters_adj_sum"] == 0 and st["fallback_solves"] == 0, st
    fwd_sum = st["iters_fwd_sum"]
    assert np.array_equal(ctx.jtvp(u), ctx.jtvp(u))
    st = ctx.jvp_stats
    assert st["iters_fwd_sum"] == 0 and st["iters_adj_sum"] > 0 and st["fallback_solves"] == 0, st
    assert np.array_equal(ctx.gn_hessvec(v), ctx.gn_hessvec(v))
    st = ctx.jvp_stats
    assert st["iters_fwd_sum"] == fwd_sum and st["iters_adj_sum"] > 0 and st["fallback_solves"] == 0, st
    out = np.empty(2 * ctx.nData)
    for wrt in (2, -1):
        assert ctx.lib.hmcmt_jvp(ctx.h, L._dp(v), wrt, L._dp(out), None) == -1
    assert ctx.lib.hmcmt_jvp(ctx.h, None, 0, L._dp(out), None) == -1
    ctx.jvp(v)                                                         # ... and the point is still valid
    ctx.grad(m + 0.01)                                                 # an intervening evaluation ends it
    with pytest.raises(HmcmtError, match="linearisation point"):
        ctx.jtvp(u)
    ctx.linearize(m)
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    dpred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device="cuda")
    dmis = torch.zeros(1, dtype=torch.float64, device="cuda")
    dg = torch.zeros(ctx.nAC, dtype=torch.float64, device="cuda")
    ctx.grad_device_async(dm.data_ptr(), dpred.data_ptr(), dmis.data_ptr(), dg.data_ptr())
    with pytest.raises(HmcmtError):
        ctx.gn_hessvec(v)
    assert ctx.lib.hmcmt_linearize(ctx.h, L._dp(np.ascontiguousarray(m))) == -1
    ctx.wait()
    ctx.grad_device(dm.data_ptr(), dpred.data_ptr(), dmis.data_ptr(), dg.data_ptr())
    assert relmax(dg.cpu().numpy(), g0) < 1e-9                         # the context still evaluates correctly
    ctx.linearize(m)
    assert np.array_equal(ctx.jvp(v).view(np.float64), a.view(np.float64))
    ctx.close()
