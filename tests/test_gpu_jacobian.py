"""The explicit Jacobian on the GPU (hmcmt_jacobian / hmcmt_jacobian_device / hmcmt_sensitivity): against oracle.compJacMat
(Impedance) and its chain rule (Rho_Pha), against golden rows of cfg3 from the oracle's compJacTMatVec, against the production
gradient (the identity J^T v, and single rows), against differences of the forward, its layout and repeatability, the
sensitivity, and that a Jacobian call leaves the context's evaluations as they were.

Tolerances against the oracle: per row, relative to max |J_k| of that row, split like the gradient's (tests/helpers.gerr_split):
1e-7 away from the deepest rows, 2e-6 in them -- looser than the 1e-8 / 5e-7 the gradient meets under gerr_split, where the
scale is max |g| over the whole gradient.  Measured on MI355X: 2.0e-8 / 6.3e-7 (cfg2, TE rows of the edge receiver, cells next to
the deepest rows), 1.1e-8 / 3.6e-7 (cfg1, Rho_Pha); the same at options.tol 1e-11 and 1e-13.  The floor is the production
gradient's, not the Jacobian's assembly: the gradient of a residual on one datum (hmcmt_grad) differs from the oracle's row by the
same 2.0e-8 / 6.3e-7, and the Jacobian's row equals it to 3e-11 (test_rows_equal_the_production_gradient_rows); the oracle's own
compJacMat and compJacTMatVec(e_k) rows agree to 3e-14."""
import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests.helpers import make_problem, ragged_problem, rhophase_problem, relmax
from tests.test_jacobian_host import oracle_jacobian, rhophase_jacobian

pytestmark = pytest.mark.gpu

SHALLOW_TOL, DEEP_TOL = 1e-7, 2e-6


def _row_errors(J, Jo, inv, mesh, deep_rows=5):
    ny, nt = mesh.gridSize
    deep = (inv.activeIdx // ny) >= nt - deep_rows
    sc = np.abs(Jo).max(axis=1, keepdims=True)
    d = np.abs(J - Jo) / sc
    return float(d[:, ~deep].max()), float(d[:, deep].max() if deep.any() else 0.0)


def _ran_the_persistent_kernel(ctx):
    info = ctx.persist_info()
    assert info["usable_now"] == 1 and info["enabled"] == 1 and info["solves"] >= 2 and info["placement_fallbacks"] == 0 and info["timeouts"] == 0, info


def _problem(name):
    if name == "ragged":
        return ragged_problem(23, 17, 3, 3, 3, 4)
    return make_problem(name)


@pytest.mark.parametrize("name", ["tiny", "cfg2", "ragged"])
def test_jacobian_equals_oracle_compJacMat(name):
    mesh, data, inv, m = _problem(name)
    ctx = HipContext(mesh, data, inv)
    J = ctx.jacobian(m)
    st = ctx.jac_stats
    ctx.close()
    Jo = oracle_jacobian(mesh, data, inv, m)
    assert J.shape == Jo.shape and J.dtype == np.complex128
    assert st["status"] == 0 and st["iters_adj_sum"] > 0 and st["iters_fwd_sum"] > 0, st
    shallow, deep = _row_errors(J, Jo, inv, mesh)
    assert shallow < SHALLOW_TOL and deep < DEEP_TOL, (shallow, deep)


@pytest.mark.parametrize("name", ["tiny", "cfg1"])
def test_rhophase_jacobian_equals_chain_rule_reference(name):
    mesh, data, inv, m, _ = rhophase_problem(name)
    ctx = HipContext(mesh, data, inv)
    J = ctx.jacobian(m)
    ctx.close()
    Jo = rhophase_jacobian(mesh, data, m)
    assert J.dtype == np.float64 and J.shape == Jo.shape
    shallow, deep = _row_errors(J, Jo, inv, mesh)
    assert shallow < SHALLOW_TOL and deep < DEEP_TOL, (shallow, deep)


def test_cfg3_rows_equal_the_golden_rows():
    """Six rows at the headline size (highest and lowest frequency, both polarisations, edge and centre receivers) against
    tests/golden/cfg3_jacrows*.npz, made by tests/golden/make_jac_rows.py from the oracle's compJacTMatVec(e_k), (i e_k)."""
    import os
    from tests.helpers import GOLDEN
    gs = [np.load(os.path.join(GOLDEN, f)) for f in ("cfg3_jacrows.npz", "cfg3_jacrows2.npz")]
    rows = np.concatenate([g["rows"] for g in gs])
    Jg = np.concatenate([g["J"] for g in gs])
    mesh, data, inv, m = make_problem("cfg3")
    ctx = HipContext(mesh, data, inv)
    J = np.concatenate([ctx.jacobian(m, rows=(int(k), int(k) + 1)) for k in rows])
    ctx.close()
    assert len(set(data.freqID[rows])) >= 3 and set(data.dtID[rows]) == {1, 2} and {1, data.rxLoc.shape[0]} <= set(data.rxID[rows])
    shallow, deep = _row_errors(J, Jg, inv, mesh)
    assert shallow < SHALLOW_TOL and deep < DEEP_TOL, (shallow, deep)


def test_rows_equal_the_production_gradient_rows():
    """Row k of J is the gradient (hmcmt_grad, the production path) of a residual on datum k alone: with W^2 (pred - obs) = e_k the
    gradient is exp(m) Re J_k, with i e_k it is exp(m) Im J_k.  Rows where the comparison with the oracle is at its floor (cfg2: 124,
    the edge receiver's TE row at the third frequency) and elsewhere."""
    from hmcmt2d_amd import invsetup as I, synthetic as S
    mesh, data, inv, m = make_problem("cfg2")
    ctx = HipContext(mesh, data, inv)
    pred, _ = ctx.forward(m)
    J = ctx.jacobian(m)
    ctx.close()
    for k in (124, 0, 200):
        parts = []
        for c in (1.0, 1j):
            obs = pred.copy()
            obs[k] -= c / inv.dataW[k] ** 2
            inv2 = I.setupInverseDataModel(mesh, [S.SIG_AIR], 0.0, 0.0, obs, 1.0 / inv.dataW)
            ctx = HipContext(mesh, data, inv2)
            parts.append(ctx.grad(m)[2] / np.exp(m))
            ctx.close()
        row = parts[0] + 1j * parts[1]
        assert np.abs(J[k] - row).max() / np.abs(row).max() < 1e-9, k


def _identity(ctx, m, inv, J):
    pred, _, g = ctx.grad(m)
    v = inv.dataW * (inv.dataW * (pred - inv.obsData))
    gJ = np.exp(m) * np.real(J.T @ np.conj(v))
    return relmax(gJ, g)


def test_identity_with_the_production_gradient_cfg3():
    mesh, data, inv, m = make_problem("cfg3")
    ctx = HipContext(mesh, data, inv)
    s0 = ctx.persist_info()["solves"]
    J = ctx.jacobian(m)
    _ran_the_persistent_kernel(ctx)
    assert ctx.persist_info()["solves"] - s0 >= 41 + 1          # the forward solve and one per receiver, all on the persistent kernel
    assert _identity(ctx, m, inv, J) < 1e-9
    ctx.close()


def test_identity_with_the_production_gradient_rhophase_cfg1():
    mesh, data, inv, m, _ = rhophase_problem("cfg1")
    ctx = HipContext(mesh, data, inv)
    J = ctx.jacobian(m)
    assert _identity(ctx, m, inv, J) < 1e-9
    ctx.close()


def test_identity_with_the_production_gradient_cfg5_device_blocks():
    """cfg5's J (6.6 GB complex) in row blocks through hmcmt_jacobian_device into torch buffers, J^T v accumulated on the device."""
    import torch
    mesh, data, inv, m = make_problem("cfg5")
    ctx = HipContext(mesh, data, inv)
    pred, _, g = ctx.grad(m)
    v = torch.tensor(inv.dataW * (inv.dataW * (pred - inv.obsData)), dtype=torch.complex128, device="cuda")
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    acc = torch.zeros(ctx.nAC, dtype=torch.complex128, device="cuda")
    blk = 648
    buf = torch.empty((blk, ctx.nAC), dtype=torch.complex128, device="cuda")
    s0 = ctx.persist_info()["solves"]
    for r0 in range(0, ctx.nData, blk):
        n = min(blk, ctx.nData - r0)
        ctx.jacobian_device(dm.data_ptr(), r0, n, buf.data_ptr())
        acc += buf[:n].T @ torch.conj(v[r0:r0 + n])
    torch.cuda.synchronize()
    _ran_the_persistent_kernel(ctx)
    assert ctx.persist_info()["solves"] - s0 >= 8 * (1 + 81)    # each of the 8 blocks: its forward solve and the 81 receivers
    gJ = np.exp(m) * acc.real.cpu().numpy()
    assert relmax(gJ, g) < 1e-9
    ctx.close()


def test_linearisation_against_differences_of_the_forward_cfg2():
    """J dm against central differences of hmcmt_forward for a smooth perturbation that vanishes on the padding and boundary cells."""
    mesh, data, inv, m = make_problem("cfg2")
    ny, nt = mesh.gridSize
    nair = len(mesh.airLayer)
    ky, kz = inv.activeIdx % ny, inv.activeIdx // ny
    yc, zc = (ny - 1) / 2.0, nair + (nt - nair) / 3.0
    dm = np.exp(-((ky - yc) / (ny / 8.0)) ** 2 - ((kz - zc) / ((nt - nair) / 8.0)) ** 2)
    dm[(ky < 8) | (ky >= ny - 8) | (kz >= nt - 6)] = 0.0
    ctx = HipContext(mesh, data, inv, tol=1e-13)
    J = ctx.jacobian(m, wrt="lnsigma")
    h = 1e-4
    pp, _ = ctx.forward(m + h * dm)
    pm, _ = ctx.forward(m - h * dm)
    ctx.close()
    fd = (pp - pm) / (2 * h)
    assert relmax(J @ dm, fd) < 1e-5


def test_layout_blocks_wrt_entry_points_and_repeatability():
    import torch
    mesh, data, inv, m = make_problem("cfg2")
    ctx = HipContext(mesh, data, inv)
    J = ctx.jacobian(m)
    J2 = ctx.jacobian(m)
    assert np.array_equal(J.view(np.float64), J2.view(np.float64))                          # two calls: identical bits
    cuts = [0, 37, 101, 102, 250, ctx.nData]
    blocks = np.concatenate([ctx.jacobian(m, rows=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(blocks.view(np.float64), J.view(np.float64))                     # row blocks = the full J
    Jl = ctx.jacobian(m, wrt="lnsigma")
    ref = J * np.exp(m)[None, :]
    for part in (np.real, np.imag):
        # sigma-scaled: the kernel multiplies by its own exp(m), which may differ from numpy's by 1 ulp -- hence 2 ulp of the product
        assert (np.abs(part(Jl) - part(ref)) <= 2 * np.spacing(np.abs(part(ref)))).all()
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    dJ = torch.empty((ctx.nData, ctx.nAC), dtype=torch.complex128, device="cuda")
    ctx.jacobian_device(dm.data_ptr(), 0, ctx.nData, dJ.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dJ.cpu().numpy().view(np.float64), J.view(np.float64))           # host and device entry points
    ctx.close()


@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_sensitivity_equals_column_norms_of_WJ(name):
    mesh, data, inv, m = make_problem(name)
    ctx = HipContext(mesh, data, inv)
    s = ctx.sensitivity(m)
    J = ctx.jacobian(m)
    sl = ctx.sensitivity(m, wrt="lnsigma")
    ctx.close()
    ref = np.sqrt((np.abs(inv.dataW[:, None] * J) ** 2).sum(axis=0))
    assert relmax(s, ref) < 1e-12
    assert relmax(sl, ref * np.exp(m)) < 1e-12


def _chain(ctx, m0, p0, calls, mesh, inv):
    """Four device trajectories (start_grad 0, then 1 or 2 by a fixed accept pattern); `calls`: a Jacobian and a sensitivity
    call between trajectories.  Returns everything the chain produced, as host arrays."""
    import torch
    dm = torch.tensor(m0, dtype=torch.float64, device="cuda")
    dp = torch.tensor(p0, dtype=torch.float64, device="cuda")
    pred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device="cuda")
    mis = torch.zeros(1, dtype=torch.float64, device="cuda")
    out = []
    start = 0
    for t, accept in enumerate((True, False, True, True)):
        mstart = dm.clone()
        ctx.leapfrog_device(dm.data_ptr(), dp.data_ptr(), 0.02, 3, 1.0, np.log(1e-4), 0.0, start_grad=start,
                            d_pred=pred.data_ptr(), d_misfit=mis.data_ptr())
        ctx.wait()
        out += [dm.cpu().numpy().copy(), dp.cpu().numpy().copy(), pred.cpu().numpy().copy(), mis.cpu().numpy().copy()]
        if not accept:
            dm.copy_(mstart)
        start = 1 if accept else 2
        if calls:
            st0 = ctx.stats()
            ctx.jacobian(dm.cpu().numpy(), rows=(5, 40))
            ctx.sensitivity(dm.cpu().numpy())
            assert ctx.stats() == st0
    return out


def test_isolation_of_the_context_state():
    mesh, data, inv, m = make_problem("cfg2")
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(len(m))
    runs = []
    for calls in (False, True):
        ctx = HipContext(mesh, data, inv)
        ctx.set_prior(inv.refModel if inv.refModel is not None else m, inv.Wm, np.ones(len(m)))
        runs.append(_chain(ctx, m, p0, calls, mesh, inv))
        if calls:
            # the memo still answers a repeated model
            a = ctx.grad(m)
            hits0 = ctx.stats()
            b = ctx.grad(m)
            assert ctx.stats()["iters_fwd_sum"] == 0 and np.array_equal(a[2], b[2])
            ctx.jacobian(m, rows=(0, 3))
            c = ctx.grad(m)
            assert ctx.stats()["iters_fwd_sum"] == 0 and np.array_equal(a[2], c[2])
        ctx.close()
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


def test_errors_leave_the_context_usable():
    import torch
    mesh, data, inv, m = make_problem("tiny")
    ctx = HipContext(mesh, data, inv)
    _, _, g0 = ctx.grad(m)
    lib = ctx.lib
    J = np.empty(2 * ctx.nAC * ctx.nData)
    mm = np.ascontiguousarray(m)
    for r0, n, wrt in ((-1, 1, 0), (0, ctx.nData + 1, 0), (ctx.nData, 1, 0), (0, 1, 2), (0, 1, -1)):
        assert lib.hmcmt_jacobian(ctx.h, L._dp(mm), r0, n, wrt, L._dp(J), None) == -1
    assert lib.hmcmt_sensitivity(ctx.h, L._dp(mm), 5, L._dp(J), None) == -1
    for rows in ((5, 2), (-1, 3), (0, ctx.nData + 1)):
        with pytest.raises(ValueError):
            ctx.jacobian(m, rows=rows)
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    dpred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device="cuda")
    dmis = torch.zeros(1, dtype=torch.float64, device="cuda")
    dg = torch.zeros(ctx.nAC, dtype=torch.float64, device="cuda")
    ctx.grad_device_async(dm.data_ptr(), dpred.data_ptr(), dmis.data_ptr(), dg.data_ptr())
    assert lib.hmcmt_jacobian(ctx.h, L._dp(mm), 0, 1, 0, L._dp(J), None) == -1
    with pytest.raises(HmcmtError):
        ctx.sensitivity(m)
    ctx.wait()
    ctx.grad_device(dm.data_ptr(), dpred.data_ptr(), dmis.data_ptr(), dg.data_ptr())
    assert relmax(dg.cpu().numpy(), g0) < 1e-9
    Jt = ctx.jacobian(m)
    ctx.close()
    Jo = oracle_jacobian(mesh, data, inv, m)
    assert max(_row_errors(Jt, Jo, inv, mesh)) < DEEP_TOL
