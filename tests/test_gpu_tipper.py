"""The tipper (TZY / RealTZY / ImagTZY) on the GPU: forward, gradient, Jacobian rows, sensitivity, trajectories and the
refusals at create, against the test reference of tests/tipper_ref.py (oracle forward fields, patched oracle J and J^T v).
Bounds are those of tests/test_gpu_parity.py (pred 1e-9, misfit 1e-9, gradient 1e-7) and tests/test_gpu_jacobian.py (rows)."""
import copy
import ctypes as C

import numpy as np
import pytest

from hmcmt2d_amd import marshal, synthetic as S
from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import tipper_ref as TR
from tests.helpers import GOLDEN, gerr_split, relmax
from tests.test_gpu_jacobian import SHALLOW_TOL, DEEP_TOL, _row_errors, _ran_the_persistent_kernel

pytestmark = pytest.mark.gpu

FAMILIES = [("Impedance", True), ("Impedance", False), ("Rho_Pha", True)]


def _dprism_problem(family, withZ):
    import os
    from hmcmt2d_amd import fileio
    ex = os.path.join(GOLDEN, "examples", "dprism3d")
    mesh = fileio.readEMModel2D(os.path.join(ex, "dprism2d_G96x49.mod"))
    d, _, _ = fileio.readMT2DData(os.path.join(ex, "dprism2dobs.dat"))
    assert d.rxLoc.shape[0] == 41
    return TR.tipper_problem(None, family, withZ, mesh=mesh, rx_y=d.rxLoc[:, 0], freqs=d.freqs)


def _problem(name, family, withZ):
    return _dprism_problem(family, withZ) if name == "dprism3d" else TR.tipper_problem(name, family, withZ)


# ---------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("family,withZ", FAMILIES)
@pytest.mark.parametrize("name", ["tiny", "cfg2", "dprism3d"])
def test_forward_against_the_reference(name, family, withZ):
    mesh, data, inv, m = _problem(name, family, withZ)
    # (options.tol 1e-12: T divides a lateral difference of Ex by Hy, and at the default tolerance its solver error reaches
    #  1.2e-9 of max |pred| on cfg2; the impedance alone stays below 1e-9 there, tests/test_gpu_parity.py)
    ctx = HipContext(mesh, data, inv, verify=True, tol=1e-12)
    pred, misfit = ctx.forward(m)
    st = ctx.stats()
    its = ctx.iters()
    ctx.close()
    po, mo, _ = (lambda r: (r[0], r[1], None))(_ref_forward_misfit(mesh, data, inv, m))
    assert relmax(pred, po) < 1e-9
    assert abs(misfit - mo) / mo < 1e-9
    assert st["status"] == 0
    nF = len(data.freqs)
    if not withZ:
        assert (its[0, nF:] == 0).all() and (its[0, :nF] > 0).all(), its          # TZY only: TM systems never solved
    if family != "Impedance":
        assert pred.dtype == np.float64


def _ref_forward_misfit(mesh, data, inv, m):
    po, _ = TR.forward(copy.deepcopy(mesh), data, TR.sigma_of(inv, m))
    r = inv.dataW * (po - inv.obsData)
    return po, 0.5 * float(np.sum(np.abs(r) ** 2))


# ---------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("name,family,withZ", [("cfg2",) + f for f in FAMILIES] + [("cfg3", "Impedance", True)])
def test_gradient_against_the_reference(name, family, withZ):
    mesh, data, inv, m = _problem(name, family, withZ)
    ctx = HipContext(mesh, data, inv, verify=True, tol=1e-12)
    pred, misfit, grad = ctx.grad(m)
    st = ctx.stats()
    _ran_the_persistent_kernel(ctx)
    ctx.close()
    po, mo, go = TR.gradient(copy.deepcopy(mesh), data, inv, m)
    assert relmax(pred, po) < 1e-9
    assert abs(misfit - mo) / mo < 1e-9
    if withZ:
        assert relmax(grad, go) < 1e-7, relmax(grad, go)
    else:
        # a gradient of tipper data alone carries the deep-row floor of the reference's bottom-boundary sensitivity that the
        # Jacobian's rows show (tests/test_gpu_jacobian.py): 2.7e-7 of max |g| on cfg2, in the deepest rows
        shallow, deep = gerr_split(grad, go, inv, mesh)
        assert shallow < 1e-7 and deep < 2e-6, (shallow, deep)
    assert st["status"] == 0


# ---------------------------------------------------------------------------------------------------------- Jacobian
@pytest.mark.parametrize("name,family,withZ", [("tiny", "Impedance", True), ("cfg2", "Impedance", True),
                                               ("cfg2", "Rho_Pha", True), ("tiny", "Rho_Pha", False)])
def test_tipper_rows_equal_the_patched_oracle_compJacMat(name, family, withZ):
    mesh, data, inv, m = _problem(name, family, withZ)
    _, it, _ = TR.split(data)
    ctx = HipContext(mesh, data, inv)
    J = ctx.jacobian(m)
    Jl = ctx.jacobian(m, wrt="lnsigma")
    st = ctx.jac_stats
    ctx.close()
    Jo = TR.tipper_row_values(data, TR.tipper_jacobian(copy.deepcopy(mesh), data, TR.sigma_of(inv, m), inv.activeIdx))
    if family != "Impedance":
        Jo = Jo.real
    assert st["status"] == 0
    shallow, deep = _row_errors(J[it], Jo[it], inv, mesh)
    assert shallow < SHALLOW_TOL and deep < DEEP_TOL, (shallow, deep)
    assert relmax(Jl, J * np.exp(m)[None, :]) < 1e-12


def test_a_row_range_of_tipper_rows_solves_only_te_systems():
    mesh, data, inv, m = TR.tipper_problem("cfg2", "Impedance", True)
    _, it, _ = TR.split(data)
    k = int(it[3])                                                   # a TZY row (every third datum)
    ctx = HipContext(mesh, data, inv)
    J = ctx.jacobian(m, rows=(k, k + 1))
    st = ctx.jac_stats
    ctx.close()
    nF = len(data.freqs)
    # the forward solve covers every system (2 nF); the adjoint batch only the TE system of that row's frequency
    assert st["status"] == 0 and st["iters_adj_sum"] > 0
    Jo = TR.tipper_jacobian(copy.deepcopy(mesh), data, TR.sigma_of(inv, m), inv.activeIdx)[k:k + 1]
    shallow, deep = _row_errors(J, Jo, inv, mesh)
    assert shallow < SHALLOW_TOL and deep < DEEP_TOL, (shallow, deep)
    assert st["iters_adj_max"] == st["iters_adj_sum"], st      # one system solved in the batch


@pytest.mark.parametrize("family", ["Impedance", "Rho_Pha"])
def test_identity_with_the_production_gradient_mixed_set(family):
    mesh, data, inv, m = TR.tipper_problem("cfg2", family, True)
    ctx = HipContext(mesh, data, inv)
    pred, _, g = ctx.grad(m)
    J = ctx.jacobian(m, wrt="lnsigma")
    ctx.close()
    wr = inv.dataW ** 2 * (pred - inv.obsData)
    gj = (np.conj(wr) @ J).real if family == "Impedance" else wr.real @ J
    assert relmax(gj, g) < 1e-9, relmax(gj, g)


@pytest.mark.parametrize("family", ["Impedance", "Rho_Pha"])
def test_sensitivity_includes_the_tipper_rows(family):
    mesh, data, inv, m = TR.tipper_problem("tiny", family, True)
    ctx = HipContext(mesh, data, inv)
    s = ctx.sensitivity(m)
    J = ctx.jacobian(m)
    ctx.close()
    ref = np.sqrt((np.abs(inv.dataW[:, None] * J) ** 2).sum(axis=0))
    assert relmax(s, ref) < 1e-12
    ni = TR.split(data)[0]
    ref_imp = np.sqrt((np.abs(inv.dataW[ni, None] * J[ni]) ** 2).sum(axis=0))
    assert relmax(s, ref_imp) > 1e-6                                # the tipper rows count


# ---------------------------------------------------------------------------------------------------------- trajectories
def test_device_leapfrog_equals_the_host_loop_with_tzy():
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd.structs import HMCPrior, initHMCParameter
    mesh, data, inv, m = TR.tipper_problem("cfg2", "Impedance", True)
    inv.refModel = np.full(len(m), np.log(0.01))
    # (dt 0.002: at 0.02 the rough start model's trajectory is so sensitive that the two loops part at 6e-4 on the impedance
    #  data alone; here they agree to 2.5e-11)
    prior = HMCPrior(dt=0.002, timestep=[3, 3], sigBounds=[1e-4, 1.0], regParam=1.0)
    ctx = HipContext(mesh, data, inv, warm_start=False)
    hp = initHMCParameter(len(m)); hp.invM[:] = 1.0; hp.sqrtM[:] = 1.0
    hp.rhomodel, hp.momentum = m.copy(), np.clip(np.random.default_rng(4).standard_normal(len(m)), -2.5, 2.5)
    pa = copy.deepcopy(prior)
    m_host, p_host = sampler.proposeLeapfrog(hp, mesh, data, copy.deepcopy(inv), pa, None, 3, ctx)
    ctx.set_prior(inv.refModel, inv.Wm, hp.invM)
    pb = copy.deepcopy(prior)
    m_dev, p_dev = sampler.proposeLeapfrogDevice(hp, mesh, data, copy.deepcopy(inv), pb, None, 3, ctx)
    ctx.close()
    assert pa.nfevals == pb.nfevals == 4
    assert relmax(m_dev, m_host) < 1e-10 and relmax(p_dev, p_host) < 1e-7        # (measured 2.5e-11, 1.2e-8)


def test_sampler_chain_with_tzy_stores_what_the_forward_computes():
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd.structs import HMCPrior
    mesh, data, inv, m = TR.tipper_problem("tiny", "Impedance", True)
    prior = HMCPrior(totalsamples=20, burninsamples=5, dt=0.02, timestep=[2, 3], sigBounds=[1e-4, 1.0])
    inv_c = copy.deepcopy(inv)
    inv_c.strModel = m.copy()
    models, stats, preds = sampler.runHMCSampler(copy.deepcopy(mesh), data, inv_c, prior, np.random.default_rng(5))
    sampler.release_context(inv_c)
    assert models.shape[1] == 20
    # (the chain's evaluations are warm-started at the default tolerance, the re-evaluations cold: they agree to the solver's
    #  tolerance, which T amplifies -- up to 2.1e-8 in the misfit and 6e-9 in pred measured)
    ctx = HipContext(mesh, data, inv)
    try:
        for it in range(1, 21):
            p, mis = ctx.forward(models[:, it - 1])
            assert abs(mis - stats.hmstats[0, it]) <= 1e-7 * mis
            assert relmax(p, preds[:, it]) < 1e-7
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------- refusals
def _create_rc(mesh, data, inv, codes):
    """hmcmt_create straight through the C ABI with the given component codes: (return code, error message)."""
    from hmcmt2d_amd import lib as L
    args = marshal.CreateArgs(mesh, data, inv)
    args.compMode = np.asarray(codes, dtype=np.int64)
    args.nComp = len(codes)
    lib = L.load_library()
    opts = L.Options()
    lib.hmcmt_default_options(C.byref(opts))
    h = C.c_void_p()
    rc = lib.hmcmt_create(C.byref(h), 0, *args.as_tuple(), C.byref(opts))
    msg = lib.hmcmt_last_error(h if rc == 0 else None)
    if rc == 0:
        lib.hmcmt_destroy(h)
    return rc, (msg or b"").decode()


@pytest.mark.parametrize("codes,word", [([1, 2, 8], "RealTZY"), ([3, 4, 5, 6, 7], "TZY"), ([7, 1, 2], "ZXY"),
                                        ([1, 2, 10], "10"), ([1, 2, 0], "0")])
def test_bad_layouts_are_refused_and_the_library_stays_usable(codes, word):
    mesh, data, inv, m = TR.tipper_problem("tiny", "Impedance", True)
    rc, msg = _create_rc(mesh, data, inv, codes)
    assert rc == -1, (rc, msg)                                     # HMCMT_EINVAL
    assert word in msg, msg
    ctx = HipContext(mesh, data, inv)
    pred, misfit = ctx.forward(m)
    ctx.close()
    assert relmax(pred, _ref_forward_misfit(mesh, data, inv, m)[0]) < 1e-9
