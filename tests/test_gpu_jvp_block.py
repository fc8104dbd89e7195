"""Block Jacobian products on the GPU (hmcmt_jvp_block / hmcmt_jtvp_block / hmcmt_gn_hessvec_block): several directions at one
linearisation point in ONE solve per route.  Against the reference's definition (oracle Jacobian times v, direction by direction),
against the single-direction products, independence of the company a direction keeps, the adjoint and Gauss-Newton identities on
the block, isolation of the context state, the state rules and errors, and the cfg5 mesh through the _device entry points.

Ceilings: against the oracle, test_gpu_jvp's (SHALLOW_TOL / DEEP_TOL of the row's maximum, summed over the entries of v); between
two routes through the library's own solves ROUTES_TOL = 1e-9 (relmax), the project's bound for that."""
import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import tipper_ref as TR
from tests.helpers import make_problem, ragged_problem, rhophase_problem, relmax
from tests.test_gpu_jacobian import SHALLOW_TOL, DEEP_TOL, _ran_the_persistent_kernel
from tests.test_gpu_jvp import ROUTES_TOL, _case, _deep, _chain

pytestmark = pytest.mark.gpu


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


@pytest.mark.parametrize("name", ["tiny", "cfg2", "ragged", "rhophase_tiny", "tipper"])
def test_jvp_block_equals_the_oracle_jacobian_times_v(name):
    """Every direction of jvp_block(V) -- three seeded normals, the side-column unit vector, one all-zero direction -- meets
    test_jvp_equals_the_oracle_jacobian_times_v's ceiling against Jo @ v, both wrt; the zero direction is exactly zero."""
    mesh, data, inv, m, Jo = _case(name)
    deep = _deep(mesh, inv)
    rng = np.random.default_rng(5)
    nA = len(m)
    e = np.zeros(nA)
    e[list(inv.activeIdx).index((len(mesh.airLayer) + 2) * mesh.gridSize[0])] = 1.0
    V = np.stack([rng.standard_normal(nA), rng.standard_normal(nA), rng.standard_normal(nA), e, np.zeros(nA)])
    ctx = HipContext(mesh, data, inv)
    ctx.linearize(m)
    worst = 0.0
    for wrt, sc in (("sigma", np.ones(nA)), ("lnsigma", np.exp(m))):
        Jw = Jo * sc[None, :]
        got = ctx.jvp_block(V, wrt=wrt)
        st = ctx.block_stats
        assert st["status"] == 0 and st["fallback_solves"] == 0, st
        assert got.shape == (5, Jo.shape[0])
        assert not np.any(got[4]), "the zero direction is not exactly zero"
        for j in range(4):
            v = V[j]
            ceil = (SHALLOW_TOL * np.abs(v[~deep]).sum() + DEEP_TOL * np.abs(v[deep]).sum()) * np.abs(Jw).max(axis=1)
            worst = max(worst, float((np.abs(got[j] - Jw @ v) / ceil).max()))
    ctx.close()
    print(f"jvp_block/oracle {name}: ratio to the ceiling {worst:.3e}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("name", ["cfg2", "cfg3"])
def test_block_products_equal_the_single_products(name):
    """nvec = 8: each direction of jvp_block, jtvp_block and gn_hessvec_block equals the single-direction call to ROUTES_TOL; on cfg3
    the persistent kernel ran and a block is ONE launch per route (persist_info()["solves"])."""
    mesh, data, inv, m = make_problem(name)
    rng = np.random.default_rng(21)
    V = rng.standard_normal((8, len(m)))
    U = rng.standard_normal((8, len(inv.dataW))) + 1j * rng.standard_normal((8, len(inv.dataW)))
    ctx = HipContext(mesh, data, inv)
    ctx.linearize(m)
    singles = (np.stack([ctx.jvp(v, wrt="lnsigma") for v in V]), np.stack([ctx.jtvp(u, wrt="lnsigma") for u in U]),
               np.stack([ctx.gn_hessvec(v, wrt="lnsigma") for v in V]))
    launches, blocks = [], []
    for fn, X in ((ctx.jvp_block, V), (ctx.jtvp_block, U), (ctx.gn_hessvec_block, V)):
        s0 = ctx.persist_info()["solves"]
        blocks.append(fn(X, wrt="lnsigma"))
        launches.append(ctx.persist_info()["solves"] - s0)
        st = ctx.block_stats
        assert st["status"] == 0 and st["fallback_solves"] == 0, st
    if name == "cfg3":
        _ran_the_persistent_kernel(ctx)
        assert launches == [1, 1, 2], launches
    ctx.close()
    errs = [max(relmax(b[j], s[j]) for j in range(8)) for b, s in zip(blocks, singles)]
    print(f"block/single {name}: jvp {errs[0]:.3e} jtvp {errs[1]:.3e} gn {errs[2]:.3e} bitwise {[_bits(b, s) for b, s in zip(blocks, singles)]} launches {launches}")
    assert max(errs) < ROUTES_TOL, errs


def test_a_direction_does_not_depend_on_its_company_cfg2():
    """One direction alone (nvec = 1), at position 3 of a block of 5 and in a block of 16: ROUTES_TOL; a block twice: same bits."""
    mesh, data, inv, m = make_problem("cfg2")
    rng = np.random.default_rng(22)
    v = rng.standard_normal(len(m))
    u = rng.standard_normal(len(inv.dataW)) + 1j * rng.standard_normal(len(inv.dataW))
    ctx = HipContext(mesh, data, inv)
    ctx.linearize(m)
    worst = 0.0
    for fn, x, n in ((ctx.jvp_block, v, len(m)), (ctx.jtvp_block, u, len(inv.dataW)), (ctx.gn_hessvec_block, v, len(m))):
        cplx = np.iscomplexobj(x)
        def others(k):
            r = rng.standard_normal((k, n))
            return r + 1j * rng.standard_normal((k, n)) if cplx else r
        alone = fn(x[None, :])[0]
        X5 = others(5); X5[3] = x
        X16 = others(16); X16[11] = x
        a5, a16 = fn(X5), fn(X16)
        worst = max(worst, relmax(a5[3], alone), relmax(a16[11], alone))
        assert _bits(fn(X16), a16) and _bits(fn(X5), a5)
    ctx.close()
    print(f"company cfg2: worst {worst:.3e}")
    assert worst < ROUTES_TOL, worst


def test_identities_on_the_block_cfg2():
    """tol 1e-11: Re(U_i^H (J V)_j) = V_j^T (J^T U)_i for every pair relative to |U_i| |J V_j|; V^T (H V) symmetric with diagonal
    |W J V_j|^2; gn_hessvec_block(V) = jtvp_block(W^2 jvp_block(V)).  Ceiling: test_adjoint_identity_and_gauss_newton_product's."""
    mesh, data, inv, m = make_problem("cfg2")
    rng = np.random.default_rng(23)
    V = rng.standard_normal((4, len(m)))
    U = rng.standard_normal((3, len(inv.dataW))) + 1j * rng.standard_normal((3, len(inv.dataW)))
    ctx = HipContext(mesh, data, inv, tol=1e-11)
    ctx.linearize(m)
    JV, JTU, HV = ctx.jvp_block(V, wrt="lnsigma"), ctx.jtvp_block(U, wrt="lnsigma"), ctx.gn_hessvec_block(V, wrt="lnsigma")
    comp = relmax(HV, ctx.jtvp_block(inv.dataW[None, :] ** 2 * JV, wrt="lnsigma"))
    ctx.close()
    adj = max(abs(np.real(np.vdot(U[i], JV[j])) - V[j] @ JTU[i]) / (np.linalg.norm(U[i]) * np.linalg.norm(JV[j]))
              for i in range(3) for j in range(4))
    G = V @ HV.T
    sym = max(abs(G[i, j] - G[j, i]) / (np.linalg.norm(V[i]) * np.linalg.norm(HV[j])) for i in range(4) for j in range(i))
    q = np.sum(np.abs(inv.dataW[None, :] * JV) ** 2, axis=1)
    pos = float(np.max(np.abs(np.diag(G) - q) / q))
    print(f"block identities cfg2: adjoint {adj:.3e} symmetry {sym:.3e} diagonal {pos:.3e} composed {comp:.3e}")
    assert np.all(np.diag(G) > 0)
    assert max(adj, sym, pos) < ROUTES_TOL, (adj, sym, pos)
    assert comp < ROUTES_TOL, comp


class _WithBlocks:
    """a context whose linearize is followed by one block product of each kind (nvec = 4): for test_gpu_jvp._chain"""
    def __init__(self, ctx):
        self._ctx, self._rng = ctx, np.random.default_rng(7)

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def linearize(self, m):
        c, rng = self._ctx, self._rng
        c.linearize(m)
        st0, it0 = c.stats(), c.iters()
        c.jvp_block(rng.standard_normal((4, c.nAC)))
        c.jtvp_block(rng.standard_normal((4, c.nData)) + 0j, wrt="lnsigma")
        c.gn_hessvec_block(rng.standard_normal((4, c.nAC)))
        assert c.stats() == st0 and np.array_equal(c.iters(), it0)


def test_isolation_of_the_context_state_with_blocks():
    """test_isolation_of_the_context_state's chain is bit for bit the same with three block products (nvec = 4) behind every
    linearize, and a single jvp afterwards is bit for bit what it is without them: on the chain's context against the same chain
    without blocks, and on a fresh context with block products in front against a fresh context without.
    (The chain's context against a FRESH one is printed, not asserted: measured on MI355X, the single jvp after the chain differs
    from a fresh context's by 1.5e-10 (relmax) with or without block products -- the chain leaves the forward solve's sweep choice
    at its own history, so linearize solves the same systems another way.  That difference is the parent's, not the blocks'.)"""
    mesh, data, inv, m = make_problem("cfg2")
    p0 = np.random.default_rng(3).standard_normal(len(m))
    v = np.random.default_rng(8).standard_normal(len(m))
    runs, after = [], []
    for blocks in (False, True):
        ctx = HipContext(mesh, data, inv)
        ctx.set_prior(inv.refModel if inv.refModel is not None else m, inv.Wm, np.ones(len(m)))
        runs.append(_chain(_WithBlocks(ctx) if blocks else ctx, m, p0, False))
        ctx.linearize(m)
        if blocks:
            ctx.jvp_block(np.stack([v, -v]))
        after.append(ctx.jvp(v))
        ctx.close()
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    assert _bits(after[0], after[1])
    fresh = []
    for blocks in (False, True):
        ctx = HipContext(mesh, data, inv)
        (_WithBlocks(ctx) if blocks else ctx).linearize(m)
        fresh.append(ctx.jvp(v))
        ctx.close()
    print(f"isolation cfg2: chain's context against a fresh one, without / with blocks: {relmax(after[0], fresh[0]):.3e} {relmax(after[1], fresh[0]):.3e}")
    assert _bits(fresh[0], fresh[1])


def test_block_state_rules_errors_and_statistics():
    mesh, data, inv, m = make_problem("tiny")
    ctx = HipContext(mesh, data, inv)
    _, _, g0 = ctx.grad(m)
    rng = np.random.default_rng(2)
    V = rng.standard_normal((16, ctx.nAC))
    out = np.full((L.BLOCK_MAX + 1) * 2 * ctx.nData, 7.0)

    def still_evaluates():
        assert relmax(ctx.grad(m)[2], g0) < 1e-9
        ctx.linearize(m)

    with pytest.raises(HmcmtError, match="linearisation point"):       # before linearize
        ctx.jvp_block(V[:2])
    still_evaluates()
    ctx.grad(m + 0.01)                                                 # an evaluation ends the point
    with pytest.raises(HmcmtError, match="linearisation point"):
        ctx.gn_hessvec_block(V[:2])
    still_evaluates()
    big = np.zeros((L.BLOCK_MAX + 1) * ctx.nAC)
    for nvec in (0, L.BLOCK_MAX + 1):
        assert ctx.lib.hmcmt_jvp_block(ctx.h, L._dp(big), nvec, 0, L._dp(out), None) == -1
        assert b"nvec" in ctx.lib.hmcmt_last_error(ctx.h)
        still_evaluates()
    bad = V[:4].copy(); bad[2, 5] = np.nan
    assert ctx.lib.hmcmt_jvp_block(ctx.h, L._dp(bad), 4, 0, L._dp(out), None) == -1
    assert b"non-finite" in ctx.lib.hmcmt_last_error(ctx.h) and np.all(out == 7.0)
    still_evaluates()
    for wrt in (2, -1):
        assert ctx.lib.hmcmt_jvp_block(ctx.h, L._dp(np.ascontiguousarray(V[:2])), 2, wrt, L._dp(out), None) == -1
    assert ctx.lib.hmcmt_jvp_block(ctx.h, None, 2, 0, L._dp(out), None) == -1
    assert np.all(out == 7.0)
    still_evaluates()
    # statistics: the systems solved
    ctx.grad(m)                                                        # (cold solves: a system that carries data iterates)
    live = int(np.count_nonzero(np.asarray(ctx.iters()).reshape(2, -1)[0]))
    assert live > 0
    ctx.linearize(m)
    a2 = ctx.jvp_block(V[:2])
    st = ctx.block_stats
    assert st["nsystems"] == 2 * live and st["iters_fwd_sum"] > 0 and st["iters_adj_sum"] == 0 and st["status"] == 0, st
    Vz = V[:4].copy(); Vz[1] = 0.0
    z = ctx.jvp_block(Vz)
    assert ctx.block_stats["nsystems"] == 3 * live and not np.any(z[1])
    Uz = rng.standard_normal((3, ctx.nData)) + 1j; Uz[2] = 0.0
    zt = ctx.jtvp_block(Uz)
    st = ctx.block_stats
    assert st["nsystems"] == 2 * live and st["iters_fwd_sum"] == 0 and st["iters_adj_sum"] > 0 and not np.any(zt[2]), st
    assert not np.any(ctx.gn_hessvec_block(np.zeros((2, ctx.nAC)))) and ctx.block_stats["nsystems"] == 0
    # growing to 16 directions and back: the arrays grow, the small block is the same bits
    a16 = ctx.jvp_block(V)
    assert ctx.block_stats["nsystems"] == 16 * live
    assert max(relmax(a16[j], a2[j]) for j in range(2)) < ROUTES_TOL
    assert _bits(ctx.jvp_block(V[:2]), a2)
    # between an asynchronous evaluation and its wait
    import torch
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    dpred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device="cuda")
    dmis = torch.zeros(1, dtype=torch.float64, device="cuda")
    dg = torch.zeros(ctx.nAC, dtype=torch.float64, device="cuda")
    ctx.grad_device_async(dm.data_ptr(), dpred.data_ptr(), dmis.data_ptr(), dg.data_ptr())
    with pytest.raises(HmcmtError, match="asynchronous evaluation is in flight") as ei:
        ctx.jtvp_block(Uz)
    assert ei.value.code == -1
    ctx.wait()
    still_evaluates()
    assert _bits(ctx.jvp_block(V[:2]), a2)
    ctx.close()


def test_fp64_preconditioner_blocks_of_16_2_16_cfg2():
    """fdm_precision = fp64 (the preconditioner's two-sweep work vector is the block instance's own, sized for its capacity):
    blocks of 16, then -- after set_options and a new point -- of 2 and of 16 again, every product against the single products
    to ROUTES_TOL, no fallback."""
    mesh, data, inv, m = make_problem("cfg2")
    rng = np.random.default_rng(24)
    V = rng.standard_normal((16, len(m)))
    U = rng.standard_normal((16, len(inv.dataW))) + 1j * rng.standard_normal((16, len(inv.dataW)))
    ctx = HipContext(mesh, data, inv)
    ctx.linearize(m)
    ctx.jvp_block(V)
    ctx.set_options(fdm_precision="fp64")
    ctx.linearize(m)
    singles = (np.stack([ctx.jvp(v) for v in V]), np.stack([ctx.jtvp(u) for u in U]), np.stack([ctx.gn_hessvec(v) for v in V]))
    worst = 0.0
    for nvec in (2, 16):
        for fn, X, ref in ((ctx.jvp_block, V, singles[0]), (ctx.jtvp_block, U, singles[1]), (ctx.gn_hessvec_block, V, singles[2])):
            got = fn(X[:nvec])
            st = ctx.block_stats
            assert st["status"] == 0 and st["fallback_solves"] == 0, st
            worst = max(worst, max(relmax(got[j], ref[j]) for j in range(nvec)))
    ctx.close()
    print(f"fp64 preconditioner, blocks of 16 / 2 / 16, cfg2: worst {worst:.3e}")
    assert worst < ROUTES_TOL, worst


def _a_block_of_one_is_the_single_product(name):
    """nvec = 1 runs the one pipeline without its block-only steps, as the single entry points do: the same bits; nsystems is the
    count of systems that carry data (ragged: a quarter of the data masked); an all-zero direction is
    exactly zero and costs no iteration.  The problems are test_gpu_jvp._case's, without their oracle Jacobians."""
    if name == "rhophase_tiny":
        mesh, data, inv, m = rhophase_problem("tiny")[:4]
    elif name == "tipper":
        mesh, data, inv, m = TR.tipper_problem("tiny", "Impedance", with_impedance=False)
    else:
        mesh, data, inv, m = ragged_problem(23, 17, 3, 3, 3, 4) if name == "ragged" else make_problem(name)
    rng = np.random.default_rng(25)
    v = rng.standard_normal(len(m))
    u = rng.standard_normal(len(inv.dataW)) + 1j * rng.standard_normal(len(inv.dataW))
    ctx = HipContext(mesh, data, inv)
    ctx.grad(m)
    live = int(np.count_nonzero(np.asarray(ctx.iters()).reshape(2, -1)[0]))
    ctx.linearize(m)
    for blk, one, x in ((ctx.jvp_block, ctx.jvp, v), (ctx.jtvp_block, ctx.jtvp, u), (ctx.gn_hessvec_block, ctx.gn_hessvec, v)):
        assert _bits(blk(x[None, :])[0], one(x))
        assert ctx.block_stats["nsystems"] == live and ctx.block_stats["status"] == 0
        z = blk(np.zeros_like(x)[None, :])
        st = ctx.block_stats
        assert not np.any(z) and st["iters_fwd_sum"] == 0 and st["iters_adj_sum"] == 0 and st["status"] == 0, st
    ctx.close()


def test_a_block_of_one_is_the_single_product_tiny():
    _a_block_of_one_is_the_single_product("tiny")


@pytest.mark.parametrize("name", ["ragged", "rhophase_tiny", "tipper"])
def test_a_block_of_one_is_the_single_product(name):
    """the same on the suite's other smallest problems: masked data and a fixed cell, real data, TE systems only"""
    _a_block_of_one_is_the_single_product(name)


def test_block_products_equal_the_single_products_cfg5_device():
    """The cfg5 mesh through the _device entry points, nvec = 4, against the single _device products: ROUTES_TOL; the persistent
    kernel ran, with two column parts.  One context."""
    import torch
    mesh, data, inv, m = make_problem("cfg5")
    ctx = HipContext(mesh, data, inv)
    rng = np.random.default_rng(9)
    nv = 4
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    dV = torch.tensor(rng.standard_normal((nv, ctx.nAC)), dtype=torch.float64, device="cuda")
    dU = torch.tensor(rng.standard_normal((nv, ctx.nData)) + 1j * rng.standard_normal((nv, ctx.nData)), dtype=torch.complex128, device="cuda")
    ctx.linearize_device(dm.data_ptr())
    sJV = torch.zeros((nv, ctx.nData), dtype=torch.complex128, device="cuda")
    sJTU = torch.zeros((nv, ctx.nAC), dtype=torch.float64, device="cuda")
    sHV = torch.zeros((nv, ctx.nAC), dtype=torch.float64, device="cuda")
    for j in range(nv):
        ctx.jvp_device(dV[j].data_ptr(), sJV[j].data_ptr())
        ctx.jtvp_device(dU[j].data_ptr(), sJTU[j].data_ptr())
        ctx.gn_hessvec_device(dV[j].data_ptr(), sHV[j].data_ptr())
    bJV, bJTU, bHV = torch.zeros_like(sJV), torch.zeros_like(sJTU), torch.zeros_like(sHV)
    s0 = ctx.persist_info()["solves"]
    ctx.jvp_block_device(dV.data_ptr(), nv, bJV.data_ptr())
    ctx.jtvp_block_device(dU.data_ptr(), nv, bJTU.data_ptr())
    ctx.gn_hessvec_block_device(dV.data_ptr(), nv, bHV.data_ptr())
    st = ctx.block_stats
    torch.cuda.synchronize()
    assert ctx.persist_info()["solves"] - s0 == 4
    assert st["status"] == 0 and st["fallback_solves"] == 0, st
    _ran_the_persistent_kernel(ctx)
    assert ctx.persist_info()["column_parts"] == 2
    errs = [max(relmax(b[j].cpu().numpy(), s[j].cpu().numpy()) for j in range(nv)) for b, s in ((bJV, sJV), (bJTU, sJTU), (bHV, sHV))]
    ctx.close()
    print(f"block/single cfg5: jvp {errs[0]:.3e} jtvp {errs[1]:.3e} gn {errs[2]:.3e}")
    assert max(errs) < ROUTES_TOL, errs
