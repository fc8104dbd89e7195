"""The MAP optimiser on the GPU (hmcmt_map_*, kernels_map.h): the direction's kernels against their host instantiation bit for bit and
against the longdouble two-loop recursion, every step of live runs replayed by the reference from the library's own previous state,
whole runs against the oracle-driven reference, the stall on tiny, and the rules of the calls."""
import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from tests import map_cases as Cs
from tests import map_ref as R
from tests.emul import emul_map_py as E

pytestmark = pytest.mark.gpu
LO, HI = -1.0, 1.0
EPS = np.finfo(float).eps


def _context(name, cold=False):
    """cold: zero initial guesses and one smoother sweep (the sweep count otherwise adapts to the solves before), so that the gradient
    at a model is a function of the model alone (tests/test_gpu_chain_checkpoint.py: cold_sampler_context) and bits can be compared
    across calls and contexts"""
    mesh, data, inv, m, mref, lo, hi = Cs.problem(name)
    if cold:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("HMCMT_SWEEPS", "1")
            ctx = L.HipContext(mesh, data, inv, device_id=0, warm_start="cold")
    else:
        ctx = L.HipContext(mesh, data, inv, device_id=0)
    ctx.set_prior(mref, inv.Wm, np.ones(len(m)))
    return ctx, inv, m, mref, lo, hi


@pytest.fixture(scope="module")
def tiny():
    ctx, inv, m, mref, lo, hi = _context("tiny")
    yield ctx, inv, m, mref, lo, hi
    ctx.close()


@pytest.mark.parametrize("bounds", [False, True])
@pytest.mark.parametrize("n,count,H,head", Cs.DIRECTION_SHAPES)
def test_direction_kernels_equal_the_host_instantiation(tiny, n, count, H, head, bounds):
    """k_map_project, k_map_coef, k_map_expand through hmcmt_debug_map_direction: pg, d, m_t, |B| and every sum bit for bit the host
    instantiation's (no step needs a rounding allowance: every sum has one owner and one order, every product stands in an fma), d
    within the host test's bound of the longdouble two-loop, exactly 0 on B, m_t inside the bounds."""
    ctx = tiny[0]
    rng = np.random.default_rng(1000 * count + n % 997 + bounds)
    pairs = Cs.quadratic_history(n, count, rng)
    rows, sy, yy = Cs.ring_of(pairs, H, head)
    m, g = Cs.planted_state(n, rng, LO, HI, bounds)
    got = ctx.debug_map_direction(rows, head, count, sy, yy, m, g, LO, HI, 0.7)
    emu = E.direction(rows, head, count, sy, yy, m, g, LO, HI, 0.7)
    for k in ("pg", "d", "mt", "coef", "proj"):
        assert np.array_equal(got[k], emu[k]), (k, np.abs(got[k] - emu[k]).max())
    ref = R.direction(m, g, LO, HI, pairs)
    dref = np.asarray(ref["d"], dtype=float)
    assert np.abs(got["d"] - dref).max() / np.abs(dref).max() <= Cs.DIRECTION_BOUND
    B = ref["B"]
    assert got["coef"][E.MC_NB] == B.sum() and np.all(got["d"][B] == 0.0) and not np.signbit(got["d"][B]).any()
    assert got["mt"].min() >= LO and got["mt"].max() <= HI and np.all(got["mt"][B] == m[B])


def test_direction_kernels_without_pairs_and_with_a_planted_non_descent_pair(tiny):
    ctx = tiny[0]
    rng = np.random.default_rng(8)
    m, g = Cs.planted_state(390, rng, LO, HI, True)
    got, emu = ctx.debug_map_direction(None, 0, 0, None, None, m, 3 * g, LO, HI), E.direction(None, 0, 0, None, None, m, 3 * g, LO, HI)
    assert all(np.array_equal(got[k], emu[k]) for k in ("pg", "d", "mt", "coef"))
    s = -g / np.abs(g).max()
    rows, sy, yy = Cs.ring_of([(s, -s)], 8, 2)
    got, emu = ctx.debug_map_direction(rows, 2, 1, sy, yy, m, g, LO, HI), E.direction(rows, 2, 1, sy, yy, m, g, LO, HI)
    assert all(np.array_equal(got[k], emu[k]) for k in ("pg", "d", "mt", "coef", "proj"))
    assert got["coef"][E.MC_FLAG] == 1.0 and got["coef"][E.MC_USED] == 0.0 and got["coef"][E.MC_GTD] < 0


def _pairs_of(ring):
    H = ring["history"]
    slots = [(ring["head"] + i) % H for i in range(ring["count"])]
    return [(ring["rows"][k].copy(), ring["rows"][H + k].copy()) for k in slots]


@pytest.mark.parametrize("name", Cs.PADDED)
def test_every_step_of_a_live_run_is_the_reference_step_from_the_same_state(name):
    """Field-replay manner: after every hmcmt_map_step the reference is applied to the library's PREVIOUS state (model, gradient, ring)
    and fed the record's own phi_trial, so no error accumulates; and the whole 12-iteration run is held to the oracle-driven
    reference: the same decisions, Phi_k within 1e-6 relative, the final model within 1e-4, Phi never rising."""
    # (a cold context: the solves stop at a relative 1e-11, so two evaluations of one model agree to 1e-12 only when they are the
    #  same computation, which they are where nothing depends on the evaluations before)
    ctx, inv, m0, mref, lo, hi = _context(name, cold=True)
    try:
        rec = ctx.map_begin(m0, Cs.LAMBDA, lo, hi, history=Cs.HISTORY)
        oracle = Cs.oracle_run(name)
        assert rec["status"] == L.MAP_RUNNING and rec["nfevals"] == 1 and rec["nbound"] == oracle["nbound0"]
        assert abs(rec["phi"] - oracle["phi0"]) <= 1e-6 * oracle["phi0"]
        m, g, _ = ctx.map_state()
        assert np.array_equal(m, np.clip(m0, lo, hi))
        ring, phi, recs = ctx.debug_map_rows(), rec["phi"], []
        for it in range(Cs.ITERS):
            pairs = _pairs_of(ring)
            dlib = ctx.debug_map_direction(ring["rows"], ring["head"], ring["count"], ring["sy"], ring["yy"], m, g, lo, hi, 1.0)
            rec = ctx.map_step()
            recs.append(rec)
            m1, g1, pred1 = ctx.map_state()
            ring1 = ctx.debug_map_rows()
            rp = R.replay_step(m, g, phi, pairs, lo, hi, rec["phi_trial"], m1, g1, resets=rec["resets"], history=Cs.HISTORY)
            assert rp["accepted"] and (rp["alpha"], rp["backtracks"]) == (rec["alpha"], rec["backtracks"]), (it, rp, rec)
            assert (rp["pair_stored"], rp["npairs"], rp["nbound"]) == (rec["pair_stored"], rec["npairs"], rec["nbound"]), (it, rp, rec)
            assert ring1["count"] == rec["npairs"] and ring1["iter"] == it + 1 == rec["iter"]
            # gamma, g'd, s'y: sums of n terms against the reference's longdouble ones
            n = len(m)
            assert abs(rec["gamma"] - rp["gamma"]) <= 8 * EPS * abs(rp["gamma"])
            gabs = float(np.abs(g) @ np.abs(dlib["d"]))
            assert abs(rec["gTd"] - rp["gTd"]) <= 64 * Cs.DIRECTION_BOUND * gabs + 4 * EPS * np.log2(n) * gabs
            assert abs(rec["sTy"] - rp["sTy"]) <= 4 * EPS * np.log2(n) * float(np.abs(m1 - m) @ np.abs(g1 - g))
            assert np.abs(dlib["d"] - rp["d"]).max() <= 64 * Cs.DIRECTION_BOUND * np.abs(rp["d"]).max() * max(1, len(pairs))
            # the new model is clip(m + alpha d) with the library's d, bit for bit (the hook runs the product's kernels)
            assert np.array_equal(m1, E.clip(m, dlib["d"], rec["alpha"], lo, hi))
            assert m1.min() >= lo and m1.max() <= hi
            if rec["pair_stored"]:
                k = (ring1["head"] + ring1["count"] - 1) % ring1["history"]
                assert np.array_equal(ring1["rows"][k], m1 - m) and np.array_equal(ring1["rows"][ring1["history"] + k], g1 - g)
                assert ring1["sy"][k, k] == rec["sTy"]
                for i, (s, y) in enumerate(_pairs_of(ring1)[:-1]):
                    ki = (ring1["head"] + i) % ring1["history"]
                    assert abs(ring1["sy"][ki, k] - s @ (g1 - g)) <= 4 * EPS * np.log2(n) * (np.abs(s) @ np.abs(g1 - g))
                    assert abs(ring1["yy"][ki, k] - y @ (g1 - g)) <= 4 * EPS * np.log2(n) * (np.abs(y) @ np.abs(g1 - g))
                    assert ring1["yy"][k, ki] == ring1["yy"][ki, k]
            # phi, D and the gradient are hmcmt_grad's at the returned model (a foreign evaluation between two steps)
            pred, D, gd = ctx.grad(m1)
            M, gp = Cs.prior_terms(inv, mref, m1)
            print(f"{name} it {it}: phi {rec['phi']:.10e} dD {abs(rec['D'] - D) / D:.2e} dM {abs(rec['M'] - M) / max(M, 1e-300):.2e} "
                  f"dg {np.abs(g1 - gd - gp).max() / np.abs(gd + gp).max():.2e} bt {rec['backtracks']} nb {rec['nbound']}")
            assert abs(rec["D"] - D) <= 1e-12 * D and abs(rec["phi"] - (D + M)) <= 1e-12 * (D + M)
            assert np.abs(g1 - (gd + gp)).max() <= 1e-12 * np.abs(gd + gp).max()
            assert rec["phi"] <= phi
            m, g, phi, ring = m1, g1, rec["phi"], ring1
        for k, (a, b) in enumerate(zip(recs, oracle["recs"])):
            assert (a["backtracks"], a["pair_stored"], a["nbound"], a["status"], a["resets"]) == \
                   (b["backtracks"], b["pair_stored"], b["nbound"], b["status"], b["resets"]), (k, a, b)
            assert abs(a["phi"] - b["phi"]) <= 1e-6 * b["phi"], (k, a["phi"], b["phi"])
        assert np.abs(m - oracle["m"]).max() <= 1e-4
        assert 1 + sum(r["nfevals"] for r in recs) == oracle["nfevals"]
    finally:
        ctx.close()


def test_the_run_stalls_on_tiny_and_leaves_the_state_untouched(tiny):
    ctx, inv, m0, mref, lo, hi = tiny
    oracle = Cs.oracle_run("tiny")
    ctx.map_begin(m0, Cs.LAMBDA, lo, hi, history=Cs.HISTORY)
    recs = [ctx.map_step() for _ in range(3)]
    assert [r["status"] for r in recs] == [L.MAP_RUNNING] * 3 and all(r["alpha"] > 0 for r in recs)
    m3, g3, p3 = ctx.map_state()
    rec = ctx.map_step()
    assert rec["status"] == L.MAP_STALLED and rec["resets"] == 1 and rec["alpha"] == 0.0 and rec["iter"] == 3
    assert rec["nfevals"] == oracle["recs"][-1]["nfevals"] and rec["phi"] == recs[-1]["phi"] and rec["D"] == recs[-1]["D"]
    assert np.all(rec["phi_trial"][:11] > rec["phi"])
    m4, g4, p4 = ctx.map_state()
    assert np.array_equal(m3, m4) and np.array_equal(g3, g4) and np.array_equal(p3, p4)
    assert abs(rec["phi"] / oracle["phi0"] - 0.3704) < 5e-5
    with pytest.raises(L.HmcmtError) as e:
        ctx.map_step()
    assert e.value.code == -1
    with pytest.raises(L.HmcmtError):
        ctx.map_run(3)
    assert np.array_equal(ctx.map_state()[0], m3)
    ctx.map_end()


def _records_equal(a, b):
    for k in a:
        if k == "phi_trial":
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def test_state_rules_of_the_calls():
    name = "r9_wide"
    ctx, inv, m0, mref, lo, hi = _context(name, cold=True)
    ctx2 = None
    try:
        n = len(m0)
        # run == steps, a begin over a live run reuses its buffers, a fresh context repeats the bits
        r0 = ctx.map_begin(m0, Cs.LAMBDA, lo, hi, history=4)
        steps = [ctx.map_step() for _ in range(5)]
        ms = ctx.map_state()
        r0b = ctx.map_begin(m0, Cs.LAMBDA, lo, hi, history=4)
        run = ctx.map_run(5)
        _records_equal(r0, r0b)
        assert len(run) == 5
        for a, b in zip(steps, run):
            _records_equal(a, b)
        assert all(np.array_equal(x, y) for x, y in zip(ms, ctx.map_state()))
        ctx2, *_ = _context(name, cold=True)
        _records_equal(r0, ctx2.map_begin(m0, Cs.LAMBDA, lo, hi, history=4))
        for a, b in zip(steps, ctx2.map_run(5)):
            _records_equal(a, b)
        # a forced iteration cap: ENOCONV, the state and the pairs untouched, the next step succeeds
        ring = ctx.debug_map_rows()
        ctx.set_options(maxit=1)
        with pytest.raises(L.HmcmtError) as e:
            ctx.map_step()
        assert e.value.code == -10
        ctx.set_options(maxit=2000)
        ring1 = ctx.debug_map_rows()
        assert all(np.array_equal(x, y) for x, y in zip(ms, ctx.map_state())) and (ring1["head"], ring1["count"]) == (ring["head"], ring["count"])
        assert np.array_equal(ring1["rows"], ring["rows"], equal_nan=True)
        nxt = ctx.map_step()
        _records_equal(nxt, ctx2.map_step())
        # between an asynchronous evaluation and its wait every MAP call is refused
        import torch
        d_m = torch.tensor(m0, device="cuda:0"); d_g = torch.empty(n, dtype=torch.float64, device="cuda:0")
        ctx.grad_device_async(d_m.data_ptr(), None, None, d_g.data_ptr())
        for call in (ctx.map_step, ctx.map_state, ctx.map_end, lambda: ctx.map_begin(m0, Cs.LAMBDA, lo, hi)):
            with pytest.raises(L.HmcmtError) as e:
                call()
            assert e.value.code == -1
        ctx.wait()
        assert ctx.map_step()["iter"] == 7
        # a chain begun before a run and stepped after it re-evaluates its start gradient and is otherwise the chain without the run
        z = np.random.default_rng(2).standard_normal((2, n))
        out = []
        for c, with_run in ((ctx, True), (ctx2, False)):
            c.map_end()
            c.chain_begin(m0, 0.01, Cs.LAMBDA, lo, hi)
            c.chain_momentum(z[0]); a = c.chain_step(3, 0.5)[0]
            if with_run:
                c.map_begin(m0, Cs.LAMBDA, lo, hi); c.map_run(2)
            c.chain_momentum(z[1]); b = c.chain_step(3, 0.5)[0]
            out.append((a, b))
        (a1, b1), (a2, b2) = out
        assert a1 == a2 and b1["nfevals"] == 4 and b2["nfevals"] == 3
        assert {k: v for k, v in b1.items() if k != "nfevals"} == {k: v for k, v in b2.items() if k != "nfevals"}
        assert ctx.map_state()[0].shape == (n,)                # (the run lives beside the chain)
        # set_prior ends the run; no prior, no run
        ctx.set_prior(mref, inv.Wm, np.ones(n))
        with pytest.raises(L.HmcmtError) as e:
            ctx.map_step()
        assert e.value.code == -1
        mesh, data, inv3, *_ = Cs.problem(name)
        ctx3 = L.HipContext(mesh, data, inv3, device_id=0)
        try:
            with pytest.raises(L.HmcmtError) as e:
                ctx3.map_begin(m0, Cs.LAMBDA, lo, hi)
            assert e.value.code == -1 and "hmcmt_set_prior" in str(e.value)
        finally:
            ctx3.close()
    finally:
        ctx.close()
        if ctx2 is not None:
            ctx2.close()


def test_findmap_returns_the_model_and_the_records():
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd.structs import HMCPrior
    mesh, data, inv, m0, mref, lo, hi = Cs.problem("r9_wide")
    inv.refModel = mref
    inv.strModel = m0.copy()
    prior = HMCPrior(sigBounds=[np.exp(lo), np.exp(hi)], regParam=Cs.LAMBDA)
    ctx = L.HipContext(mesh, data, inv, device_id=0)
    try:
        model, st = sampler.findMAP(mesh, data, inv, prior, ctx=ctx, maxiter=Cs.ITERS, history=Cs.HISTORY)
        oracle = Cs.oracle_run("r9_wide")
        assert st.status == "RUNNING" and st.niter == Cs.ITERS and st.nfevals == oracle["nfevals"] and len(st.phi) == Cs.ITERS + 1
        assert np.abs(model - oracle["m"]).max() <= 1e-4 and np.all(np.diff(st.phi) <= 0)
        with pytest.raises(ValueError):
            sampler.findMAP(mesh, data, inv, prior, ctx=ctx, history=99)
    finally:
        ctx.close()
