"""The covariance accumulator of the device chain's commit on the GPU (hmcmt_chain_cov_begin, hmcmt_chain_cov, hmcmt_chain_corr;
k_chain_cov_commit, k_chain_cov_flush, k_chain_cov_out, k_chain_corr): mean, variance, covariance and correlation of the committed
models against tests/cov_ref.py under the bounds of tests/test_cov_host.py, bit for bit against the host instantiation of the item
bodies and between batch lengths, and the state rules -- at one partly filled workgroup (tiny, 96 cells) and, on the ragged problem
(390 cells, all rows), 13 row tiles with a partial last one and two column tiles with a partial last one; on the forced chain
(A A R R R A R A) x 3 behind a burn-in of 2 of tests/test_gpu_chain_kernels.py: 22 counted commits."""
import ctypes

import numpy as np
import pytest

from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import cov_ref as R
from tests.emul import emul_cov_py as E
from tests.test_gpu_chain_kernels import BURNIN, HI, LO, REG, SEQ, normals, problem, run_chain

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
NAMES = ["tiny", "ragged"]
SEED = 31
SEQ3 = SEQ * 3
NBINS = 300
BATCHES = [1, 3, 8, 16]


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def chain(P, cov=None, others=False, seq=SEQ3, begin_at=0, at5=None):
    """The forced chain on a context of its own; cov = (rows or None, batch): begun through run_chain's hook in front of step
    `begin_at`; others: an all-cells histogram and autocovariances (7 lags) beside it.  Returns a dict: records, models, committed
    models, the final state, the moments, and what the accumulator holds at the end on the host path and on the device path."""
    out = {}
    ctx = P.context()
    try:
        def between(it):
            if it == begin_at:
                if others:
                    ctx.chain_hist_begin(np.arange(P.n), NBINS, LO, HI)
                    ctx.chain_acov_begin(None, 7)
                if cov is not None:
                    ctx.chain_cov_begin(*cov)
            if it == 5 and at5 is not None:
                out["at5"] = at5(ctx)

        recs, models, ks, _, committed = run_chain(P, ctx, seq, seed=SEED, full=False, between=between)
        out.update(recs=recs, models=models, ks=ks, committed=committed, state=ctx.chain_state(), moments=ctx.chain_moments())
        if others:
            out["hist"] = ctx.chain_hist()
            out["acov"] = ctx.chain_acov()
        if cov is not None:
            import torch
            dev = torch.device("cuda", 0)
            out["cov"] = ctx.chain_cov()
            out["corr"] = ctx.chain_corr()
            nrow, n = out["corr"].shape
            guard = lambda size: torch.full((size + 16,), -77.0, dtype=torch.float64, device=dev)      # (16 words behind the array)
            d = [guard(n), guard(n), guard(nrow * n), guard(nrow * n)]
            torch.cuda.synchronize()
            out["dev_count"] = ctx.chain_cov_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr())
            assert ctx.chain_corr(d[3].data_ptr()) is None
            h = [t.cpu().numpy() for t in d]
            for a, size in zip(h, (n, n, nrow * n, nrow * n)):
                assert np.all(a[size:] == -77.0)
            out["cov_dev"] = (h[0][:n], h[1][:n], h[2][:nrow * n].reshape(nrow, n), h[3][:nrow * n].reshape(nrow, n))
    finally:
        ctx.close()
    return out


_plain = {}


def plain(name):
    """the chain with a histogram and autocovariances and without the covariance (shared, left unchanged): the chain repeats bitwise"""
    if name not in _plain:
        _plain[name] = chain(problem(name), others=True)
    return _plain[name]


def check_cov(run, committed, rows, batch):
    """the accumulator's results against the reference over the committed models under the bounds of the host test, the exact
    equalities of the contract, and the bits of the host instantiation fed the same models; returns (mean, var, cov, corr)"""
    x = np.array(committed).T                                         # [n, N]
    n, N = x.shape
    r = np.arange(n) if rows is None else np.asarray(rows)
    count, mean, var, cov = run["cov"]
    corr = run["corr"]
    assert count == N == run["dev_count"] and cov.shape == corr.shape == (len(r), n) and mean.shape == var.shape == (n,)
    rmean, rvar, rcov, rcorr = R.two_pass(x, rows)
    bmean, bvar, bcov = R.bounds(x, rows)
    em, ev, ec = np.abs(mean - rmean).astype(float), np.abs(var - rvar).astype(float), np.abs(cov - rcov).astype(float)
    worst = max(np.max(e[b > 0] / b[b > 0], initial=0.0) for e, b in ((em, bmean), (ev, bvar), (ec, bcov)))
    bcorr = R.corr_bound(rcov.astype(float), rvar.astype(float), bcov, bvar, rows)
    keep = bcorr <= 0.5
    ecorr = np.abs(corr - rcorr).astype(float)
    print(f"\n[{len(r)} rows x {n} cells, batch {batch}, N {N}] largest error over its bound: values {worst:.3g}, "
          f"corr {np.max(ecorr[keep & (bcorr > 0)] / bcorr[keep & (bcorr > 0)], initial=0.0):.3g}; {(~keep).sum()} of {keep.size} corr left out")
    assert np.all(em <= bmean) and np.all(ev <= bvar) and np.all(ec <= bcov)
    assert (~keep).mean() <= 0.01 and np.all(ecorr[keep] <= bcorr[keep]) and np.all(np.abs(corr) <= 1.0)
    # the equalities of the contract
    assert all(cov[i, c] == var[c] for i, c in enumerate(r))
    moved = var > 0
    assert all(corr[i, c] == (1.0 if moved[c] else 0.0) for i, c in enumerate(r))
    still = np.flatnonzero(x.max(axis=1) == x.min(axis=1))
    assert np.all(var[still] == 0.0) and np.all(cov[:, still] == 0.0) and np.all(corr[:, still] == 0.0)
    assert all(np.all(cov[i] == 0.0) and np.all(corr[i] == 0.0) for i, c in enumerate(r) if c in still)
    if rows is None:
        assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()
    # the host instantiation of the item bodies, fed the same models: the same bits
    st = E.accumulate(x, rows, batch)
    assert same((mean, var, cov), E.readout(st)) and corr.tobytes() == E.corr(st).tobytes()
    # the device path holds the same bits
    assert same(run["cov_dev"], (mean, var, cov, corr))
    return mean, var, cov, corr


_first = {}


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_values_bits_and_batch_independence(name, batch):
    """all cells, a list with repeats, the single cell that moved most; 22 commits: full flushes and (but for batch 1) a partial one
    at the read-out; every batch length gives the bits of the first one run"""
    P = problem(name)
    n = P.n
    v = np.array(plain(name)["committed"])
    moved = int(np.argmax(v.max(axis=0) - v.min(axis=0)))             # the cell that moved most
    for key, rows in (("all", None), ("list", np.array([5, 5, n - 1, 0])), ("one", np.array([moved]))):
        run = chain(P, cov=(rows, batch))
        assert all(np.array_equal(a, b) for a, b in zip(run["committed"], plain(name)["committed"]))
        got = check_cov(run, run["committed"], rows, batch)
        if key == "list":
            assert np.array_equal(got[2][0], got[2][1]) and np.array_equal(got[3][0], got[3][1])      # repeats are rows of their own
        if key == "one":
            assert got[1][moved] > 0 and got[3][0, moved] == 1.0
        first = _first.setdefault((name, key), got)
        assert same(got, first)


@pytest.mark.parametrize("name", NAMES)
def test_chain_is_bitwise_that_without_the_accumulator_and_repeats(name):
    P = problem(name)
    ref = plain(name)
    run = chain(P, cov=(None, 0), others=True)
    assert run["recs"] == ref["recs"] and run["ks"] == ref["ks"]
    assert all(np.array_equal(a, b) for a, b in zip(run["models"], ref["models"]))
    assert all(np.array_equal(a, b) for a, b in zip(run["state"], ref["state"]))
    assert run["moments"][0] == ref["moments"][0] and same(run["moments"][1:], ref["moments"][1:])
    assert run["hist"][0] == ref["hist"][0] and run["hist"][1].tobytes() == ref["hist"][1].tobytes()
    assert run["acov"][0] == ref["acov"][0] and same(run["acov"][1:], ref["acov"][1:])
    again = chain(P, cov=(None, 0), others=True)
    assert again["cov"][0] == run["cov"][0] == len(SEQ3) - BURNIN
    assert same(again["cov"][1:], run["cov"][1:]) and again["corr"].tobytes() == run["corr"].tobytes()


def test_a_begin_in_front_of_step_5_and_a_read_out_inside_a_batch():
    P = problem("tiny")
    run = chain(P, cov=(None, 8), begin_at=5)
    assert run["cov"][0] == len(SEQ3) - 5 and run["moments"][0] == len(SEQ3) - BURNIN
    check_cov(run, run["models"][5:], None, 8)
    # inside the burn-in a begin counts nothing before the burn-in ends
    early = chain(P, cov=(None, 8), begin_at=1)
    assert early["cov"][0] == len(SEQ3) - BURNIN
    whole = check_cov(early, early["committed"], None, 8)
    # a read-out in front of step 5 (3 of 8 commits parked) flushes them and leaves the final bits what they were
    mid = chain(P, cov=(None, 8), at5=lambda ctx: (ctx.chain_cov(), ctx.chain_corr()))
    (count5, mean5, var5, cov5), corr5 = mid["at5"]
    assert count5 == 5 - BURNIN
    st = E.accumulate(np.array(mid["committed"][:count5]).T, None, 8)
    assert same((mean5, var5, cov5), E.readout(st)) and corr5.tobytes() == E.corr(st).tobytes()
    assert same(mid["cov"][1:] + (mid["corr"],), whole)


def test_device_read_out_with_any_of_the_outputs_null():
    """The device path of hmcmt_chain_cov with every choice of outputs: each one asked for holds the bytes of the read-out of all
    three between intact guard words, the count comes with each.  Ten commits at batch 8 on tiny (one flush in the commit, two
    commits parked), a row list with a repeat.  Read-outs of the mean, the variance or both inside a batch flush nothing (the flush
    launches are counted by the timing hook), and the read-out of all three behind them gives the bits of the chain that was never
    read out in between."""
    import itertools
    import torch
    P = problem("tiny")
    n, G = P.n, 16
    seq = SEQ + SEQ[:4]
    ncommit = len(seq) - BURNIN
    rows = np.array([5, 5, n - 1, 0])
    sizes = {"mean": n, "var": n, "cov": len(rows) * n}
    dev = torch.device("cuda", 0)

    def read(ctx, which):
        bufs = {k: torch.full((G + sizes[k] + G,), -77.0, dtype=torch.float64, device=dev) for k in which}
        torch.cuda.synchronize()
        count = ctx.chain_cov_device(*(bufs[k][G:].data_ptr() if k in bufs else None for k in sizes))
        out = {}
        for k, t in bufs.items():
            a = t.cpu().numpy()
            assert np.all(a[:G] == -77.0) and np.all(a[G + sizes[k]:] == -77.0), (which, k)
            out[k] = a[G:G + sizes[k]].tobytes()
        return count, out

    def run(mid):
        ctx = P.context()
        seen = []
        try:
            def between(it):
                if it == 0:
                    ctx.chain_cov_begin(rows, 8)
                    ctx.chain_cov_timing(True)
                if it > BURNIN:
                    seen.append(ctx.chain_state()[0])                 # (what step it - 1 committed)
                if mid and it in (5, 11):                             # three commits parked, one parked
                    for which in (("mean",), ("var",), ("mean", "var")):
                        count, got = read(ctx, which)
                        st = E.accumulate(np.array(seen).T, rows, 8)
                        assert count == it - BURNIN == len(seen) and all(got[k] == a.tobytes() for k, a in zip(("mean", "var"), E.readout(st)) if k in got)

            run_chain(P, ctx, seq, seed=SEED, full=False, between=between)
            assert ctx.chain_cov_timing()["flush"][1] == 1            # (the commit's, at the eighth)
            count, full = read(ctx, tuple(sizes))
            assert count == ncommit and ctx.chain_cov_timing()["flush"][1] == 2
            if not mid:
                assert all(full[k] == a.tobytes() for k, a in zip(sizes, ctx.chain_cov()[1:]))      # (the host path)
                for r in range(len(sizes)):
                    for which in itertools.combinations(sizes, r):
                        count, got = read(ctx, which)
                        assert count == ncommit and set(got) == set(which) and all(got[k] == full[k] for k in which), which
            return full
        finally:
            ctx.close()

    assert run(mid=True) == run(mid=False)


def test_an_all_rejected_chain_gives_exact_zeros():
    P = problem("tiny")
    run = chain(P, cov=(None, 3), seq="R" * 8)
    count, mean, var, cov = run["cov"]
    assert count == 6 and np.all(cov == 0.0) and np.all(var == 0.0) and np.all(run["corr"] == 0.0) and np.array_equal(mean, P.start)


@pytest.mark.parametrize("name", NAMES)
def test_mean_and_variance_agree_with_the_moments(name):
    """hmcmt_chain_moments counts the same commits: m2 / count against var under the sum of the two bounds.  Welford's update
    (item_chain_welford), with X = max|x| and Rg = max x - min x of the cell: its running mean is rounded once per commit and takes
    a rounded quotient, so it is off by at most 2 N u X; both factors of d (x - mu) are off by that plus u Rg, each is at most Rg, and
    the N products are added serially:
        |m2 / N - exact| <= 2 Rg (2 N u X + u Rg) + 3 u Rg^2 + (N + 2) u var =: wv,     |mean - exact| <= 2 N u X =: wm"""
    run = chain(problem(name), cov=([0], 8))
    x = np.array(run["committed"]).T
    N = x.shape[1]
    count, mean, var, _ = run["cov"]
    mcount, mmean, m2 = run["moments"]
    assert mcount == count == N
    rmean, rvar, _, _ = R.two_pass(x, [0])
    bmean, bvar, _ = R.bounds(x, [0])
    X, Rg = np.abs(x).max(axis=1), x.max(axis=1) - x.min(axis=1)
    wm = 2 * N * R.U * X
    wv = 2 * Rg * (wm + R.U * Rg) + 3 * R.U * Rg * Rg + (N + 2) * R.U * rvar.astype(float)
    ev, em = np.abs(m2 / mcount - var), np.abs(mmean - mean)
    print(f"\n[{name}] var against m2 / count: {np.max(ev[bvar + wv > 0] / (bvar + wv)[bvar + wv > 0], initial=0.0):.3g} of the bound, mean {np.max(em / (bmean + wm)):.3g}")
    assert np.all(ev <= bvar + wv) and np.all(em <= bmean + wm)


def test_state_rules_of_the_accumulator():
    P = problem("tiny")
    n = P.n
    rng = np.random.default_rng(3)
    ctx = HipContext(P.mesh, P.data, P.inv, device_id=0)
    lib, h = ctx.lib, ctx.h
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    buf = np.zeros(4 * n)

    def steps(k, L=1):
        for _ in range(k):
            ctx.chain_momentum(normals(rng, n))
            ctx.chain_step(L, 0.5)

    try:
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
        # no chain
        assert code_of(lambda: ctx.chain_cov_begin(None, 0)) == EINVAL
        assert code_of(lambda: ctx.chain_cov()) == EINVAL and code_of(lambda: ctx.chain_corr()) == EINVAL
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=1)
        # a chain, no accumulator begun
        assert code_of(lambda: ctx.chain_cov()) == EINVAL and code_of(lambda: ctx.chain_corr()) == EINVAL
        assert code_of(lambda: ctx.chain_cov_timing()) == EINVAL
        # bad sizes, indices and batch
        for r, B in ((None, 17), (None, -1), ([0, -1], 8), ([0, n], 8), ([2 ** 40], 8), ([0], 17)):
            assert code_of(lambda: ctx.chain_cov_begin(r, B)) == EINVAL, (r, B)
        assert lib.hmcmt_chain_cov_begin(h, 3, None, 8) == EINVAL and lib.hmcmt_chain_cov_begin(h, 0, i64([0]), 8) == EINVAL
        assert lib.hmcmt_chain_cov_begin(h, -1, i64([0]), 8) == EINVAL
        assert code_of(lambda: ctx.chain_cov()) == EINVAL                 # (none of them began one)
        ctx.chain_cov_begin(None, 16)
        ctx.chain_cov_begin([0, 3, 3], 2)                                 # a second begin replaces the first
        n0 = ctypes.c_int64(-1)
        assert lib.hmcmt_chain_cov(h, ctypes.byref(n0), None, None, None, 0) == 0 and n0.value == 0
        assert code_of(lambda: ctx.chain_cov()) == EINVAL and code_of(lambda: ctx.chain_corr()) == EINVAL      # N = 0
        for _ in range(4):                                                # four steps: one inside the burn-in
            ctx.chain_momentum(normals(rng, n))
            ctx.chain_step(2, rng.random())
        count, mean, var, cov = ctx.chain_cov()
        assert count == 3 and cov.shape == (3, n) and np.array_equal(cov[1], cov[2]) and ctx.chain_cov_count() == 3
        assert lib.hmcmt_chain_corr(h, None, 0) == 0 and lib.hmcmt_chain_cov(h, None, buf.ctypes.data, None, None, 0) == 0
        assert np.array_equal(buf[:n], mean) and np.all(buf[n:] == 0.0)
        assert lib.hmcmt_chain_cov(h, None, None, buf.ctypes.data, None, 0) == 0 and np.array_equal(buf[:n], var)
        # a step that fails touches nothing
        before = ctx.chain_cov() + (ctx.chain_corr(),)
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)                                          # an iteration cap no solve on this mesh meets
        ctx.chain_momentum(normals(rng, n))
        assert code_of(lambda: ctx.chain_step(2, 0.5)) == ENOCONV
        after = ctx.chain_cov() + (ctx.chain_corr(),)
        assert before[0] == after[0] == 3 and same(before[1:], after[1:])
        ctx.set_options(maxit=maxit)
        steps(1, L=2)
        assert ctx.chain_cov()[0] == 4 and ctx.chain_cov_count() == 4
        # the measurement hook: event pairs round the launches change no result; batch 2 and nothing parked: five commits, two
        # flushes in the commit and one of the read-out
        assert ctx.chain_cov_timing(True) == {"commit": (0.0, 0), "flush": (0.0, 0)}
        steps(5)
        timed_result = ctx.chain_cov() + (ctx.chain_corr(),)
        timed = ctx.chain_cov_timing(False)
        assert timed["commit"][1] == 5 and timed["flush"][1] == 3 and timed["commit"][0] > 0 and timed["flush"][0] > 0
        assert ctx.chain_cov_timing() == {"commit": (0.0, 0), "flush": (0.0, 0)}
        models = []                                                       # the same nine commits untimed, on the host instantiation
        assert timed_result[0] == 9
        ctx.chain_cov_begin([0, 3, 3], 2)                                 # back to four commits for what follows
        for _ in range(4):
            ctx.chain_momentum(normals(rng, n))
            models.append(ctx.chain_step(1, 0.5, outputs=True)[1])
        assert ctx.chain_cov_count() == 4
        ctx.chain_cov_timing(True)                                        # timed and untimed read-outs of the same state: the same bits
        a = ctx.chain_cov() + (ctx.chain_corr(),)
        ctx.chain_cov_timing(False)
        b = ctx.chain_cov() + (ctx.chain_corr(),)
        st = E.accumulate(np.array(models).T, [0, 3, 3], 2)
        assert same(a[1:], b[1:]) and same(a[1:4], E.readout(st)) and a[4].tobytes() == E.corr(st).tobytes()
        # between grad_device_async and wait
        import torch
        dev = torch.device("cuda", 0)
        d_m = torch.from_numpy(P.m_other).to(dev)
        d_pred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device=dev)
        d_mis = torch.zeros(1, dtype=torch.float64, device=dev)
        d_g = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.grad_device_async(d_m.data_ptr(), d_pred.data_ptr(), d_mis.data_ptr(), d_g.data_ptr())
        assert code_of(lambda: ctx.chain_cov_begin(None, 8)) == EINVAL
        assert code_of(lambda: ctx.chain_cov()) == EINVAL and code_of(lambda: ctx.chain_corr()) == EINVAL
        assert code_of(lambda: ctx.chain_cov_timing()) == EINVAL
        ctx.wait()
        assert ctx.chain_cov()[0] == 4
        # a begin over the live chain ends it
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=0)
        assert code_of(lambda: ctx.chain_cov()) == EINVAL and code_of(lambda: ctx.chain_corr()) == EINVAL
        steps(1)                                                          # (and the chain runs on without it)
        assert code_of(lambda: ctx.chain_cov()) == EINVAL
        # set_prior, set_mass and chain_end end it with the chain
        for end in (lambda: ctx.set_prior(P.mref, P.inv.Wm, P.invM), lambda: ctx.set_mass(0), ctx.chain_end):
            ctx.chain_begin(P.start, P.dt, REG, LO, HI)
            ctx.chain_cov_begin([1, 2], 9)
            steps(1)
            assert ctx.chain_cov()[3].shape == (2, n)
            end()
            assert code_of(lambda: ctx.chain_cov()) == EINVAL and code_of(lambda: ctx.chain_corr()) == EINVAL
    finally:
        ctx.close()


def test_sampler_fills_hmcstats_cov():
    """runHMCSampler(device_chain=True, keep_samples=True, cov={...}) on tiny: hmcstats.cov against covOf of the kept samples, each
    under its bound against the reference"""
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd.structs import HMCPrior
    from tests.helpers import make_problem
    mesh, data, inv, m = make_problem("tiny")
    n = len(inv.activeIdx)
    rows = [3, n - 1, 3]
    burn, total = 2, 8
    prior = HMCPrior(totalsamples=total, burninsamples=burn, dt=0.02, timestep=[1, 2], sigBounds=[1e-4, 1.0], regParam=1.0)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        model, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(4), rhoref=100.0, ctx=ctx, device_chain=True,
                                             keep_samples=True, cov={"rows": rows, "batch": 3})
    finally:
        ctx.close()
    c = st.cov
    x = model[:, burn:]
    assert set(c) == {"count", "rows", "mean", "var", "cov", "corr"} and c["count"] == total - burn and np.array_equal(c["rows"], rows)
    ref = sampler.covOf(x, rows)
    rmean, rvar, rcov, rcorr = R.two_pass(x, rows)
    b, bo = R.bounds(x, rows), R.covof_bound(x, rows)
    for i, k in enumerate(("mean", "var", "cov")):
        assert c[k].shape == ref[k].shape and np.all(np.abs(c[k] - ref[k]) <= b[i] + bo[i]), k
    bc = R.corr_bound(rcov.astype(float), rvar.astype(float), b[2], b[1], rows) + R.corr_bound(rcov.astype(float), rvar.astype(float), bo[2], bo[1], rows)
    keep = bc <= 0.5
    assert (~keep).mean() <= 0.01 and np.all(np.abs(c["corr"] - ref["corr"])[keep] <= bc[keep])
    assert st.nAccept >= 1 and np.any(c["var"] > 0)
