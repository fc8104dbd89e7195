"""The autocovariance accumulator of the device chain's commit on the GPU (hmcmt_chain_acov_begin, hmcmt_chain_acov, hmcmt_chain_ess;
k_chain_acov, k_chain_acov_out, k_chain_ess): the streamed autocovariances, tau, ess and window of the committed models against
tests/acov_ref.py under the bounds of tests/test_acov_host.py, and the state rules -- at one partly filled workgroup (tiny, 96
parameters) and a full one plus a partial one (the ragged problem, 390), on the forced chain (A A R R R A R A) x 3 behind a burn-in
of 2 of tests/test_gpu_chain_kernels.py: 22 counted commits."""
import ctypes

import numpy as np
import pytest

from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import acov_ref as R
from tests.test_gpu_chain_kernels import BURNIN, HI, LO, REG, SEQ, normals, problem, run_chain

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
NAMES = ["tiny", "ragged"]
SEED = 31
SEQ3 = SEQ * 3
NBINS = 300


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def chain(P, acov=None, hist=False, seq=SEQ3, begin_at=0, at5=None):
    """The forced chain on a context of its own; acov = (targets or None, maxlag): begun through run_chain's hook in front of step
    `begin_at`; hist: an all-cells histogram beside it.  Returns a dict: records, models, committed models, the final state, the
    moments, and what the accumulator holds at the end on the host path and on the device path."""
    out = {}
    ctx = P.context()
    try:
        def between(it):
            if it == begin_at:
                if hist:
                    ctx.chain_hist_begin(np.arange(P.n), NBINS, LO, HI)
                if acov is not None:
                    ctx.chain_acov_begin(*acov)
            if it == 5 and at5 is not None:
                at5(ctx)

        recs, models, ks, _, committed = run_chain(P, ctx, seq, seed=SEED, full=False, between=between)
        out.update(recs=recs, models=models, ks=ks, committed=committed, state=ctx.chain_state(), moments=ctx.chain_moments())
        if hist:
            out["hist"] = ctx.chain_hist()
        if acov is not None:
            import torch
            dev = torch.device("cuda", 0)
            out["acov"] = ctx.chain_acov()
            out["ess"] = ctx.chain_ess()
            K1, nt = out["acov"][2].shape
            guard = lambda size, dtype, fill: torch.full((size + 16,), fill, dtype=dtype, device=dev)      # (16 words behind the array)
            d_mean, d_acov = guard(nt, torch.float64, -77.0), guard(K1 * nt, torch.float64, -77.0)
            d_tau, d_ess, d_win = guard(nt, torch.float64, -77.0), guard(nt, torch.float64, -77.0), guard(nt, torch.int32, 7)
            torch.cuda.synchronize()
            out["dev_count"] = ctx.chain_acov_device(d_mean.data_ptr(), d_acov.data_ptr())
            assert ctx.chain_ess(d_tau.data_ptr(), d_ess.data_ptr(), d_win.data_ptr()) is None
            h = [t.cpu().numpy() for t in (d_mean, d_acov, d_tau, d_ess, d_win)]
            for a, size, fill in zip(h, (nt, K1 * nt, nt, nt, nt), (-77.0, -77.0, -77.0, -77.0, 7)):
                assert np.all(a[size:] == fill)
            out["acov_dev"] = (h[0][:nt], h[1][:K1 * nt].reshape(K1, nt))
            out["ess_dev"] = (h[2][:nt], h[3][:nt], h[4][:nt])
    finally:
        ctx.close()
    return out


_plain = {}


def plain(name):
    """the chain with a histogram and without the autocovariances (shared, left unchanged): the chain repeats bitwise"""
    if name not in _plain:
        _plain[name] = chain(problem(name), hist=True)
    return _plain[name]


def check_acov(run, committed, targets, K, n):
    """the accumulator's results against the reference over the committed models, under the bounds of the host test; returns the
    number of targets left out of the tau comparison"""
    t = np.arange(n) if targets is None else np.asarray(targets)
    x = np.array(committed)[:, t].T                                   # [ntarget, N]
    N = x.shape[1]
    ref = R.streamed_state(x, K)
    mean_ref, acov_ref, cbound = R.readout(ref)
    count, mean, acov = run["acov"]
    assert count == N == run["dev_count"] and acov.shape == (K + 1, len(t)) and mean.shape == (len(t),)
    err = np.abs(acov - acov_ref)
    print(f"\n[{len(t)} targets, K {K}, N {N}] largest c_k error over its bound {np.max(err[cbound > 0] / cbound[cbound > 0]):.3g}")
    assert np.all(err <= cbound)
    assert np.all(acov[N:] == 0.0)
    two = R.two_pass(x, K)
    assert np.all(np.abs(acov - two) <= cbound + 1e-13 * two[0][None, :])
    assert np.abs(mean - mean_ref).max() <= 4 * R.U * np.abs(mean_ref).max()
    tau_ref, ess_ref, win_ref, gammas = R.geyer(acov_ref, N)
    tb = R.tau_bound(acov_ref, cbound, gammas)
    keep = R.tie_free(gammas)
    left_out = int((~keep).sum())
    tau, ess, win = run["ess"]
    assert left_out <= len(t) // 100, f"{left_out} of {len(t)} targets left out"
    assert np.array_equal(win[keep], win_ref[keep]), f"{left_out} of {len(t)} targets left out"
    assert np.all(np.abs(tau - tau_ref)[keep] <= tb[keep]), f"{left_out} of {len(t)} targets left out"
    assert np.all(np.abs(ess - ess_ref)[keep] <= ((tb / np.abs(tau_ref) + 12 * R.U) * ess_ref)[keep])
    # the device path holds the same bits
    assert run["acov_dev"][0].tobytes() == mean.tobytes() and run["acov_dev"][1].tobytes() == acov.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(run["ess_dev"], run["ess"]))
    return left_out


@pytest.mark.parametrize("K", [1, 7, 8, 70])
@pytest.mark.parametrize("name", NAMES)
def test_autocovariances_tau_ess_window_against_the_reference(name, K):
    """all cells, a list with repeats, a single cell; at K = 70 there are fewer commits than lags and the lags span more than one
    wavefront of runs"""
    P = problem(name)
    n = P.n
    v = np.array(plain(name)["committed"])
    moved = int(np.argmax(v.max(axis=0) - v.min(axis=0)))             # the cell that moved most
    for targets in (None, np.array([5, 5, n - 1, 0]), np.array([moved])):
        run = chain(P, acov=(targets, K))
        assert all(np.array_equal(a, b) for a, b in zip(run["committed"], plain(name)["committed"]))
        check_acov(run, run["committed"], targets, K, n)
        count, mean, acov = run["acov"]
        if targets is not None and len(targets) == 4:
            assert np.array_equal(acov[:, 0], acov[:, 1]) and mean[0] == mean[1]          # repeats are rows of their own
        if targets is not None and len(targets) == 1:
            assert acov[0, 0] > 0 and abs(run["ess"][2][0]) >= 1


@pytest.mark.parametrize("name", NAMES)
def test_chain_is_bitwise_that_without_the_accumulator_and_repeats(name):
    P = problem(name)
    ref = plain(name)
    run = chain(P, acov=(None, 7), hist=True)
    assert run["recs"] == ref["recs"] and run["ks"] == ref["ks"]
    assert all(np.array_equal(a, b) for a, b in zip(run["models"], ref["models"]))
    assert all(np.array_equal(a, b) for a, b in zip(run["state"], ref["state"]))
    assert run["moments"][0] == ref["moments"][0] and all(np.array_equal(a, b) for a, b in zip(run["moments"][1:], ref["moments"][1:]))
    assert run["hist"][0] == ref["hist"][0] and run["hist"][1].tobytes() == ref["hist"][1].tobytes()
    again = chain(P, acov=(None, 7), hist=True)
    assert again["acov"][0] == run["acov"][0] == len(SEQ3) - BURNIN
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again["acov"][1:], run["acov"][1:]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again["ess"], run["ess"]))


def test_a_begin_in_front_of_step_5_counts_only_later_commits():
    P = problem("tiny")
    run = chain(P, acov=(None, 8), begin_at=5)
    assert run["acov"][0] == len(SEQ3) - 5 and run["moments"][0] == len(SEQ3) - BURNIN
    check_acov(run, run["models"][5:], None, 8, P.n)
    # inside the burn-in a begin counts nothing before the burn-in ends
    early = chain(P, acov=(None, 8), begin_at=1)
    assert early["acov"][0] == len(SEQ3) - BURNIN
    check_acov(early, early["committed"], None, 8, P.n)


def test_device_read_out_with_any_of_the_outputs_null():
    """The device paths of hmcmt_chain_acov and hmcmt_chain_ess with every choice of outputs: each one asked for holds the bytes of
    the read-out of all of them (which are the host path's) between intact guard words, and hmcmt_chain_acov's count comes with each.
    Ten commits on tiny, 7 lags, a target list with a repeat."""
    import itertools
    import torch
    P = problem("tiny")
    n, G, K = P.n, 16, 7
    seq = SEQ + SEQ[:4]
    targets = np.array([5, 5, n - 1, 0])
    nt = len(targets)
    sizes = {"mean": nt, "acov": (K + 1) * nt, "tau": nt, "ess": nt, "window": nt}
    dev = torch.device("cuda", 0)
    ctx = P.context()

    def read(fn, names, which):
        """fn into guarded device arrays for the outputs `which` of its outputs `names`, None for the others"""
        fill = lambda k: (torch.int32, 7) if k == "window" else (torch.float64, -77.0)
        bufs = {k: torch.full((G + sizes[k] + G,), fill(k)[1], dtype=fill(k)[0], device=dev) for k in which}
        torch.cuda.synchronize()
        ret = fn(*(bufs[k][G:].data_ptr() if k in bufs else None for k in names))
        out = {}
        for k, t in bufs.items():
            a = t.cpu().numpy()
            assert np.all(a[:G] == fill(k)[1]) and np.all(a[G + sizes[k]:] == fill(k)[1]), (which, k)
            out[k] = a[G:G + sizes[k]].tobytes()
        return ret, out

    try:
        run_chain(P, ctx, seq, seed=SEED, full=False, between=lambda it: ctx.chain_acov_begin(targets, K) if it == 0 else None)
        ncommit = len(seq) - BURNIN
        host = dict(zip(sizes, ctx.chain_acov()[1:] + ctx.chain_ess()))
        for fn, names in ((ctx.chain_acov_device, ("mean", "acov")), (ctx.chain_ess, ("tau", "ess", "window"))):
            ret, full = read(fn, names, names)
            assert ret == (ncommit if fn == ctx.chain_acov_device else None) and all(full[k] == host[k].tobytes() for k in names)
            for r in range(0 if fn == ctx.chain_acov_device else 1, len(names)):      # (chain_ess without a pointer is the host path)
                for which in itertools.combinations(names, r):
                    got = read(fn, names, which)
                    assert got[0] == ret and set(got[1]) == set(which) and all(got[1][k] == full[k] for k in which), which
    finally:
        ctx.close()


def test_an_all_rejected_chain_gives_exact_zeros():
    P = problem("tiny")
    run = chain(P, acov=(None, 7), seq="R" * 8)
    count, mean, acov = run["acov"]
    tau, ess, win = run["ess"]
    assert count == 6 and np.all(acov == 0.0) and np.array_equal(mean, P.start)
    assert np.all(tau == 6.0) and np.all(ess == 1.0) and np.all(win == 0)


def test_state_rules_of_the_accumulator():
    P = problem("tiny")
    n = P.n
    rng = np.random.default_rng(3)
    ctx = HipContext(P.mesh, P.data, P.inv, device_id=0)
    lib, h = ctx.lib, ctx.h
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    buf = np.zeros(80 * n)
    try:
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
        # no chain
        assert code_of(lambda: ctx.chain_acov_begin(None, 7)) == EINVAL
        assert code_of(lambda: ctx.chain_acov()) == EINVAL and code_of(lambda: ctx.chain_ess()) == EINVAL
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=1)
        # a chain, no accumulator begun
        assert code_of(lambda: ctx.chain_acov()) == EINVAL and code_of(lambda: ctx.chain_ess()) == EINVAL
        # bad sizes, lags, indices
        for t, K in ((None, 0), (None, 1024), (None, -1), ([0, -1], 7), ([0, n], 7), ([2 ** 40], 7)):
            assert code_of(lambda: ctx.chain_acov_begin(t, K)) == EINVAL, (t, K)
        assert lib.hmcmt_chain_acov_begin(h, 3, None, 7) == EINVAL and lib.hmcmt_chain_acov_begin(h, 0, i64([0]), 7) == EINVAL
        assert lib.hmcmt_chain_acov_begin(h, -1, i64([0]), 7) == EINVAL
        assert code_of(lambda: ctx.chain_acov()) == EINVAL                # (none of them began one)
        ctx.chain_acov_begin(None, 1023)
        ctx.chain_acov_begin([0, 3, 3], 5)                                # a second begin replaces the first
        n0 = ctypes.c_int64(-1)
        assert lib.hmcmt_chain_acov(h, ctypes.byref(n0), None, None, 0) == 0 and n0.value == 0
        assert code_of(lambda: ctx.chain_acov()) == EINVAL and code_of(lambda: ctx.chain_ess()) == EINVAL      # N = 0
        for _ in range(4):                                                # four steps: one inside the burn-in
            ctx.chain_momentum(normals(rng, n))
            ctx.chain_step(2, rng.random())
        count, mean, acov = ctx.chain_acov()
        assert count == 3 and acov.shape == (6, 3) and np.array_equal(acov[:, 1], acov[:, 2]) and np.all(acov[3:] == 0.0)
        assert lib.hmcmt_chain_ess(h, None, None, None, 0) == 0 and lib.hmcmt_chain_acov(h, None, buf.ctypes.data, None, 0) == 0
        assert np.array_equal(buf[:3], mean)
        # a step that fails touches nothing
        before = (ctx.chain_acov(), ctx.chain_ess())
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)                                          # an iteration cap no solve on this mesh meets
        ctx.chain_momentum(normals(rng, n))
        assert code_of(lambda: ctx.chain_step(2, 0.5)) == ENOCONV
        after = (ctx.chain_acov(), ctx.chain_ess())
        assert before[0][0] == after[0][0] == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(before[0][1:], after[0][1:]))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[1], after[1]))
        ctx.set_options(maxit=maxit)
        ctx.chain_momentum(normals(rng, n))
        ctx.chain_step(2, 0.5)
        assert ctx.chain_acov()[0] == 4 and ctx.chain_acov_count() == 4
        # the measurement hook: event pairs round the launch change no result; K = 5 and four commits so far: one more fills, then steady
        assert ctx.chain_acov_timing(True) == {"filling": (0.0, 0), "steady": (0.0, 0)}
        for _ in range(3):
            ctx.chain_momentum(normals(rng, n))
            ctx.chain_step(1, 0.5)
        timed = ctx.chain_acov_timing(False)
        assert timed["filling"][1] == 1 and timed["steady"][1] == 2 and timed["filling"][0] > 0 and timed["steady"][0] > 0
        assert ctx.chain_acov_timing() == {"filling": (0.0, 0), "steady": (0.0, 0)}
        ctx.chain_acov_begin([0, 3, 3], 5)                                # back to four commits for what follows
        for _ in range(4):
            ctx.chain_momentum(normals(rng, n))
            ctx.chain_step(1, 0.5)
        assert ctx.chain_acov_count() == 4
        # between grad_device_async and wait
        import torch
        dev = torch.device("cuda", 0)
        d_m = torch.from_numpy(P.m_other).to(dev)
        d_pred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device=dev)
        d_mis = torch.zeros(1, dtype=torch.float64, device=dev)
        d_g = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.grad_device_async(d_m.data_ptr(), d_pred.data_ptr(), d_mis.data_ptr(), d_g.data_ptr())
        assert code_of(lambda: ctx.chain_acov_begin(None, 7)) == EINVAL
        assert code_of(lambda: ctx.chain_acov()) == EINVAL and code_of(lambda: ctx.chain_ess()) == EINVAL
        ctx.wait()
        assert ctx.chain_acov()[0] == 4
        # a begin over the live chain ends it
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=0)
        assert code_of(lambda: ctx.chain_acov()) == EINVAL and code_of(lambda: ctx.chain_ess()) == EINVAL
        ctx.chain_momentum(normals(rng, n))
        ctx.chain_step(1, 0.5)                                            # (and the chain runs on without it)
        assert code_of(lambda: ctx.chain_acov()) == EINVAL
        # set_prior, set_mass and chain_end end it with the chain
        for end in (lambda: ctx.set_prior(P.mref, P.inv.Wm, P.invM), lambda: ctx.set_mass(0), ctx.chain_end):
            ctx.chain_begin(P.start, P.dt, REG, LO, HI)
            ctx.chain_acov_begin([1, 2], 9)
            ctx.chain_momentum(normals(rng, n))
            ctx.chain_step(1, 0.5)
            assert ctx.chain_acov()[2].shape == (10, 2)
            end()
            assert code_of(lambda: ctx.chain_acov()) == EINVAL and code_of(lambda: ctx.chain_ess()) == EINVAL
    finally:
        ctx.close()
