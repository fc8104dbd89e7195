"""The optional accumulators of the device chain's commit on the GPU (hmcmt_chain_hist_*, hmcmt_chain_data_moments*; k_chain_hist,
k_chain_quantiles, k_chain_hist_out and the second k_chain_welford launch): counts against numpy for equality, quantiles against
tests/hist_ref.py, data moments against tests/chain_ref.py, and the state rules -- at one partly filled workgroup (tiny, 96
parameters) and a full one plus a partial one (the ragged problem, 390), on the forced chain A A R R R A R A behind a burn-in of 2
of tests/test_gpu_chain_kernels.py."""
import ctypes

import numpy as np
import pytest

from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import chain_ref as R
from tests import hist_ref as H
from tests.helpers import rhophase_problem
from tests.test_gpu_chain_kernels import BURNIN, HI, LO, REG, SEQ, Maxima, Problem, normals, problem, run_chain

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
QS = [0.0, 0.05, 0.25, 0.5, 0.95, 1.0]
NAMES = ["tiny", "ragged"]
SEED = 31


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def chain(P, hist=None, dmom=False, seq=SEQ, begin_at=0, at5=None):
    """The forced chain on a context of its own; hist = (targets, nbins, lo, hi) / dmom: begun through run_chain's hook in front of
    step `begin_at`.  Returns a dict: records, models, committed models, the predicted data after every step, the final state and
    what the accumulators hold at the end (host path, device path, quantiles on both paths)."""
    out = {"preds": []}
    ctx = P.context()
    try:
        def between(it):
            if it > 0:
                out["preds"].append(ctx.chain_state()[2])       # the predicted data after step it - 1
            if it == begin_at:
                if hist is not None:
                    ctx.chain_hist_begin(*hist)
                if dmom:
                    ctx.chain_data_moments_begin()
            if it == 5 and at5 is not None:
                at5(ctx)

        recs, models, ks, _, committed = run_chain(P, ctx, seq, seed=SEED, full=False, between=between)
        out.update(recs=recs, models=models, ks=ks, committed=committed, state=ctx.chain_state(), moments=ctx.chain_moments())
        out["preds"].append(out["state"][2])
        if hist is not None:
            import torch
            out["hist"] = ctx.chain_hist()
            nt, nb = out["hist"][1].shape
            d = torch.full((nt * nb + 16,), 7, dtype=torch.int32, device=torch.device("cuda", 0))          # (a guard behind the array)
            dq = torch.full((len(QS) * nt + 16,), -77.0, dtype=torch.float64, device=torch.device("cuda", 0))
            torch.cuda.synchronize()
            out["hist_dev_count"] = ctx.chain_hist_device(d.data_ptr())
            out["q"] = ctx.chain_quantiles(QS)
            assert ctx.chain_quantiles(QS, d_out=dq.data_ptr()) is None
            dh, dqh = d.cpu().numpy(), dq.cpu().numpy()
            assert np.all(dh[nt * nb:] == 7) and np.all(dqh[len(QS) * nt:] == -77.0)
            out["hist_dev"] = dh[:nt * nb].view(np.uint32).reshape(nt, nb)
            out["q_dev"] = dqh[:len(QS) * nt].reshape(len(QS), nt)
        if dmom:
            out["dmom"] = ctx.chain_data_moments()
            out["dmom_raw"] = ctx.chain_data_moments(raw=True)
    finally:
        ctx.close()
    return out


_plain = {}


def plain(name):
    """the chain without accumulators (shared, left unchanged): its committed values give the ranges -- the chain repeats bitwise"""
    if name not in _plain:
        _plain[name] = chain(problem(name))
    return _plain[name]


def ranges(name):
    """(lo, hi) = the smallest and the largest committed value: one value sits exactly on lo, one gives t == nbins and clamps; and a
    narrower range strictly inside the spread, whose edge bins both receive clamped values"""
    v = np.array(plain(name)["committed"])
    lo, hi = float(v.min()), float(v.max())
    assert hi > lo
    return (lo, hi), (lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo))


def check_hist(run, targets, nbins, lo, hi):
    count, counts = run["hist"]
    ref = H.counts_of(run["committed"], targets, nbins, lo, hi)
    assert count == 6 == len(run["committed"]) and counts.dtype == np.uint32 and counts.shape == ref.shape
    assert np.array_equal(counts, ref)                               # integer for integer
    assert np.all(counts.sum(axis=1) == count)
    assert run["hist_dev_count"] == count and run["hist_dev"].tobytes() == counts.tobytes()
    rv, rb = H.quantiles(ref, count, lo, hi, QS)
    bound = H.quantile_bound(lo, hi)
    errs = [float(np.abs(run[k] - rv).max()) for k in ("q", "q_dev")]
    print(f"\n[quantiles, {len(targets)} targets, {nbins} bins] largest error host path {errs[0]:.3g}, device path {errs[1]:.3g}, bound {bound:.3g}")
    assert run["q"].shape == rv.shape == (len(QS), len(targets))
    assert max(errs) <= bound
    assert np.array_equal(run["q"], run["q_dev"])
    return counts, ref


@pytest.mark.parametrize("name", NAMES)
def test_all_cell_counts_quantiles_and_data_moments(name):
    P = problem(name)
    (lo, hi), _ = ranges(name)
    targets = np.arange(P.n)
    seen = {}

    def at5(ctx):                                                    # after A A R R R: three times the model of step 2
        seen["hist"] = ctx.chain_hist()
        seen["dmom"] = ctx.chain_data_moments(raw=True)
        seen["pred"] = ctx.chain_state()[2]

    ref = plain(name)
    run = chain(P, hist=(targets, 300, lo, hi), dmom=True, at5=at5)
    c5, counts5 = seen["hist"]
    assert c5 == 3 and np.all(counts5.max(axis=1) == 3) and np.all(counts5.sum(axis=1) == 3)          # every row holds a single 3
    assert np.array_equal(np.argmax(counts5, axis=1), H.bin_of(run["models"][1], 300, lo, hi))
    assert seen["dmom"][0] == 3 and np.all(seen["dmom"][2] == 0.0)
    assert np.array_equal(seen["dmom"][1], np.ascontiguousarray(seen["pred"], dtype=np.complex128).view(np.float64))
    counts, _ = check_hist(run, targets, 300, lo, hi)
    v = np.array(run["committed"])
    assert (v == lo).sum() >= 1 and (v == hi).sum() >= 1 and counts[:, 0].sum() >= 1 and counts[:, 299].sum() >= 1
    assert H.bin_of(np.array([lo, hi]), 300, lo, hi).tolist() == [0, 299]
    # the data moments, on the committed predicted data
    mx = Maxima()
    preds = np.array(run["preds"][BURNIN:]).T
    assert preds.shape == (len(run["dmom"][1]), 6) and np.iscomplexobj(preds)
    dc, dmean, dm2 = run["dmom"]
    assert dc == 6
    for part, key in ((np.real, "re"), (np.imag, "im")):
        cr, mean_ref, m2_ref = R.moments(part(preds))
        bmean, bvar = R.moments_bounds(mean_ref, m2_ref, cr)
        moved = m2_ref > 0
        assert moved.any()
        mx.check("mean " + key, np.abs(part(dmean) - mean_ref).max(), bmean)
        mx.check("var " + key, np.abs(part(dm2) / dc - m2_ref / cr)[moved], bvar[moved])
        assert np.all(part(dm2)[~moved] == 0.0)
    raw = run["dmom_raw"]
    assert np.array_equal(raw[1], dmean.view(np.float64)) and np.array_equal(raw[2], dm2.view(np.float64))
    print(f"\n[data moments, {name}] nData {len(dmean)}; largest error over its bound: {mx}")
    # records, moments and state equal those of the chain without the accumulators, bit for bit
    assert run["recs"] == ref["recs"] and run["ks"] == ref["ks"]
    assert all(np.array_equal(a, b) for a, b in zip(run["models"], ref["models"]))
    assert all(np.array_equal(a, b) for a, b in zip(run["preds"], ref["preds"]))
    assert all(np.array_equal(a, b) for a, b in zip(run["state"], ref["state"]))
    assert run["moments"][0] == ref["moments"][0] and all(np.array_equal(a, b) for a, b in zip(run["moments"][1:], ref["moments"][1:]))
    # two runs give the same counts, quantiles and data moments
    again = chain(P, hist=(targets, 300, lo, hi), dmom=True)
    assert again["hist"][0] == 6 and again["hist"][1].tobytes() == counts.tobytes() and again["q"].tobytes() == run["q"].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(again["dmom_raw"][1:], raw[1:]))


@pytest.mark.parametrize("name", NAMES)
def test_repeated_targets_and_a_range_inside_the_spread(name):
    P = problem(name)
    _, (lo, hi) = ranges(name)
    v = np.array(plain(name)["committed"])
    cmin, cmax = int(np.unravel_index(v.argmin(), v.shape)[1]), int(np.unravel_index(v.argmax(), v.shape)[1])   # the cells of the extremes
    targets = np.array([cmin, cmin, P.n - 1, 0, cmax, cmin, P.n // 2, cmax])                              # repeats are rows of their own
    assert (v[:, targets] < lo).any() and (v[:, targets] > hi).any()
    for nbins in (7, 2):
        run = chain(P, hist=(targets, nbins, lo, hi))
        counts, ref = check_hist(run, targets, nbins, lo, hi)
        assert np.array_equal(counts[0], counts[1]) and np.array_equal(counts[0], counts[5]) and np.array_equal(counts[4], counts[7])
        clamped_lo = int((v[:, targets] < lo).sum()); clamped_hi = int((v[:, targets] >= hi).sum())
        assert counts[:, 0].sum() >= clamped_lo >= 1 and counts[:, -1].sum() >= clamped_hi >= 1       # both edge bins hold clamped values


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nbins", [1, 4096])
def test_a_single_target(name, nbins):
    P = problem(name)
    (lo, hi), _ = ranges(name)
    v = np.array(plain(name)["committed"])
    t = int(np.argmax(v.max(axis=0) - v.min(axis=0)))                # the cell that moved most
    run = chain(P, hist=(np.array([t]), nbins, lo, hi))
    counts, _ = check_hist(run, np.array([t]), nbins, lo, hi)
    assert counts.shape == (1, nbins) and (nbins == 1 or (counts > 0).sum() > 1)


def test_imaginary_slots_of_a_real_data_type_are_exactly_zero():
    mesh, data, inv, _, _ = rhophase_problem("tiny")
    base = problem("tiny")
    P = Problem.__new__(Problem)
    P.__dict__.update(base.__dict__)
    P.name, P.mesh, P.data, P.inv = "tiny Rho_Pha", mesh, data, inv
    assert len(inv.strModel) == base.n
    run = chain(P, dmom=True)
    count, mean, m2 = run["dmom_raw"]
    assert count == 6 and mean.shape == m2.shape == (2 * len(inv.obsData),)
    assert np.all(mean[1::2] == 0.0) and np.all(m2[1::2] == 0.0)
    assert np.all(mean[0::2] != 0.0) and (m2[0::2] > 0).any()
    dc, dmean, dm2 = run["dmom"]
    assert dmean.dtype == np.float64 and np.array_equal(dmean, mean[0::2]) and np.array_equal(dm2, m2[0::2])
    preds = np.array(run["preds"][BURNIN:]).T
    assert not np.iscomplexobj(preds)
    cr, mean_ref, m2_ref = R.moments(preds)
    bmean, bvar = R.moments_bounds(mean_ref, m2_ref, cr)
    moved = m2_ref > 0
    assert np.abs(dmean - mean_ref).max() <= bmean and np.all(np.abs(dm2 / dc - m2_ref / cr)[moved] <= bvar[moved])
    assert np.all(dm2[~moved] == 0.0)


def test_a_begin_in_the_middle_of_a_chain_counts_only_later_commits():
    P = problem("tiny")
    (lo, hi), _ = ranges("tiny")
    targets = np.arange(P.n)
    run = chain(P, hist=(targets, 300, lo, hi), dmom=True, begin_at=4)      # in front of step 4: the commits of steps 4 .. 7
    count, counts = run["hist"]
    assert count == 4 and np.array_equal(counts, H.counts_of(run["models"][4:], targets, 300, lo, hi))
    assert run["dmom"][0] == 4 and run["moments"][0] == 6
    cr, mean_ref, _ = R.moments(np.array(run["preds"][4:]).T.real)
    assert np.abs(run["dmom"][1].real - mean_ref).max() <= 4 * np.finfo(float).eps * np.abs(mean_ref).max()
    # inside the burn-in a begin counts nothing before the burn-in ends
    early = chain(P, hist=(targets, 300, lo, hi), begin_at=1)
    assert early["hist"][0] == 6 and np.array_equal(early["hist"][1], H.counts_of(early["committed"], targets, 300, lo, hi))


def test_state_rules_of_the_accumulators():
    P = problem("tiny")
    (lo, hi), _ = ranges("tiny")
    n = P.n
    targets = np.arange(n)
    rng = np.random.default_rng(3)
    ctx = HipContext(P.mesh, P.data, P.inv, device_id=0)
    lib, h = ctx.lib, ctx.h
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    buf = np.zeros(4 * n)
    try:
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
        # no chain
        assert code_of(lambda: ctx.chain_hist_begin(targets, 300, lo, hi)) == EINVAL
        assert code_of(lambda: ctx.chain_data_moments_begin()) == EINVAL
        assert code_of(lambda: ctx.chain_hist()) == EINVAL and code_of(lambda: ctx.chain_data_moments()) == EINVAL
        assert code_of(lambda: ctx.chain_quantiles([0.5])) == EINVAL
        # NULL context
        assert lib.hmcmt_chain_hist_begin(None, n, i64(targets), 300, lo, hi) == EINVAL
        assert lib.hmcmt_chain_hist(None, None, None, 0) == EINVAL
        assert lib.hmcmt_chain_hist_quantiles(None, 1, f64([0.5]), buf.ctypes.data, 0) == EINVAL
        assert lib.hmcmt_chain_data_moments_begin(None) == EINVAL and lib.hmcmt_chain_data_moments(None, None, None, None, 0) == EINVAL
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=1)
        # a chain, no accumulator begun
        assert code_of(lambda: ctx.chain_hist()) == EINVAL and code_of(lambda: ctx.chain_quantiles([0.5])) == EINVAL
        assert code_of(lambda: ctx.chain_data_moments()) == EINVAL
        # bad sizes, ranges, indices
        assert lib.hmcmt_chain_hist_begin(h, n, None, 300, lo, hi) == EINVAL
        for bad in (dict(t=[]), dict(nbins=0), dict(nbins=4097), dict(nbins=-3), dict(lo=hi, hi=lo), dict(hi=lo), dict(lo=float("nan")),
                    dict(hi=float("inf")), dict(lo=-float("inf")), dict(t=[0, -1]), dict(t=[0, n]), dict(t=[2 ** 40])):
            a = dict(t=targets, nbins=300, lo=lo, hi=hi); a.update(bad)
            assert code_of(lambda: ctx.chain_hist_begin(a["t"], a["nbins"], a["lo"], a["hi"])) == EINVAL, bad
        assert code_of(lambda: ctx.chain_hist()) == EINVAL              # (none of them began one)
        ctx.chain_hist_begin(targets, 4096, lo, hi)
        ctx.chain_hist_begin(targets, 300, lo, hi)                      # a second begin replaces the first
        ctx.chain_data_moments_begin()
        assert ctx.chain_hist()[0] == 0 and ctx.chain_hist()[1].shape == (n, 300) and not ctx.chain_hist()[1].any()
        assert code_of(lambda: ctx.chain_quantiles([0.5])) == EINVAL    # N = 0
        # three steps: one inside the burn-in
        for _ in range(3):
            ctx.chain_momentum(normals(rng, n))
            ctx.chain_step(2, rng.random())
        assert ctx.chain_hist()[0] == 2 and ctx.chain_data_moments()[0] == 2
        assert lib.hmcmt_chain_hist_quantiles(h, 0, f64([0.5]), buf.ctypes.data, 0) == EINVAL
        assert lib.hmcmt_chain_hist_quantiles(h, 1, None, buf.ctypes.data, 0) == EINVAL
        assert lib.hmcmt_chain_hist_quantiles(h, 1, f64([0.5]), None, 0) == EINVAL
        for q in ([-1e-9], [1.0 + 1e-9], [0.5, float("nan")]):
            assert code_of(lambda: ctx.chain_quantiles(q)) == EINVAL
        # a step that fails touches neither accumulator
        before = (ctx.chain_hist(), ctx.chain_data_moments(raw=True))
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)                                        # an iteration cap no solve on this mesh meets
        ctx.chain_momentum(normals(rng, n))
        assert code_of(lambda: ctx.chain_step(2, 0.5)) == ENOCONV
        after = (ctx.chain_hist(), ctx.chain_data_moments(raw=True))
        assert before[0][0] == after[0][0] == 2 and before[0][1].tobytes() == after[0][1].tobytes()
        assert before[1][0] == after[1][0] == 2 and all(a.tobytes() == b.tobytes() for a, b in zip(before[1][1:], after[1][1:]))
        ctx.set_options(maxit=maxit)
        ctx.chain_momentum(normals(rng, n))
        ctx.chain_step(2, 0.5)
        assert ctx.chain_hist()[0] == 3 and ctx.chain_data_moments()[0] == 3
        # between grad_device_async and wait
        import torch
        dev = torch.device("cuda", 0)
        d_m = torch.from_numpy(P.m_other).to(dev)
        d_pred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device=dev)
        d_mis = torch.zeros(1, dtype=torch.float64, device=dev)
        d_g = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.grad_device_async(d_m.data_ptr(), d_pred.data_ptr(), d_mis.data_ptr(), d_g.data_ptr())
        assert code_of(lambda: ctx.chain_hist_begin(targets, 300, lo, hi)) == EINVAL
        assert code_of(lambda: ctx.chain_hist()) == EINVAL and code_of(lambda: ctx.chain_quantiles([0.5])) == EINVAL
        assert code_of(lambda: ctx.chain_data_moments_begin()) == EINVAL and code_of(lambda: ctx.chain_data_moments()) == EINVAL
        ctx.wait()
        assert ctx.chain_hist()[0] == 3 and ctx.chain_data_moments()[0] == 3
        # a begin over the live chain ends both
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=0)
        assert code_of(lambda: ctx.chain_hist()) == EINVAL and code_of(lambda: ctx.chain_quantiles([0.5])) == EINVAL
        assert code_of(lambda: ctx.chain_data_moments()) == EINVAL
        ctx.chain_momentum(normals(rng, n))
        ctx.chain_step(1, 0.5)                                          # (and the chain runs on without them)
        assert code_of(lambda: ctx.chain_hist()) == EINVAL
        # set_prior, set_mass and chain_end end them with the chain
        for end in (lambda: ctx.set_prior(P.mref, P.inv.Wm, P.invM), lambda: ctx.set_mass(0), ctx.chain_end):
            ctx.chain_begin(P.start, P.dt, REG, LO, HI)
            ctx.chain_hist_begin(targets[:5], 10, lo, hi)
            ctx.chain_data_moments_begin()
            assert ctx.chain_hist()[1].shape == (5, 10)
            end()
            assert code_of(lambda: ctx.chain_hist()) == EINVAL and code_of(lambda: ctx.chain_data_moments()) == EINVAL
    finally:
        ctx.close()
