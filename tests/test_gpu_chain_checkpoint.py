"""Checkpoint and resume of the device chain on the GPU (hmcmt_chain_save, hmcmt_chain_restore): a blob's round trip through a new
context with every accumulator and a low-rank adaptation in an awkward state, the continuation of a restored chain against the
uninterrupted one bit for bit, save as a read-out, the refusals, a warm context, and the sampler's chain_checkpoint= keyword.  The
bitwise tests run on cold contexts with one smoother sweep (tests/test_gpu_chain_adapt_lowrank.py: cold_context), where the gradient
at a model is a function of the model alone; problems: tiny (96 cells) and ragged (390, tails in every 256- and 64-wide launch)."""
import copy
import ctypes
import struct

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd import sampler
from hmcmt2d_amd.lib import HipContext, HmcmtError, HMCMT_MASS_WM
from tests import chain_blob_ref as B
from tests.test_gpu_chain import RHO as RHO_RUN, SEED_RUN, hm_err, prior_of, problem as run_problem
from tests.test_gpu_chain_adapt import REC_KEYS, bits
from tests.test_gpu_chain_adapt_lowrank import LR, NUTS_KEYS, WIN, cold_context
from tests.test_gpu_chain_kernels import HI, LO, REG, normals, problem

pytestmark = pytest.mark.gpu

EINVAL = -1
TOL_H, TOL_M = 1e-6, 1e-7                                  # tests/test_gpu_chain_nuts.py: the bars of a trajectory rebuilt from a cold start
ALL_TAGS = ["CHAN", "MASS", "HIST", "DMOM", "ACOV", "COV ", "ADPT", "ADLR"]
WIN_ONE = dict(nwarmup=10, init_buffer=2, term_buffer=2, base_window=6)     # one window, [2 .. 7]: what it estimates stays in force
DIAG = dict(nwarmup=12, init_buffer=2, term_buffer=2, base_window=3)        # windows [2 .. 4] and [5 .. 9]


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def begin_accumulators(ctx, n, cov=True):
    ctx.chain_hist_begin(np.array([3, 3, n - 1, 0]), 17, -6.0, -3.5)       # (a repeat, the last cell and the first)
    ctx.chain_data_moments_begin()
    ctx.chain_acov_begin(None, 3)
    if cov:
        ctx.chain_cov_begin(np.array([0, n // 2, n - 1]), 4)


def readout(ctx, accs=True, adapt=True, lowrank=True, seeded=True, wm=False, timing=True):
    """everything a chain can be asked, as bytes.  timing=False leaves out host_ms of the low-rank info: a wall-clock time of the window
    end, which a blob carries but two runs that each close the window do not share"""
    m, _, pred = ctx.chain_state()
    out = {"m": bits(m), "pred": bits(pred), "moments": tuple(bits(np.asarray(x)) for x in ctx.chain_moments())}
    if not wm:
        out["mass_diag"] = bits(ctx.chain_mass_diag())
        out["mass_lowrank"] = tuple(bits(x) for x in ctx.chain_mass_lowrank())
    if seeded:
        out["rng"] = ctx.chain_rng_state()
    if adapt:
        out["adapt_info"] = tuple(sorted((k, bits(np.float64(v))) for k, v in ctx.chain_adapt_info().items()))
    if lowrank:
        out["lowrank_info"] = tuple(sorted((k, bits(np.float64(v))) for k, v in ctx.chain_adapt_lowrank_info().items() if timing or k != "host_ms"))
        out["rows"] = tuple(bits(x) for x in ctx.debug_adapt_lowrank_rows())
    if accs:
        out["hist"] = tuple(bits(np.asarray(x)) for x in ctx.chain_hist())
        out["quantiles"] = bits(ctx.chain_quantiles([0.05, 0.5, 0.95]))
        out["dmom"] = tuple(bits(np.asarray(x)) for x in ctx.chain_data_moments(raw=True))
        out["acov"] = tuple(bits(np.asarray(x)) for x in ctx.chain_acov())
        out["ess"] = tuple(bits(x) for x in ctx.chain_ess())
        out["cov"] = tuple(bits(np.asarray(x)) for x in ctx.chain_cov())
        out["corr"] = bits(ctx.chain_corr())
    return out


def rec_key(rec, nuts):
    return tuple(bits(np.float64(rec[k])) for k in REC_KEYS if k != "nfevals") + \
        (tuple(rec[k] for k in NUTS_KEYS) + (bits(np.float64(rec["alpha"])),) if nuts else ())


def cov_scalars(blob):
    return struct.unpack("<5q", B.read(blob)["sections"]["COV "][:40])


# ---- 3. the round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,burnin", [("tiny", 0), ("ragged", 0), ("tiny", 3)], ids=["tiny-wrapped", "ragged-wrapped", "tiny-filling"])
def test_round_trip_through_a_new_context(name, burnin):
    """A seeded chain with all four accumulators and the low-rank adaptation of WIN / LR, saved behind sample 5: inside the first
    window with three stored pairs, two cross-moment commits parked in a batch of four, maxlag 3 with five counted commits (the ring
    has wrapped; burn-in 0, the cross moments begun behind sample 3) or with two (H_2 and H_3 still filling; burn-in 3), histogram
    targets with a repeat.  A new cold context restored from the blob answers every read-out with the same bits."""
    P = problem(name)
    ctx = cold_context(P)
    try:
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=burnin)
        ctx.chain_seed(50, 3)
        begin_accumulators(ctx, P.n, cov=burnin > 0)
        ctx.chain_adapt_begin(**WIN)
        ctx.chain_adapt_lowrank(**LR)
        for it in range(5):
            if it == 3 and burnin == 0:
                ctx.chain_cov_begin(np.array([0, P.n // 2, P.n - 1]), 4)
            ctx.chain_sample(1, 3)
        size = ctx.chain_save_size()
        blob = ctx.chain_save()
        assert blob.size == size and bits(ctx.chain_save()) == bits(blob)
        assert ctx.chain_acov_count() == 5 - burnin and ctx.chain_cov_count() == 2 and cov_scalars(blob) == (3, 0, 4, 2, 2)
        assert len(ctx.debug_adapt_lowrank_rows()[0]) == 3 and ctx.chain_adapt_info()["window_count"] == 3
        # the container, read from the header's text alone: exactly the sections that were begun, CHAN equal to the chain's answers
        ref = B.read(blob)
        info = L.chain_blob_info(blob)
        assert ref["order"] == ALL_TAGS and [t for t, _ in info["sections"]] == ALL_TAGS
        assert [b for _, b in info["sections"]] == [len(ref["sections"][t]) for t in ALL_TAGS]
        assert (info["nAC"], info["nData"], info["mass_kind"], info["seeded"], info["nsamples"], info["nmoments"]) == (P.n, ctx.nData, 0, 1, 5, 5 - burnin)
        chan = B.read_chan(ref["sections"]["CHAN"], P.n, ctx.nData)
        m, _, pred = ctx.chain_state()
        count, mean, m2 = ctx.chain_moments()
        assert bits(chan["m"]) == bits(m) and bits(chan["pred"]) == bits(np.ascontiguousarray(pred).view(np.float64)) and bits(chan["mean"]) == bits(mean)
        assert bits(chan["m2"]) == bits(m2) and (chan["nsamples"], chan["nmoments"], chan["burnin"]) == (5, count, burnin)
        assert (chan["seed"], chan["stream"], chan["t"], chan["seeded"]) == (50, 3, 5, 1) == ctx.chain_rng_state() + (1,)
        assert (chan["dt"], chan["regParam"], chan["lo"], chan["hi"]) == (ctx.chain_adapt_info()["dt"], REG, LO, HI)
        before = readout(ctx)
        assert ctx.chain_save_size() == size - 2 * 8 * P.n                   # (the cross moments' read-out folded the two parked commits in)
    finally:
        ctx.close()
    new = cold_context(P)
    try:
        new.chain_restore(blob)
        assert bits(new.chain_save()) == bits(blob)
        assert readout(new) == before
    finally:
        new.close()


# ---- 4. and 5. continuation; save is a read-out -----------------------------------------------------------------------------------------
def chain(P, kind, nsteps, cut=None, blob=None, save_every_sample=False):
    """samples [first, nsteps) of one of the three chains on a cold context of its own -- from the start, or restored from `blob`
    saved behind sample `cut`.  Returns records, models, the final read-out, the blob saved behind sample `cut` (uninterrupted runs),
    the low-rank rank in force at the end."""
    nuts, wm = kind.startswith("nuts"), kind == "host-wm"
    ctx = cold_context(P)
    try:
        if wm:
            ctx.set_mass(HMCMT_MASS_WM)
        rng = np.random.default_rng(7)
        draws = [(normals(rng, P.n), int(rng.integers(1, 4)), rng.random()) for _ in range(nsteps)]
        if blob is None:
            first = 0
            ctx.chain_begin(P.start, 0.006 if nuts else P.dt, REG, LO, HI, burnin=2)
            begin_accumulators(ctx, P.n)
            if wm:
                ctx.chain_adapt_begin(8, adapt_mass=0)
            else:
                ctx.chain_seed(50, 1)
                ctx.chain_adapt_begin(**{"fixed-diag": DIAG, "nuts-inside": WIN, "nuts-behind": WIN_ONE}[kind])
                if nuts:
                    ctx.chain_adapt_lowrank(**LR)
        else:
            first = cut
            ctx.chain_restore(blob)
        recs, models, saved = [], [], None
        for it in range(first, nsteps):
            if wm:
                ctx.chain_momentum(draws[it][0])
                rec, m, _ = ctx.chain_step(draws[it][1], draws[it][2])
            else:
                rec, m, _ = ctx.chain_nuts_sample(3) if nuts else ctx.chain_sample(1, 3)
            recs.append(rec); models.append(m)
            if save_every_sample or (blob is None and it + 1 == cut):
                b = ctx.chain_save()
                saved = b if it + 1 == cut else saved
        rank = None if wm else len(ctx.chain_mass_lowrank()[2])
        return recs, models, readout(ctx, lowrank=nuts, seeded=not wm, wm=wm, timing=False), saved, rank
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,cut", [("fixed-diag", 5), ("nuts-inside", 5), ("nuts-behind", 11), ("host-wm", 5)])
def test_a_restored_chain_continues_the_uninterrupted_one_bit_for_bit(kind, cut):
    """14 samples uninterrupted against `cut` samples, save, destroy, a new cold context, restore, the rest: every record equal bit for
    bit but nfevals of the first resumed sample, which is exactly one more (its start gradient), every model and every final read-out
    equal bit for bit.  fixed-diag: fixed L from the seeded generator with the diagonal adaptation, cut where its second window opens;
    nuts-inside / nuts-behind: NUTS (max_depth 3) with the low-rank adaptation, cut inside the first window and behind the warm-up with
    the low-rank mass in force; host-wm: the host-fed momentum / step loop under HMCMT_MASS_WM with a step-size warm-up."""
    P = problem("tiny")
    N, nuts = 14, kind.startswith("nuts")
    full = chain(P, kind, N, cut=cut)
    assert full[3] is not None
    if kind == "nuts-behind":
        assert full[4] >= 1, "the window kept no direction: the low-rank mass is not in force behind the warm-up"
        assert B.read(full[3])["mass_kind"] == 2
    if kind == "host-wm":
        assert B.read(full[3])["mass_kind"] == 1 and len(B.read(full[3])["sections"]["MASS"]) == 32
    resumed = chain(P, kind, N, cut=cut, blob=full[3])
    assert len(resumed[0]) == N - cut
    assert [rec_key(r, nuts) for r in resumed[0]] == [rec_key(r, nuts) for r in full[0][cut:]]
    assert [r["nfevals"] for r in resumed[0]] == [full[0][cut]["nfevals"] + 1] + [r["nfevals"] for r in full[0][cut + 1:]]
    assert bits(np.array(resumed[1])) == bits(np.array(full[1][cut:]))
    assert resumed[2] == full[2] and resumed[4] == full[4]
    print(f"\n[{kind}] decisions behind the cut: {[r['accepted'] for r in full[0][cut:]]}, rank in force {full[4]}")


def test_save_is_a_read_out():
    """a chain saved behind every sample gives the bits of one that is never saved"""
    P = problem("tiny")
    a = chain(P, "nuts-inside", 9)
    b = chain(P, "nuts-inside", 9, save_every_sample=True)
    assert [rec_key(r, True) + (r["nfevals"],) for r in a[0]] == [rec_key(r, True) + (r["nfevals"],) for r in b[0]]
    assert bits(np.array(a[1])) == bits(np.array(b[1])) and a[2] == b[2]


# ---- 6. the refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    P, Q = problem("tiny"), problem("ragged")
    ctx, sib, other = cold_context(P), cold_context(P), Q.context()
    bare = HipContext(P.mesh, P.data, P.inv, device_id=0)
    wm = P.context("wm")
    try:
        n = ctypes.c_uint64()
        buf = np.zeros(1 << 16, dtype=np.uint8)
        assert code_of(ctx.chain_save) == EINVAL and code_of(ctx.chain_save_size) == EINVAL                # no chain
        for c in (ctx, sib):
            c.chain_begin(P.start, P.dt, REG, LO, HI)
            c.chain_seed(9, 1)
            begin_accumulators(c, P.n)
            c.chain_sample(1, 3)
        blob = ctx.chain_save()
        small = np.full(blob.size - 8, 0xAB, dtype=np.uint8)                                              # too small a capacity
        assert ctx.lib.hmcmt_chain_save(ctx.h, small.ctypes.data, small.size, ctypes.byref(n)) == EINVAL
        assert n.value == blob.size and (small == 0xAB).all()
        assert ctx.lib.hmcmt_chain_save(ctx.h, None, 0, ctypes.byref(n)) == EINVAL and n.value == blob.size
        assert code_of(lambda: bare.chain_restore(blob)) == EINVAL                                        # no prior
        assert code_of(lambda: other.chain_restore(blob)) == EINVAL                                       # a tiny blob into a ragged context
        wm.chain_begin(P.start, P.dt, REG, LO, HI)
        wmblob = wm.chain_save()
        assert L.chain_blob_info(wmblob)["mass_kind"] == 1
        assert code_of(lambda: sib.chain_restore(wmblob)) == EINVAL                                       # a Wm blob into a diagonal context
        # between grad_device_async and wait
        import torch
        dev = torch.device("cuda", 0)
        d_m = torch.tensor(P.start, dtype=torch.float64, device=dev)
        d_pred, d_mis, d_g = (torch.zeros(k, dtype=torch.float64, device=dev) for k in (2 * ctx.nData, 1, P.n))
        torch.cuda.synchronize()
        ctx.grad_device_async(d_m.data_ptr(), d_pred.data_ptr(), d_mis.data_ptr(), d_g.data_ptr())
        assert code_of(ctx.chain_save) == EINVAL and code_of(ctx.chain_save_size) == EINVAL and code_of(lambda: ctx.chain_restore(blob)) == EINVAL
        ctx.wait()
        # a corrupted blob over a live chain: the chain goes on as its undisturbed sibling does
        for at in (blob.size // 2, 70, blob.size - 1):
            bad = blob.copy(); bad[at] ^= 0x01
            assert code_of(lambda: sib.chain_restore(bad)) == EINVAL
        assert code_of(lambda: sib.chain_restore(blob[:-8])) == EINVAL
        ranged = blob.copy()                                                                              # a valid container whose dt is -dt
        ranged[64 + 24 * 6 + 7] ^= 0x80
        ranged[-8:] = np.frombuffer(struct.pack("<Q", B.checksum(ranged[:-8].tobytes())), dtype=np.uint8)
        assert L.chain_blob_info(ranged)["nsamples"] == 1 and code_of(lambda: sib.chain_restore(ranged)) == EINVAL
        fresh = cold_context(P)
        try:                                                                                              # (ctx evaluated a foreign gradient: a third chain)
            fresh.chain_begin(P.start, P.dt, REG, LO, HI)
            fresh.chain_seed(9, 1)
            begin_accumulators(fresh, P.n)
            a = [fresh.chain_sample(1, 3) for _ in range(3)]
            b = [sib.chain_sample(1, 3) for _ in range(2)]
            assert [rec_key(r[0], False) + (r[0]["nfevals"],) for r in b] == [rec_key(r[0], False) + (r[0]["nfevals"],) for r in a[1:]]
            assert readout(sib, adapt=False, lowrank=False) == readout(fresh, adapt=False, lowrank=False)
        finally:
            fresh.close()
        # a valid restore over a live chain that has other accumulators leaves exactly the blob's
        sib.chain_end()
        sib.chain_begin(P.start, P.dt, REG, LO, HI)
        sib.chain_data_moments_begin()
        plain = sib.chain_save()
        assert [t for t, _ in L.chain_blob_info(plain)["sections"]] == ["CHAN", "MASS", "DMOM"]
        ctx.chain_adapt_begin(8, adapt_mass=0)
        ctx.chain_restore(plain)
        assert bits(ctx.chain_save()) == bits(plain)
        for fn in (ctx.chain_hist, ctx.chain_acov_count, ctx.chain_cov_count, ctx.chain_adapt_info, ctx.chain_rng_state):
            assert code_of(fn) == EINVAL
        assert ctx.chain_data_moments()[0] == 0
        assert code_of(lambda: ctx.chain_step(1, 0.5)) == EINVAL                                          # no momentum is restored
    finally:
        for c in (ctx, sib, other, bare, wm):
            c.close()


# ---- 7. a default (warm) context --------------------------------------------------------------------------------------------------------
def test_a_warm_context_resumes_to_solver_tolerance():
    """On a default context the solves of a restored chain start cold where the uninterrupted chain's start warm, so nothing is
    bitwise: 5 samples, save, a new context, restore, 6 more against the uninterrupted 11.  The decisions are equal; energies agree
    to 1e-6 and models to 1e-7, relative as in tests/test_gpu_chain_nuts.py (measured: energies 1.1e-10, models equal, the smallest
    |u - exp(hdif)| 0.43).  Seed 50, stream 1 (the seed of this file's other
    chains): a decision could flip only where u lies within the energies' error of exp(hdif), so the test first asserts that no
    decision behind the cut has |u - exp(hdif)| < 1e-6 -- a seed that came that close would be reported as that, not as a mismatch."""
    P = problem("tiny")

    def run(first, n, blob=None):
        ctx = P.context()
        try:
            if blob is None:
                ctx.chain_begin(P.start, P.dt, REG, LO, HI)
                ctx.chain_seed(50, 1)
                begin_accumulators(ctx, P.n)
            else:
                ctx.chain_restore(blob)
            out = [ctx.chain_sample(1, 3) for _ in range(first, n)]
            return out, ctx.chain_save(), ctx.chain_moments(), ctx.chain_hist()
        finally:
            ctx.close()

    blob = run(0, 5)[1]
    ctx = P.context()
    try:
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        ctx.chain_seed(50, 1)
        begin_accumulators(ctx, P.n)
        whole = [ctx.chain_sample(1, 3) for _ in range(11)]
        moments, hist = ctx.chain_moments(), ctx.chain_hist()
    finally:
        ctx.close()
    resumed, _, moments2, hist2 = run(5, 11, blob)
    worst_h = worst_m = 0.0
    margins = []
    for t, ((a, ma, _), (b, mb, _)) in enumerate(zip(resumed, whole[5:]), start=5):
        u = L.rng_draw(50, 1, t, 1, 3)[1]
        margins.append(abs(u - np.exp(min(b["hdif"], 0.0))) if b["hdif"] <= 0 else np.inf)
        got, want = (np.array([r[k] for k in ("K0", "K1", "D1", "M1", "D", "M")]) for r in (a, b))
        worst_h, worst_m = max(worst_h, hm_err(got, want)), max(worst_m, np.abs(ma - mb).max() / max(np.abs(mb).max(), 1.0))
    print(f"\nwarm resume: energies {worst_h:.2e}, models {worst_m:.2e}, smallest |u - exp(hdif)| {min(margins):.2e}")
    assert min(margins) >= 1e-6, margins
    assert [a[0]["accepted"] for a in resumed] == [b[0]["accepted"] for b in whole[5:]]
    assert [a[0]["nfevals"] for a in resumed] == [whole[5][0]["nfevals"] + 1] + [b[0]["nfevals"] for b in whole[6:]]
    assert worst_h < TOL_H and worst_m <= TOL_M
    assert moments2[0] == moments[0] and np.abs(moments2[1] - moments[1]).max() <= TOL_M * max(np.abs(moments[1]).max(), 1.0)
    assert hist2[0] == hist[0]


# ---- 8. the sampler's keyword -----------------------------------------------------------------------------------------------------------
class Crash(Exception):
    pass


def cold_sampler_context(mesh, data, inv):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("HMCMT_SWEEPS", "1")
        return HipContext(mesh, data, inv, device_id=0, warm_start="cold")


def same_status(a, b):
    """field for field -- but for host_ms of the low-rank windows, a wall-clock time that each run measures for itself"""
    from tests.test_chain_host import _same
    for st in (a, b):
        for w in ((st.adapt or {}).get("lowrank") or {}).get("windows", []):
            assert w.pop("host_ms") >= 0.0
    for f in ("hmstats", "acceptstats", "nAccept", "nReject", "moments", "hist", "dataMoments", "ess", "cov", "adapt", "nuts", "rng"):
        assert _same(getattr(a, f, None), getattr(b, f, None)), f


@pytest.mark.parametrize("loop", ["library-nuts-lowrank", "host-fed"])
def test_sampler_keyword_resumes_a_killed_run(loop, tmp_path):
    """runHMCSampler(chain_checkpoint=..., chain_checkpoint_every=4) killed by a patched sample call behind its second block of four and
    run again: hmcstats equals the uninterrupted run's field for field on cold contexts, and hmcprior.nfevals is one more (the
    resumed chain's start gradient)."""
    ns, burn = 14, 10
    mesh, data, inv, _ = run_problem("tiny")
    if loop == "host-fed":
        kw = dict(hist={"targets": [3, 3, len(inv.strModel) - 1, 0], "nbins": 17}, ess={"maxlag": 3})
        method = "chain_step"
    else:
        kw = dict(library_rng=(1, 0), nuts={"max_depth": 3}, adapt={"lowrank": {"rank": 4, "max_samples": 8}, "init_buffer": 2, "term_buffer": 2, "base_window": 6})
        method = "chain_nuts_run"                           # (adapt= watches every step: a call is one sample)

    def run(path=None, die_at=None):
        ctx = cold_sampler_context(mesh, data, inv)
        calls, real = [0], getattr(ctx, method)

        def counted(*a, **k):
            calls[0] += 1
            if die_at is not None and calls[0] >= die_at:
                raise Crash()
            return real(*a, **k)

        setattr(ctx, method, counted)
        prior = prior_of(ns, burn)
        try:
            st = sampler.runHMCSampler(mesh, data, copy.deepcopy(inv), prior, np.random.default_rng(SEED_RUN), rhoref=RHO_RUN["tiny"], ctx=ctx,
                                       device_chain=True, keep_samples=False, chain_checkpoint=path, chain_checkpoint_every=4, **kw)[1]
            return st, prior.nfevals, calls[0]
        finally:
            ctx.close()

    full, nf, ncalls = run()
    assert ncalls == ns
    ck = str(tmp_path / "chain.ckpt")
    with pytest.raises(Crash):
        run(ck, die_at=10)                                  # inside sample 10: the file is the flush behind sample 8
    g = np.load(ck)
    assert int(g["it"]) == 8 and L.chain_blob_info(g["blob"])["nsamples"] == 8
    res, nf2, ncalls2 = run(ck)
    assert ncalls2 == ns - 8 and nf2 == nf + 1
    same_status(res, full)
    assert int(np.load(ck)["it"]) == ns
