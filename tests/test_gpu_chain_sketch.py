"""The row sketch of the device chain's commit on the GPU (hmcmt_chain_sketch_begin, hmcmt_chain_sketch, hmcmt_chain_pca;
k_chain_sketch_commit, k_chain_sketch_gram, k_chain_sketch_shrink, k_chain_sketch_mean, k_chain_sketch_lift): the kernels through the
debug hook bit for bit against the host instantiation of the item bodies (tests/emul/emul_sketch.cpp), the sketch of real commits
against the hook, the guarantee and the PCA bounds of tests/test_sketch_host.py, the state rules, the checkpoint and the sampler's
keyword -- on tiny (96 cells, one partly filled workgroup) and ragged (390 cells: a full 256-wide workgroup and a partial one, six
64-wide shrink workgroups and a partial one) of tests/test_gpu_chain_kernels.py, on its forced chain (A A R R R A R A) x 3 behind a
burn-in of 2: 22 counted commits."""
import contextlib
import ctypes

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd import sampler
from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import sketch_ref as R
from tests.emul import emul_sketch_py as E
from tests.test_gpu_chain_adapt_lowrank import cold_context
from tests.test_gpu_chain_kernels import BURNIN, HI, LO, REG, SEQ, normals, problem, run_chain
from tests.test_sketch_host import PCA_REL, PCA_RES, check_eigenvalues, check_guarantee

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
NAMES = ["tiny", "ragged"]
SEED = 31
SEQ3 = SEQ * 3
NCOUNT = len(SEQ3) - BURNIN
GUARD = 16
RANK = 3
# (problem, ell, rows): 8 Gram rows and four shrinks; 24 Gram rows = one full 16-tile and a partial one, two shrinks; 128 Gram rows,
# eight tiles, the largest size, three shrinks
HOOK_CASES = [("tiny", 4, 22), ("ragged", 4, 22), ("tiny", 12, 38), ("ragged", 12, 38), ("ragged", 64, 300)]


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_sketch(a, b, keys=("x0", "tot", "q", "rows")):
    """two sketch dicts hold the same counters and the same bytes"""
    assert all(a[k] == b[k] for k in ("count", "ell", "fill", "shrinks", "pivot_given")), (a, b)
    assert bits(np.float64(a["Delta"])) == bits(np.float64(b["Delta"]))
    for k in keys:
        assert a[k].shape == b[k].shape and bits(a[k]) == bits(b[k]), k
    return True


def emulate(n, ell, X, pivot, T):
    """the host instantiation fed the rows X with the library's own T at every shrink"""
    return E.commit(E.begin(n, ell, pivot), X, T_given=list(T))


@contextlib.contextmanager
def hook_context(name):
    """a context for the hook (it needs the prior only), open while no chain's context is: one context at a time"""
    ctx = problem(name).context()
    try:
        yield ctx
    finally:
        ctx.close()


def hook(name, rows, ell, pivot=None):
    with hook_context(name) as ctx:
        return ctx.debug_chain_sketch(np.asarray(rows), ell, pivot)


# ---- 1. the kernels through the hook ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ell,N", HOOK_CASES)
def test_hook_kernels_are_the_host_instantiation_bit_for_bit(name, ell, N):
    P = problem(name)
    n = P.n
    X = R.synthetic_chain(n, N, modes=3, seed=ell + N) + P.start[None, :]
    shrinks = (N - ell) // ell
    with hook_context(name) as ctx:
        check_hook(ctx, P, X, ell, N, shrinks)


def check_hook(ctx, P, X, ell, N, shrinks):
    n, name = P.n, P.name
    for pivot in (None, P.start + 0.25):
        out = ctx.debug_chain_sketch(X, ell, pivot)
        assert (out["count"], out["ell"], out["shrinks"], out["fill"], out["pivot_given"]) == (N, ell, shrinks, N - shrinks * ell, int(pivot is not None))
        assert out["K"].shape == (shrinks, 2 * ell, 2 * ell) and out["T"].shape == (shrinks, ell, 2 * ell)
        st = emulate(n, ell, X, pivot, out["T"])
        # the commit's sums and rows, every Gram matrix, and (below) every shrunk B given the library's own T
        assert bits(out["x0"]) == bits(st["x0"]) == bits(X[0] if pivot is None else pivot)
        assert bits(out["tot"]) == bits(st["tot"]) and bits(out["q"]) == bits(st["q"])
        assert bits(out["rows"]) == bits(st["B"][:st["fill"]])
        for s in range(shrinks):
            assert bits(out["K"][s]) == bits(st["K"][s]), s
            assert bits(out["K"][s]) == bits(np.ascontiguousarray(out["K"][s].T))
            # the library's T is the host code's, up to how two compilers contract the Jacobi rotations: T T' = diag(c^2) to 1e-9,
            # and row i is the emulation's up to its sign wherever the eigenvalue d_i stands clear of its neighbours (an eigenvector
            # moves by about eps |K| / gap under a perturbation of eps |K|; rows with eps |K| / gap above 1e-9 are left out, row 0
            # never is: a transposed or misordered V fails here)
            assert np.abs(np.abs(out["T"][s] @ out["T"][s].T) - np.abs(st["T"][s] @ st["T"][s].T)).max() <= 1e-9
            d = np.linalg.eigvalsh(st["K"][s])[::-1]
            gap = np.minimum(np.abs(np.diff(d))[:ell], np.concatenate([[np.inf], np.abs(np.diff(d))[:ell - 1]]))
            clear = np.finfo(float).eps * d[0] / np.maximum(gap, 1e-300) <= 1e-9
            assert clear[0], (s, d[:3])
            for i in np.flatnonzero(clear):
                a, b = out["T"][s][i], st["T"][s][i]
                assert min(np.abs(a - b).max(), np.abs(a + b).max()) <= 1e-6, (s, i)
            cut = ctx.debug_chain_sketch(X[:2 * ell + s * ell], ell, pivot)
            assert cut["shrinks"] == s + 1 and cut["fill"] == ell and bits(cut["rows"]) == bits(st["shrunk"][s]), s
            assert bits(cut["K"][s]) == bits(out["K"][s]) and bits(cut["T"][s]) == bits(out["T"][s])
        # the library's Delta is its own eigenvalues' sum; the emulation's the same to rounding
        assert abs(out["Delta"] - st["Delta"]) <= 1e-10 * out["Delta"]
        # the end result under the guarantee and the eigenvalue bound of the host test
        A = X - out["x0"][None, :]
        sk = dict(out)
        s_ = check_guarantee(sk, A, f"hook {name} ell {ell} N {N}")
        lam, U, err = sampler.pcaFromSketch(sk, RANK)
        check_eigenvalues(lam, err, A, s_, f"hook {name} ell {ell} N {N}")
        # again: the same bytes
        again = ctx.debug_chain_sketch(X, ell, pivot)
        assert same_sketch(again, out) and bits(again["K"]) == bits(out["K"]) and bits(again["T"]) == bits(out["T"])


def test_hook_refuses_what_the_header_names():
    with hook_context("tiny") as ctx:
        X = np.zeros((5, ctx.nAC))
        for ell in (1, 65):
            assert code_of(lambda: ctx.debug_chain_sketch(X, ell)) == EINVAL
        out = ctx.debug_chain_sketch(X, 2, max_shrinks=0)      # K and T are not asked for
    assert out["count"] == 5 and out["shrinks"] == 1 and out["fill"] == 3 and out["K"].shape[0] == 0 and np.all(out["rows"] == 0.0) and out["Delta"] == 0.0


# ---- 2. the forced chain -----------------------------------------------------------------------------------------------------------------
def chain(P, sketch=None, others=False, seq=SEQ3, begin_at=0, at=None, rank=RANK):
    """The forced chain on a context of its own; sketch = (ell, pivot): begun through run_chain's hook in front of step `begin_at`;
    others: an all-cells histogram and autocovariances (7 lags) beside it; at = (step, fn): fn(ctx) in front of that step."""
    out = {}
    ctx = P.context()
    try:
        def between(it):
            if it == begin_at:
                if others:
                    ctx.chain_hist_begin(np.arange(P.n), 300, LO, HI)
                    ctx.chain_acov_begin(None, 7)
                if sketch is not None:
                    ctx.chain_sketch_begin(*sketch)
            if at is not None and it == at[0]:
                out["at"] = at[1](ctx)

        recs, models, ks, _, committed = run_chain(P, ctx, seq, seed=SEED, full=False, between=between)
        out.update(recs=recs, models=models, ks=ks, committed=committed, state=ctx.chain_state(), moments=ctx.chain_moments())
        if others:
            out["hist"] = ctx.chain_hist()
            out["acov"] = ctx.chain_acov()
        if sketch is not None:
            import torch
            dev = torch.device("cuda", 0)
            n, ell = P.n, sketch[0]
            out["sketch"] = ctx.chain_sketch()
            if out["sketch"]["count"] >= 2:
                out["pca"] = ctx.chain_pca(rank)
            fill = out["sketch"]["fill"]
            sizes = {"mean": n, "var": n, "rows": fill * n, "lam": rank, "U": rank * n}
            d = {k: torch.full((GUARD + v + GUARD,), -77.0, dtype=torch.float64, device=dev) for k, v in sizes.items()}
            torch.cuda.synchronize()
            ptr = lambda k: d[k][GUARD:].data_ptr()
            out["dev_info"] = ctx.chain_sketch_device(ptr("mean"), ptr("var"), ptr("rows"))
            if out["sketch"]["count"] >= 2:
                out["dev_kept"], out["dev_err"] = ctx.chain_pca(rank, d_lambda=ptr("lam"), d_U=ptr("U"))
            torch.cuda.synchronize()
            h = {k: t.cpu().numpy() for k, t in d.items()}
            kept = out.get("dev_kept", 0)
            wrote = dict(sizes, lam=kept, U=kept * n)
            for k, a in h.items():
                assert np.all(a[:GUARD] == -77.0) and np.all(a[GUARD + wrote[k]:] == -77.0), k
            out["dev"] = {k: a[GUARD:GUARD + wrote[k]].copy() for k, a in h.items()}
            out["after"] = ctx.chain_sketch()
    finally:
        ctx.close()
    return out


_plain = {}


def plain(name):
    """the chain with a histogram and autocovariances and without the sketch (shared, left unchanged)"""
    if name not in _plain:
        _plain[name] = chain(problem(name), others=True)
    return _plain[name]


def check_pca(run, committed, what):
    """the device's PCA: the bytes of its device path and of a second call, the eigenvalue bound of the header, orthonormal
    directions with the sign convention, and the host instantiation fed the same models to the Gram route's measured accuracy"""
    sk = run["sketch"]
    lam, U, err = run["pca"]
    n, N = U.shape[1], sk["count"]
    X = np.array(committed)
    A = X - sk["x0"][None, :]
    assert err == sk["Delta"] / N == run["dev_err"] and run["dev_kept"] == len(lam) >= 1
    assert bits(run["dev"]["lam"]) == bits(lam) and bits(run["dev"]["U"]) == bits(U)
    s = check_guarantee(sk, A, what)
    check_eigenvalues(lam, err, A, s, what)
    assert np.abs(U @ U.T - np.eye(len(lam))).max() <= 1e-8
    assert all(U[k, np.argmax(np.abs(U[k]))] > 0 for k in range(len(lam)))
    st = E.commit(E.begin(n, sk["ell"], sk["x0"] if sk["pivot_given"] else None), X)
    elam, eU = E.pca(st, RANK)[:2]
    assert len(elam) == len(lam) and np.all(np.abs(lam - elam) <= PCA_REL * lam[0])
    C = R.centred_cov(A)
    if sk["shrinks"] == 0:
        exact = np.linalg.eigvalsh(C)[::-1][:len(lam)]
        # PCA_REL was measured where the smallest component is 2e-5 of the first, and there it is eps lam_1 / lam_k: the Gram route's
        # error is absolute, a multiple of eps lam_1.  So EVERY component is held to PCA_REL of itself or, below that ratio, to the
        # absolute error PCA_REL stands for at it
        bound = np.maximum(PCA_REL * exact, PCA_REL * 2e-5 * lam[0])
        res = max(np.linalg.norm(C @ U[k] - lam[k] * U[k]) / lam[0] for k in range(len(lam)))
        print(f"{what}: {len(lam)} components, {int((lam < 2e-5 * lam[0]).sum())} below 2e-5 of the first; lam / lam_1 {lam / lam[0]}; "
              f"error over bound {np.max(np.abs(lam - exact) / bound):.2e} residual {res:.2e}")
        assert np.all(np.abs(lam - exact) <= bound) and res <= PCA_RES
    # reading changed nothing
    assert same_sketch(run["after"], sk) and bits(run["after"]["mean"]) == bits(sk["mean"])
    assert run["dev_info"] == {k: sk[k] for k in run["dev_info"]}
    for k in ("mean", "var"):
        assert bits(run["dev"][k]) == bits(sk[k])
    assert bits(run["dev"]["rows"]) == bits(sk["rows"])


@pytest.mark.parametrize("ell", [4, 12])
@pytest.mark.parametrize("name", NAMES)
def test_sketch_of_real_commits_is_the_hook_fed_the_committed_models(name, ell):
    P = problem(name)
    run = chain(P, sketch=(ell, None))
    sk = run["sketch"]
    assert all(np.array_equal(a, b) for a, b in zip(run["committed"], plain(name)["committed"]))
    assert sk["count"] == NCOUNT == 22 and sk["shrinks"] == (0 if ell == 12 else 4) and sk["pivot_given"] == 0
    assert same_sketch(sk, hook(name, run["committed"], ell))
    X = np.array(run["committed"])
    N = float(NCOUNT)
    assert bits(sk["mean"]) == bits(sk["x0"] + sk["tot"] / N) and bits(sk["var"]) == bits((sk["q"] - (sk["tot"] * sk["tot"]) / N) / N)
    assert bits(sk["x0"]) == bits(X[0])
    check_pca(run, run["committed"], f"chain {name} ell {ell}")
    if ell == 12:
        assert sk["Delta"] == 0.0 and bits(sk["rows"]) == bits(X - X[0][None, :])


@pytest.mark.parametrize("name", NAMES)
def test_chain_is_bitwise_that_without_the_sketch(name):
    P = problem(name)
    ref = plain(name)
    run = chain(P, sketch=(4, None), others=True)
    assert run["recs"] == ref["recs"] and run["ks"] == ref["ks"]
    assert all(np.array_equal(a, b) for a, b in zip(run["models"], ref["models"]))
    assert all(np.array_equal(a, b) for a, b in zip(run["state"], ref["state"]))
    assert run["moments"][0] == ref["moments"][0] and all(bits(a) == bits(b) for a, b in zip(run["moments"][1:], ref["moments"][1:]))
    assert run["hist"][0] == ref["hist"][0] and bits(run["hist"][1]) == bits(ref["hist"][1])
    assert run["acov"][0] == ref["acov"][0] and all(bits(a) == bits(b) for a, b in zip(run["acov"][1:], ref["acov"][1:]))


def test_a_begin_in_the_middle_and_a_given_pivot():
    P = problem("tiny")
    run = chain(P, sketch=(4, None), begin_at=5)
    assert run["sketch"]["count"] == len(SEQ3) - 5 and run["moments"][0] == NCOUNT
    assert same_sketch(run["sketch"], hook("tiny", run["models"][5:], 4))
    early = chain(P, sketch=(4, None), begin_at=1)           # inside the burn-in a begin counts nothing before the burn-in ends
    assert early["sketch"]["count"] == NCOUNT
    pivot = P.start - 0.125
    given = chain(P, sketch=(4, pivot))
    assert given["sketch"]["pivot_given"] == 1 and bits(given["sketch"]["x0"]) == bits(pivot)
    assert same_sketch(given["sketch"], hook("tiny", given["committed"], 4, pivot))
    check_pca(given, given["committed"], "chain tiny ell 4, pivot given")
    # a read-out and a PCA in front of step 9 (7 commits: behind the first shrink at ell 2 x 2) leave the final bits what they were
    mid = chain(P, sketch=(2, None), at=(9, lambda c: (c.chain_sketch(), c.chain_pca(2), c.chain_pca(2), c.chain_sketch())))
    s1, p1, p2, s2 = mid["at"]
    assert s1["count"] == 9 - BURNIN and s1["shrinks"] == 2 and same_sketch(s1, s2)
    assert all(bits(a) == bits(b) for a, b in zip(p1[:2], p2[:2])) and p1[2] == p2[2]
    assert same_sketch(mid["sketch"], chain(P, sketch=(2, None))["sketch"])


def test_a_nuts_sampled_seeded_chain_feeds_the_sketch():
    P = problem("tiny")
    ctx = P.context()
    try:
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=1)
        ctx.chain_seed(7, 1)
        ctx.chain_sketch_begin(2)
        models = [ctx.chain_nuts_sample(2)[1] for _ in range(4)]
        models += list(ctx.chain_nuts_run(3, 2)[1])
        models.append(ctx.chain_sample(1, 2)[1])
        sk = ctx.chain_sketch()
    finally:
        ctx.close()
    assert sk["count"] == 7 and sk["shrinks"] == 2
    assert same_sketch(sk, hook("tiny", models[1:], 2))


# ---- 3. the state rules ------------------------------------------------------------------------------------------------------------------
def test_state_rules_of_the_sketch():
    P = problem("tiny")
    n = P.n
    rng = np.random.default_rng(3)
    ctx = P.context()
    lib, h = ctx.lib, ctx.h
    info = L.SketchInfo()
    kept, err = ctypes.c_int32(), ctypes.c_double()
    buf = np.zeros(4 * n)
    try:
        assert code_of(lambda: ctx.chain_sketch_begin(4)) == EINVAL                    # no chain
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=0)
        assert code_of(ctx.chain_sketch_info) == EINVAL                               # no sketch begun
        assert code_of(lambda: ctx.chain_pca(2)) == EINVAL
        for ell in (1, 65, -3):
            assert code_of(lambda: ctx.chain_sketch_begin(ell)) == EINVAL
        bad = P.start.copy()
        bad[n - 1] = np.nan
        assert code_of(lambda: ctx.chain_sketch_begin(4, bad)) == EINVAL
        ctx.chain_sketch_begin(4)
        assert ctx.chain_sketch_info() == {"count": 0, "ell": 4, "fill": 0, "shrinks": 0, "Delta": 0.0, "pivot_given": 0}
        assert lib.hmcmt_chain_sketch(h, ctypes.byref(info), buf.ctypes.data, None, None, 0) == EINVAL      # N = 0 and an array
        assert lib.hmcmt_chain_pca(h, 2, ctypes.byref(kept), None, None, ctypes.byref(err), 0) == EINVAL

        def steps(k, L_=1):
            for _ in range(k):
                ctx.chain_momentum(normals(rng, n))
                ctx.chain_step(L_, rng.random())

        steps(1)
        assert ctx.chain_sketch_info()["count"] == 1
        assert code_of(lambda: ctx.chain_pca(2)) == EINVAL                            # N < 2
        steps(2)
        for rank in (0, 33):
            assert code_of(lambda: ctx.chain_pca(rank)) == EINVAL
        assert lib.hmcmt_chain_pca(h, 2, None, None, None, None, 0) == EINVAL          # kept is NULL
        # every output may be NULL
        assert lib.hmcmt_chain_sketch(h, None, None, None, None, 0) == 0
        assert lib.hmcmt_chain_pca(h, 2, ctypes.byref(kept), None, None, None, 0) == 0 and 0 <= kept.value <= 2
        # the PCA twice in a row: the same bytes, the sketch unchanged
        before = ctx.chain_sketch()
        a, b = ctx.chain_pca(2), ctx.chain_pca(2)
        assert all(bits(x) == bits(y) for x, y in zip(a[:2], b[:2])) and a[2] == b[2]
        assert same_sketch(ctx.chain_sketch(), before)
        # a step that fails touches nothing
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)                                          # an iteration cap no solve on this mesh meets
        ctx.chain_momentum(normals(rng, n))
        assert code_of(lambda: ctx.chain_step(2, 0.5)) == ENOCONV
        assert same_sketch(ctx.chain_sketch(), before)
        ctx.set_options(maxit=maxit)
        steps(1, L_=2)
        assert ctx.chain_sketch_info()["count"] == 4
        # the measurement hook changes no result: five commits at ell 4 from fill 4: one shrink = two launches
        assert ctx.chain_sketch_timing(True)["commit"]["launches"] == 0
        steps(5)
        t = ctx.chain_sketch_timing(False)
        assert t["commit"]["launches"] == 5 and t["shrink"]["launches"] == 2 and t["host_ms"] > 0.0 and t["commit"]["ms"] > 0.0
        assert ctx.chain_sketch_info()["shrinks"] == 1 and ctx.chain_sketch_info()["count"] == 9
        # a second begin replaces the first
        ctx.chain_sketch_begin(2, P.start)
        assert ctx.chain_sketch_info() == {"count": 0, "ell": 2, "fill": 0, "shrinks": 0, "Delta": 0.0, "pivot_given": 1}
        steps(2)
        assert ctx.chain_sketch()["rows"].shape == (2, n)
        # a begin over the chain, set_prior and chain_end end the sketch
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=0)
        assert code_of(ctx.chain_sketch_info) == EINVAL
        ctx.chain_sketch_begin(2)
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
        assert code_of(ctx.chain_sketch_info) == EINVAL
    finally:
        ctx.close()


# ---- 4. the checkpoint -------------------------------------------------------------------------------------------------------------------
def seeded(P, nsteps, ell, cut=None, blob=None):
    """samples [first, nsteps) of a seeded chain with the sketch on a cold context of its own, from the start or restored from `blob`
    saved behind sample `cut`; returns the final read-out and the blob saved behind `cut`"""
    ctx = cold_context(P)
    saved = None
    try:
        if blob is None:
            ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=1)
            ctx.chain_seed(50, 3)
            ctx.chain_sketch_begin(ell)
            first = 0
        else:
            ctx.chain_restore(blob)
            assert bits(ctx.chain_save()) == bits(blob)
            first = cut
        for it in range(first, nsteps):
            ctx.chain_sample(1, 2)
            if blob is None and it + 1 == cut:
                saved = ctx.chain_save()
        sk = ctx.chain_sketch()
        return sk, ctx.chain_pca(2), saved
    finally:
        ctx.close()


@pytest.mark.parametrize("cut,fill", [(4, 3), (5, 2)], ids=["half-filled", "behind-a-shrink"])
def test_a_restored_sketch_continues_bit_for_bit(cut, fill):
    P = problem("tiny")
    whole, pca, blob = seeded(P, 8, 2, cut=cut)
    info = L.chain_blob_info(blob)
    assert [t for t, _ in info["sections"]] == ["CHAN", "MASS", "SKCH"]
    assert info["sections"][-1][1] == 48 + 8 * P.n * (3 + fill)
    again, pca2, _ = seeded(P, 8, 2, cut=cut, blob=blob)
    assert whole["count"] == 7 and whole["shrinks"] >= 2 and same_sketch(again, whole)
    assert all(bits(a) == bits(b) for a, b in zip(pca[:2], pca2[:2])) and pca[2] == pca2[2]


def test_a_blob_without_the_sketch_keeps_its_layout_and_a_damaged_one_is_refused():
    P = problem("tiny")
    n = P.n
    ctx = cold_context(P)
    try:
        ctx.chain_begin(P.start, P.dt, REG, LO, HI, burnin=0)
        ctx.chain_seed(50, 3)
        ctx.chain_data_moments_begin()
        ctx.chain_sample(1, 2)
        plain_blob = ctx.chain_save()
        info = L.chain_blob_info(plain_blob)
        assert info["sections"] == [("CHAN", 96 + 8 * (3 * n + 2 * ctx.nData)), ("MASS", 32 + 8 * n), ("DMOM", 8 + 8 * 4 * ctx.nData)]
        ctx.chain_sketch_begin(2)
        ctx.chain_sample(1, 2)
        blob = ctx.chain_save()
        table = L.chain_blob_info(blob)["sections"]
        assert [t for t, _ in table] == ["CHAN", "MASS", "DMOM", "SKCH"] and table[:3] == info["sections"]
        # fill = 2 ell in the SKCH section (and the checksum mended): refused, the running chain untouched
        at = 64 + 24 * len(table) + sum(b for _, b in table[:3])
        bad = blob.copy()
        bad[at + 8:at + 16] = np.frombuffer(np.int64(4).tobytes(), dtype=np.uint8)
        words = bad[:-8].view(np.uint64)
        hsh = 0xcbf29ce484222325
        for w in words.tolist():
            hsh = ((hsh ^ w) * 0x100000001b3) % 2 ** 64
        bad[-8:] = np.frombuffer(np.uint64(hsh).tobytes(), dtype=np.uint8)
        assert L.chain_blob_info(bad)["sections"] == table
        assert code_of(lambda: ctx.chain_restore(bad)) == EINVAL
        assert ctx.chain_sketch_info()["count"] == 1
    finally:
        ctx.close()


# ---- 5. the sampler ----------------------------------------------------------------------------------------------------------------------
def test_sampler_fills_hmcstats_sketch_and_its_mass_runs():
    """runHMCSampler(device_chain=True, sketch={...}) on tiny with the samples kept: hmcstats.sketch against sketchOf of the kept
    samples under the guarantee, then a second run under mass_lowrank=lowRankMassFromSketch(...)"""
    from hmcmt2d_amd.structs import HMCPrior
    from tests.helpers import make_problem
    mesh, data, inv, m = make_problem("tiny")
    burn, total = 2, 9
    prior = HMCPrior(totalsamples=total, burninsamples=burn, dt=0.02, timestep=[1, 2], sigBounds=[1e-4, 1.0], regParam=1.0)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        model, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(4), rhoref=100.0, ctx=ctx, device_chain=True,
                                             keep_samples=True, sketch={"ell": 2, "rank": 2})
        sk = st.sketch
        x = model[:, burn:]
        assert sk["count"] == total - burn and sk["ell"] == 2 and sk["shrinks"] == 2 and st.nAccept >= 1
        A = (x - sk["x0"][:, None]).T
        s = check_guarantee(sk, A, "sampler")
        check_eigenvalues(sk["lam"], sk["err"], A, s, "sampler")
        ref = sampler.sketchOf(x, 2)
        assert bits(ref["x0"]) == bits(sk["x0"]) and bits(ref["tot"]) == bits(sk["tot"]) and np.allclose(ref["var"], sk["var"], rtol=1e-9, atol=1e-14 * float(sk["q"].max()))
        assert np.allclose(sk["explained"], sk["lam"] / sk["var"].sum()) and np.all(sk["explained"] <= 1.0 + 1e-12)
        lam, U, err = sampler.pcaFromSketch(sk, 2)
        assert np.all(np.abs(lam - sk["lam"]) <= PCA_REL * lam[0]) and err == sk["err"]
        mass = sampler.lowRankMassFromSketch(sk, invM=np.full(len(inv.activeIdx), 1e-4), rank=2, cutoff=1.0 + 1e-9)
        assert mass[1].shape[1] == len(inv.activeIdx)
        _, st2, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(4), rhoref=100.0, ctx=ctx, device_chain=True,
                                          keep_samples=False, sketch={"ell": 2, "rank": 2}, mass_lowrank=mass)
        assert st2.sketch["count"] == total - burn and st2.sketch["lam"] is not None
    finally:
        ctx.close()
