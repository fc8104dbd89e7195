"""The low-rank mass adaptation on the device (hmcmt_chain_adapt_lowrank, hmcmt_chain_set_mass_lowrank, hmcmt_chain_mass_lowrank;
k_adapt_lr_store, k_adapt_lr_mean, k_adapt_lr_gram, k_adapt_lr_lift, k_adapt_lr_sign): the kernels through a hook against the host
instantiation bit for bit, the stored pairs against the chain's own models and a sibling context's gradient, a window end against
the numpy reference (tests/adapt_lowrank_ref.py), a bitwise replay of an adapted chain through the setters, an adaptation that keeps
no direction against the diagonal one, the state rules, and the sampler's adapt={"lowrank": ...} keyword.  Contexts whose siblings
must reproduce values are cold and run one smoother sweep (HMCMT_SWEEPS=1), as in tests/test_gpu_leapfrog_updates.py."""
import ctypes

import numpy as np
import pytest

from hmcmt2d_amd import sampler
from hmcmt2d_amd.lib import AdaptLowrankOptions, HipContext, HmcmtError
from tests import adapt_lowrank_ref as R
from tests.emul import emul_adapt_lowrank_py as E
from tests.test_gpu_chain import RHO as RHO_RUN, SEED_RUN, prior_of, problem as run_problem, run
from tests.test_gpu_chain_adapt import bits, rec_bits
from tests.test_gpu_chain_kernels import FORCE, HI, LO, REG, normals, problem

pytestmark = pytest.mark.gpu

EINVAL = -1
NUTS_KEYS = ("depth", "nleaves", "stop", "dirs", "selected")


def code_of(fn):
    with pytest.raises(HmcmtError) as e:
        fn()
    return e.value.code


def cold_context(P):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("HMCMT_SWEEPS", "1")                         # (read once, at hmcmt_create)
        ctx = HipContext(P.mesh, P.data, P.inv, device_id=0, warm_start="cold")
    try:
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
    except Exception:
        ctx.close()
        raise
    return ctx


# ---- 1. the kernels through the hook ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["tiny", "ragged", "cfg3"])
def hook(request):
    P = problem(request.param)
    ctx = HipContext(P.mesh, P.data, P.inv, device_id=0)      # (create and set_prior: no solve)
    ctx.set_prior(P.mref, P.inv.Wm, P.invM)
    yield P, ctx
    ctx.close()


@pytest.mark.parametrize("n", [4, 5, 17, 64, 128])
def test_kernels_against_the_host_instantiation(n, hook):
    P, ctx = hook
    X, G, invM = R.rows_problem(P.n, n)
    B = np.random.default_rng(n).standard_normal((2 * n, 9 if n == 17 else 5))
    K, U = ctx.debug_adapt_lowrank(X, G, invM, B)
    assert bits(K) == bits(E.gram(X, G, invM))
    assert bits(U) == bits(E.lift(X, G, invM, B, sign=True))
    K2, U2 = ctx.debug_adapt_lowrank(X, G, invM, B)
    assert bits(K2) == bits(K) and bits(U2) == bits(U)
    K3, none = ctx.debug_adapt_lowrank(X, G, invM)             # (the Gram matrix alone)
    assert none is None and bits(K3) == bits(K)


def test_the_hook_refuses():
    P = problem("tiny")
    ctx = HipContext(P.mesh, P.data, P.inv, device_id=0)
    try:
        X, G, invM = R.rows_problem(P.n, 4)
        assert code_of(lambda: ctx.debug_adapt_lowrank(X, G, invM)) == EINVAL              # no prior
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
        assert code_of(lambda: ctx.debug_adapt_lowrank(X[:3], G[:3], invM)) == EINVAL      # fewer than four pairs
        assert code_of(lambda: ctx.debug_adapt_lowrank(X, G, invM, np.zeros((8, 33)))) == EINVAL
    finally:
        ctx.close()


# ---- 2. and 3. the stored rows, and a window's end against the reference -------------------------------------------------------------
WIN = dict(nwarmup=12, init_buffer=2, term_buffer=2, base_window=6)      # windows [2 .. 7] and [8 .. 9]
LR = dict(rank=4, max_samples=8, cutoff=2.0, gamma=1e-5)
# forced decisions: the first window's six steps are accepted, the rejections stand in front of it and in the second window
SEQ12 = "ARAAAAAAARAA"


def full_gradient(sib, P, m):
    _, _, g = sib.grad(m)
    return g + REG * (P.inv.Wm.tocsr() @ (m - P.mref))


def window_run(P, nuts):
    """12 steps with the windows of WIN on a cold context; behind every step the hook's rows.  Returns per step (record, model, rows X,
    rows G, lowrank info or None, read-out) and the sibling's full gradient at every model."""
    ctx, sib = cold_context(P), cold_context(P)
    try:
        rng = np.random.default_rng(5)
        D, Mn = ctx.chain_begin(P.start, 0.006 if nuts else P.dt, REG, LO, HI)
        if nuts:
            ctx.chain_seed(50, 0)
        ctx.chain_adapt_begin(**WIN)
        ctx.chain_adapt_lowrank(**LR)
        steps = []
        for it in range(12):
            if nuts:
                rec, m, _ = ctx.chain_nuts_sample(3)
            else:
                ctx.chain_momentum(normals(rng, P.n))
                force = SEQ12[it]
                ctx.chain_set_energy(D + FORCE if force == "A" else D - FORCE, Mn)
                rec, m, _ = ctx.chain_step((1, 2)[it % 2], rng.random())
                assert rec["accepted"] == int(force == "A")
                if rec["accepted"]:
                    D, Mn = rec["D"], rec["M"]
                else:
                    ctx.chain_set_energy(D, Mn)
            X, G = ctx.debug_adapt_lowrank_rows()
            steps.append({"rec": rec, "m": m, "X": X, "G": G, "info": ctx.chain_adapt_lowrank_info(), "mass": ctx.chain_mass_lowrank(),
                          "diag": ctx.chain_mass_diag(), "g": full_gradient(sib, P, m)})
        return steps
    finally:
        ctx.close()
        sib.close()


@pytest.fixture(scope="module", params=[("tiny", False), ("ragged", False), ("tiny", True)], ids=["tiny", "ragged", "tiny-nuts"])
def windows(request):
    name, nuts = request.param
    P = problem(name)
    return P, nuts, window_run(P, nuts)


def test_stored_rows_are_the_chains_models_and_full_gradients(windows):
    """row i's draw is the model the step returned, bit for bit; its gradient is the sibling's data gradient there plus
    regParam Wm (m - m_ref), to 1e-9 of the gradient's largest entry (the project's gradient parity).  Steps 2 .. 7 fill rows 0 .. 5,
    step 8 starts the next window at row 0; a rejected step repeats its pair."""
    P, nuts, steps = windows
    worst = 0.0
    for it, s in enumerate(steps):
        if it < 2 or it > 9:
            continue
        row = it - 2 if it <= 7 else it - 8
        if it == 7:
            assert len(s["X"]) == 6                              # (the closed window's rows stay readable until the next pair)
        else:
            assert len(s["X"]) == row + 1
        assert bits(s["X"][row]) == bits(s["m"])
        err = np.abs(s["G"][row] - s["g"]).max() / np.abs(s["g"]).max()
        worst = max(worst, err)
        assert err <= 1e-9, (it, err)
        if row > 0:
            assert bits(s["X"][:row]) == bits(steps[it - 1]["X"][:row]) and bits(s["G"][:row]) == bits(steps[it - 1]["G"][:row])
        if not s["rec"]["accepted"] and row > 0:
            assert bits(s["X"][row]) == bits(s["X"][row - 1]) and bits(s["G"][row]) == bits(s["G"][row - 1])
    kinds = [s["rec"]["accepted"] for s in steps[2:10]]
    assert nuts or (0 in kinds and 1 in kinds)
    print(f"\n[{P.name}{' nuts' if nuts else ''}] stored gradients against the sibling: {worst:.2e}")


def test_a_windows_end_against_the_reference(windows):
    """hmcmt_chain_mass_lowrank behind the step that closes the first window against adapt_lowrank_ref on the stored rows: invM has the
    diagonal rule's bits -- the plain window rule on all six samples -- and stays what hmcmt_chain_mass_diag returns; the rank, the
    dimensions and the orthonormality agree; theta and the projector of the directions whose reference theta is 5 % clear of the
    cutoffs and of every other theta agree to 1e-8 (the bar of tests/test_adapt_lowrank_host.py, test 5), and so do theta_min and
    theta_max over all dimensions.  Measured, theta / projector: tiny 2.1e-11 / 1.3e-12, ragged 7.1e-11 / 7.1e-11, tiny with NUTS samples
    (seed 50) 4.8e-12 / 2.1e-13; theta_min and theta_max to 3.4e-10."""
    P, nuts, steps = windows
    s = steps[7]
    info, (invM, U, lam) = s["info"], s["mass"]
    kw = dict(rank=LR["rank"], cutoff=LR["cutoff"], gamma=LR["gamma"])
    assert info["windows"] == 1 and info["stored"] == 6 and info["stride"] == 1 and info["skipped"] == 0
    assert steps[6]["info"]["windows"] == 0 and steps[9]["info"]["windows"] == 2 and steps[9]["info"]["stored"] == 2
    assert steps[9]["info"]["fallback"] == 1 and len(steps[9]["mass"][2]) == 0       # two pairs: the second window ends on the diagonal
    assert bits(invM) == bits(s["diag"])
    Xw = np.array([t["m"] for t in steps[2:8]])
    assert np.allclose(invM, R.window_invM(Xw), rtol=1e-12, atol=0)
    Ur, lamr, thr = R.estimate(s["X"], s["G"], invM, **kw)
    print(f"\n[{P.name}{' nuts' if nuts else ''}] window 1: dims {info['dims']}, kept {info['rank']} (reference {len(lamr)}), theta {lam}, "
          f"reference {lamr}, defect {info['defect']:.1e}, host {info['host_ms']:.2f} ms, fallback {info['fallback']}")
    assert info["fallback"] == 0 and info["rank"] == len(lam) == len(lamr) >= 1 and info["dims"] == len(thr)
    assert info["defect"] <= 1e-8 and np.abs(U @ U.T - np.eye(len(lam))).max() <= 1e-8
    gaps = []
    for t in lamr:
        others = thr[thr != t]
        gaps.append(min(np.abs(others / t - 1).min(), abs(t / LR["cutoff"] - 1), abs(t * LR["cutoff"] - 1)))
    clear = [k for k, g in enumerate(gaps) if g >= 0.05]
    assert clear, gaps
    dth = np.abs(lam[clear] / lamr[clear] - 1).max()
    dproj = np.abs(U[clear].T @ U[clear] - Ur[clear].T @ Ur[clear]).max()
    dall = max(abs(info["theta_min"] / thr[0] - 1), abs(info["theta_max"] / thr[-1] - 1))
    print(f"   directions {clear}: theta {dth:.2e}, projector {dproj:.2e}; theta_min / theta_max {dall:.2e}")
    assert dth <= 1e-8 and dproj <= 1e-8 and dall <= 1e-8


# ---- 4. replay ---------------------------------------------------------------------------------------------------------------------------
REPLAY = dict(nwarmup=40, init_buffer=5, term_buffer=5, base_window=10)   # windows close behind steps 14 and 34 (counted from 0)
REPLAY_LR = dict(rank=4, max_samples=8)                                   # strides 2 and 3: five and seven pairs


def seeded_chain(P, nuts, nsteps, adapt=None, lowrank=None, replay=None):
    ctx = P.context()
    try:
        ctx.chain_begin(P.start, 0.006 if nuts else P.dt, REG, LO, HI)
        ctx.chain_seed(50, 0)
        if adapt is not None:
            ctx.chain_adapt_begin(**adapt)
            if lowrank is not None:
                ctx.chain_adapt_lowrank(**lowrank)
        out = {"recs": [], "models": [], "dts": [], "masses": {}, "ranks": [], "infos": []}
        done = 0
        for it in range(nsteps):
            if replay is not None:
                ctx.chain_set_dt(replay["dts"][it])
                if it in replay["masses"]:
                    ctx.chain_set_mass_lowrank(*replay["masses"][it])
            out["dts"].append(ctx.chain_adapt_info()["dt"] if adapt is not None else replay["dts"][it])
            rec, m, _ = ctx.chain_nuts_sample(3) if nuts else ctx.chain_sample(1, 3)
            out["recs"].append(rec); out["models"].append(m)
            if adapt is not None:
                info = ctx.chain_adapt_info()
                if info["windows_done"] > done:
                    done = info["windows_done"]
                    out["masses"][it + 1] = ctx.chain_mass_lowrank()
                    if lowrank is not None:
                        out["infos"].append(ctx.chain_adapt_lowrank_info())
            if lowrank is not None:
                out["ranks"].append(len(ctx.chain_mass_lowrank()[2]))
        out["invM"] = ctx.chain_mass_diag()
        return out
    finally:
        ctx.close()


def all_bits(recs, nuts):
    extra = [tuple(r[k] for k in NUTS_KEYS) + (bits(np.float64(r["alpha"])),) for r in recs] if nuts else []
    return rec_bits(recs), extra


@pytest.mark.parametrize("nuts", [False, True], ids=["fixed-L", "nuts"])
def test_replay_of_an_adapted_chain_through_the_setters(nuts):
    P = problem("tiny")
    a = seeded_chain(P, nuts, 60, adapt=REPLAY, lowrank=REPLAY_LR)
    assert sorted(a["masses"]) == [15, 35]
    assert [(i["stored"], i["stride"]) for i in a["infos"]] == [(5, 2), (7, 3)]
    print(f"\n[{'nuts' if nuts else 'fixed L'}] windows: " + "; ".join(f"rank {i['rank']} of {i['dims']} dims, theta {i['theta_min']:.3g} .. {i['theta_max']:.3g}, "
                                                                     f"fallback {i['fallback']}, host {i['host_ms']:.2f} ms" for i in a["infos"]))
    b = seeded_chain(P, nuts, 60, replay=a)
    assert all_bits(a["recs"], nuts) == all_bits(b["recs"], nuts)
    assert bits(np.array(a["models"])) == bits(np.array(b["models"]))
    assert any(len(m[2]) > 0 for m in a["masses"].values())                # (a direction was kept: the replay went through the low-rank mass)


# ---- 5. no direction kept ------------------------------------------------------------------------------------------------------------------
def test_with_no_direction_kept_it_is_the_diagonal_adaptation():
    P = problem("tiny")
    a = seeded_chain(P, False, 44, adapt=REPLAY)
    b = seeded_chain(P, False, 44, adapt=REPLAY, lowrank=dict(rank=4, max_samples=8, cutoff=1e30))
    assert rec_bits(a["recs"]) == rec_bits(b["recs"]) and bits(np.array(a["models"])) == bits(np.array(b["models"]))
    assert a["dts"] == b["dts"] and bits(a["invM"]) == bits(b["invM"])
    assert all(bits(a["masses"][k][0]) == bits(b["masses"][k][0]) for k in a["masses"])
    assert b["ranks"] == [0] * 44 and [i["rank"] for i in b["infos"]] == [0, 0] and [i["fallback"] for i in b["infos"]] == [0, 0]


# ---- 6. the state rules --------------------------------------------------------------------------------------------------------------------
def test_state_rules():
    P = problem("tiny")
    n = P.n
    rng = np.random.default_rng(3)
    U = np.linalg.qr(rng.standard_normal((n, 3)))[0].T
    lam = np.array([4.0, 0.5, 2.5])
    ctx = P.context()
    try:
        assert code_of(lambda: ctx.chain_adapt_lowrank()) == EINVAL                     # no chain
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        ctx.chain_seed(9, 1)
        assert code_of(lambda: ctx.chain_adapt_lowrank()) == EINVAL                     # no adaptation
        assert code_of(ctx.chain_adapt_lowrank_info) == EINVAL
        ctx.chain_adapt_begin(8, adapt_mass=0)
        assert code_of(lambda: ctx.chain_adapt_lowrank()) == EINVAL                     # a step-size-only adaptation
        ctx.chain_adapt_begin(**WIN)
        for bad in (dict(rank=0), dict(rank=33), dict(max_samples=3), dict(max_samples=129), dict(cutoff=1.0), dict(cutoff=float("nan")),
                    dict(gamma=0.0), dict(gamma=float("inf"))):                         # (past the Python wrapper, which checks the same)
            o = AdaptLowrankOptions(**{**dict(rank=4, max_samples=8, cutoff=2.0, gamma=1e-5), **bad})
            assert ctx.lib.hmcmt_chain_adapt_lowrank(ctx.h, ctypes.byref(o)) == EINVAL
        assert ctx.lib.hmcmt_chain_adapt_lowrank(ctx.h, None) == EINVAL
        assert code_of(ctx.chain_adapt_lowrank_info) == EINVAL                          # (nothing has changed: not upgraded)
        ctx.chain_sample(1, 2)
        assert code_of(lambda: ctx.chain_adapt_lowrank()) == EINVAL                     # a step has been counted
        ctx.chain_adapt_begin(**WIN)
        ctx.chain_adapt_lowrank(rank=4, max_samples=8)
        assert code_of(lambda: ctx.chain_adapt_lowrank()) == EINVAL                     # upgraded already
        assert code_of(lambda: ctx.chain_set_mass_lowrank(P.invM, U, lam)) == EINVAL    # the setter during a mass adaptation
        assert ctx.chain_adapt_lowrank_info()["windows"] == 0
        # a foreign trajectory between two steps inside a window: the next step evaluates its own start gradient (one evaluation more
        # in ITS record), its pair is stored from the gradient its decision leaves, nothing is skipped and nothing else evaluates
        recs = [ctx.chain_sample(2, 2)[0] for _ in range(3)]                            # steps 0 .. 2
        ctx.leapfrog(P.start, np.zeros(n), P.dt, 1, REG, LO, HI)
        rec, m, _ = ctx.chain_sample(2, 2)                                              # step 3
        assert [r["nfevals"] for r in recs] == [2, 2, 2] and rec["nfevals"] == 3
        X, G = ctx.debug_adapt_lowrank_rows()
        assert len(X) == 2 and bits(X[1]) == bits(m)
        for _ in range(4):
            ctx.chain_sample(2, 2)                                                      # steps 4 .. 7: the first window closes
        info = ctx.chain_adapt_lowrank_info()
        assert info["windows"] == 1 and info["stored"] == 6 and info["skipped"] == 0
        ctx.chain_adapt_end()
        # the setter between two steps
        before = ctx.chain_mass_lowrank()
        bad = U.copy(); bad[1] = bad[0]
        ctx.chain_momentum(normals(rng, n))
        assert code_of(lambda: ctx.chain_set_mass_lowrank(P.invM, bad, lam)) == EINVAL  # not orthonormal: nothing changes ...
        assert "orthonormal" in str(pytest.raises(HmcmtError, ctx.chain_set_mass_lowrank, P.invM, bad, lam).value)
        assert all(bits(x) == bits(y) for x, y in zip(before, ctx.chain_mass_lowrank()))
        ctx.chain_step(1, 0.5)                                                          # ... the momentum included
        for wrong in (dict(lam=-lam), dict(lam=lam * np.nan), dict(U=np.where(U == U[0, 0], np.inf, U)), dict(invM=-P.invM)):
            args = {**dict(invM=P.invM, U=U, lam=lam), **wrong}
            assert code_of(lambda: ctx.chain_set_mass_lowrank(args["invM"], args["U"], args["lam"])) == EINVAL
        ctx.chain_momentum(normals(rng, n))
        ctx.chain_set_mass_lowrank(P.invM, U, lam)
        assert code_of(lambda: ctx.chain_step(1, 0.5)) == EINVAL                        # the momentum was dropped
        got = ctx.chain_mass_lowrank()
        assert bits(got[0]) == bits(P.invM) and bits(got[1]) == bits(U) and bits(got[2]) == bits(lam)
        assert bits(ctx.chain_mass_diag()) == bits(P.invM)
        rec1, m1, _ = ctx.chain_sample(2, 2)
        assert rec1["nfevals"] == 2                                                     # (the stored gradient stayed valid)
        ctx.chain_set_mass_lowrank(2.0 * P.invM)                                        # rank 0: back to the diagonal
        got = ctx.chain_mass_lowrank()
        assert len(got[2]) == 0 and got[1].shape == (0, n) and bits(got[0]) == bits(2.0 * P.invM)
        ctx.chain_set_mass_diag(P.invM)                                                 # (the diagonal setter works again)
        # hmcmt_set_prior releases everything
        ctx.chain_adapt_begin(8, adapt_mass=0)
        ctx.set_prior(P.mref, P.inv.Wm, P.invM)
        assert code_of(ctx.chain_mass_lowrank) == EINVAL and code_of(ctx.chain_adapt_lowrank_info) == EINVAL
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        assert len(ctx.chain_mass_lowrank()[2]) == 0
    finally:
        ctx.close()
    wm = P.context("wm")
    try:
        wm.chain_begin(P.start, P.dt, REG, LO, HI)
        assert code_of(lambda: wm.chain_set_mass_lowrank(P.invM, U, lam)) == EINVAL     # HMCMT_MASS_WM
        assert code_of(wm.chain_mass_lowrank) == EINVAL
        wm.chain_adapt_begin(8, adapt_mass=0)                                           # (adapt_mass = 1 is refused under M = Wm ...)
        assert code_of(lambda: wm.chain_adapt_lowrank()) == EINVAL                      # ... so there is nothing to upgrade
    finally:
        wm.close()


def test_a_pair_stored_behind_a_foreign_leapfrog():
    """a foreign hmcmt_leapfrog between two steps inside a window, on cold contexts: the step behind it evaluates its own start
    gradient (one evaluation more in its record), and the pair it stores is the model it returned, bit for bit, with the sibling's
    full gradient there to 1e-9 -- not the foreign trajectory's gradient; nothing is skipped."""
    P = problem("tiny")
    ctx, sib = cold_context(P), cold_context(P)
    try:
        ctx.chain_begin(P.start, P.dt, REG, LO, HI)
        ctx.chain_seed(9, 1)
        ctx.chain_adapt_begin(**WIN)
        ctx.chain_adapt_lowrank(rank=4, max_samples=8)
        recs = [ctx.chain_sample(2, 2)[0] for _ in range(3)]                                # steps 0 .. 2; step 2 fills row 0
        ctx.leapfrog(P.start + 0.3, np.ones(P.n), P.dt, 1, REG, LO, HI)
        rec, m, _ = ctx.chain_sample(2, 2)                                                  # step 3
        assert [r["nfevals"] for r in recs] == [3, 2, 2] and rec["nfevals"] == 3
        X, G = ctx.debug_adapt_lowrank_rows()
        g = full_gradient(sib, P, m)
        assert len(X) == 2 and bits(X[1]) == bits(m)
        err = np.abs(G[1] - g).max() / np.abs(g).max()
        print(f"\nstored gradient behind a foreign leapfrog against the sibling: {err:.2e}")
        assert err <= 1e-9
        for _ in range(4):
            ctx.chain_sample(2, 2)
        info = ctx.chain_adapt_lowrank_info()
        assert info["windows"] == 1 and info["stored"] == 6 and info["skipped"] == 0
        t = ctx.debug_adapt_lowrank_time()
        assert t["gram_ms"] > 0 and t["wait_ms"] > 0 and (t["lift_ms"] > 0) == (info["rank"] > 0)
    finally:
        ctx.close()
        sib.close()


@pytest.mark.parametrize("nuts", [False, True], ids=["fixed-L", "nuts"])
def test_a_refused_setter_leaves_the_next_samples_their_bits(nuts):
    """hmcmt_chain_set_mass_lowrank with a non-orthonormal U between two samples of a seeded chain under the diagonal mass: the call
    waits for the stream, allocates, uploads, runs the projections and first-allocates the vectors every non-diagonal mass shares --
    and is refused.  The samples behind it have the records and the models, bit for bit, of a chain on a context of its own that
    never made the call."""
    P = problem("tiny")
    rng = np.random.default_rng(3)
    bad = np.linalg.qr(rng.standard_normal((P.n, 3)))[0].T
    bad[1] = bad[0]
    lam = np.array([4.0, 0.5, 2.5])

    def chain(refuse):
        ctx = P.context()
        try:
            ctx.chain_begin(P.start, 0.006 if nuts else P.dt, REG, LO, HI)
            ctx.chain_seed(9, 1)
            recs, models = [], []
            for it in range(5):
                if refuse and it == 2:
                    assert code_of(lambda: ctx.chain_set_mass_lowrank(P.invM, bad, lam)) == EINVAL
                    assert len(ctx.chain_mass_lowrank()[2]) == 0
                rec, m, _ = ctx.chain_nuts_sample(3) if nuts else ctx.chain_sample(1, 3)
                recs.append(rec); models.append(m)
            return recs, models, ctx.chain_moments()
        finally:
            ctx.close()

    a, b = chain(False), chain(True)
    assert all_bits(a[0], nuts) == all_bits(b[0], nuts)
    assert bits(np.array(a[1])) == bits(np.array(b[1]))
    assert a[2][0] == b[2][0] and all(bits(x) == bits(y) for x, y in zip(a[2][1:], b[2][1:]))


# ---- 7. the sampler ------------------------------------------------------------------------------------------------------------------------
def test_sampler_lowrank_keyword():
    ns, burn = 46, 40
    adapt = {"lowrank": {"rank": 4, "max_samples": 8}, "init_buffer": 5, "term_buffer": 5, "base_window": 10}
    mesh, data, inv, _ = run_problem("tiny")
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        hm, st, hd = sampler.runHMCSampler(mesh, data, inv, prior_of(ns, burn), np.random.default_rng(SEED_RUN), rhoref=RHO_RUN["tiny"], ctx=ctx,
                                           device_chain=True, keep_samples=False, library_rng=(1, 0), nuts={"max_depth": 4}, adapt=adapt)
        seen = ctx.chain_mass_lowrank()
    finally:
        ctx.close()
    lr = st.adapt["lowrank"]
    assert [w["windows"] for w in lr["windows"]] == [1, 2] and [(w["stored"], w["stride"]) for w in lr["windows"]] == [(5, 2), (7, 3)]
    assert bits(lr["invM"]) == bits(seen[0]) and bits(lr["U"]) == bits(seen[1]) and bits(lr["lam"]) == bits(seen[2])
    assert lr["U"].shape == (lr["windows"][-1]["rank"], len(inv.strModel)) and bits(lr["invM"]) == bits(st.adapt["invM"])
    assert st.adapt["windows"] == [(15, 10), (35, 20)]
    plain = run("tiny", prior_of(ns, burn), device_chain=True, keep_samples=False, library_rng=(1, 0), nuts={"max_depth": 4},
                adapt={k: v for k, v in adapt.items() if k != "lowrank"})[1]
    assert "lowrank" not in plain.adapt
