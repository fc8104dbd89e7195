"""The No-U-turn sampler of the device chain (hmcmt_chain_nuts_sample, hmcmt_chain_nuts_run; k_nuts_leaf, k_nuts_final): the two kernels
through hmcmt_debug_nuts_leaf against the host instantiation bit for bit, every sample's tree rebuilt from hmcmt_leapfrog_device(L = 1)
steps and tests/nuts_ref.py with hmcmt_rng_nuts' draws, the shapes a tree can take, repeatability, a run against its samples with the
accumulators and a warm-up alongside, a fixed-length sample behind a NUTS sample, the refusals, a failing leaf, and the sampler's
nuts keyword.  Sizes: tiny (96 cells: one partly filled workgroup) and the ragged problem (390: a full and a partial one), under a
non-unit diagonal and the five-direction low-rank mass; the kernels also at 20000 cells (the second grid-stride pass).  max_depth <= 4:
a sample is at most 15 evaluations."""
import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd.lib import HMCMT_MASS_OP_INV
from tests import nuts_ref as N
from tests.emul import emul_nuts_py as E
from tests.test_gpu_chain import hm_err, prior_of, run, same_bits
from tests.test_gpu_chain_adapt import WINDOWS, begin_accumulators, bits, read_accumulators, rec_bits
from tests.test_gpu_chain_kernels import HI, LO, REG, Maxima, check_moments, problem
from tests.test_gpu_chain_seeded import code_of, context
from tests.test_nuts_host import copy_case, leaf_cases, leaf_longdouble

pytestmark = pytest.mark.gpu

EINVAL, ENOCONV = -1, -10
LD = np.longdouble
TOL_H, TOL_M = 1e-6, 1e-7                        # tests/test_gpu_chain.py: device chain against host loop, Hamiltonian terms / samples
MARGIN = 100.0                                   # tolerances a uniform keeps from its threshold, a U-turn's cosine from 0
NUTS_KEYS = ("depth", "nleaves", "stop", "dirs", "selected")
DT = {"tiny": 0.006, "ragged": 0.02}             # step sizes at which these problems' trees double several times within depth 4
# (seed, stream) per replayed chain: found by running the reference over the seeds 1 .. 80 -- the first whose NREPLAY samples keep every
# uniform and every U-turn test at its margin.  The Hamiltonian of these problems is 1e3 to 3e4, so 100 tolerances of a threshold are
# 0.1 to 3 of its value, which most seeds miss in some leaf
REPLAY_SEEDS = {("tiny", "diagonal"): (50, 0), ("tiny", "lowrank"): (50, 0), ("ragged", "diagonal"): (18, 0), ("ragged", "lowrank"): (18, 0)}
NREPLAY = 3


def begin(ctx, P, seed, stream=0, burnin=0, dt=None, lo=LO, hi=HI):
    D, Mn = ctx.chain_begin(P.start, DT[P.name] if dt is None else dt, REG, lo, hi, burnin=burnin)
    ctx.chain_seed(seed, stream)
    return D, Mn


def all_bits(recs):
    return rec_bits(recs), [tuple(r[k] for k in NUTS_KEYS) + (bits(np.float64(r["alpha"])),) for r in recs]


# ---- 1. the kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hook_ctx():
    ctx = context(problem("tiny"))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", [96, 390, 20000])
def test_kernels_against_the_host_instantiation(n, hook_ctx):
    """hmcmt_debug_nuts_leaf = k_nuts_leaf + k_nuts_final on device vectors: 0, 1, 4 and 9 due checkpoints (9: three passes), the
    merged-tree pair, both signs, an even leaf (checkpoint written) and odd ones.  Sums and written vectors equal the host
    instantiation's bit for bit, nothing behind n is touched, and the sums keep n 2^-53 sum |terms| from a longdouble evaluation."""
    import torch
    dev = torch.device("cuda", 0)
    GUARD = 8

    def up(a):
        t = torch.full((n + GUARD,), 7.0, dtype=torch.float64, device=dev)
        t[:n] = torch.from_numpy(np.ascontiguousarray(a))
        return t

    for name, kw in leaf_cases(n).items():
        host = copy_case(kw)
        ref_sums = E.leaf(**host)
        t = {k: up(kw[k]) for k in ("p", "rho_s", "x", "inv_m") if kw.get(k) is not None}
        ckw = [up(a) for a in kw["ck_write"]] if "ck_write" in kw else None
        due = [[up(a) for a in trip] for trip in kw.get("ck_due", ())]
        merged, mt = None, {}
        if "merged" in kw:
            mt = {k: up(v) for k, v in kw["merged"].items() if isinstance(v, np.ndarray)}
            merged = {k: v.data_ptr() for k, v in mt.items()}
            merged["other_backward"] = kw["merged"].get("other_backward", False)
        torch.cuda.synchronize()
        sums = hook_ctx.debug_nuts_leaf(n, t["p"].data_ptr(), t["rho_s"].data_ptr(), x=t["x"].data_ptr() if "x" in t else None,
                                        inv_m=t["inv_m"].data_ptr() if "inv_m" in t else None, backward=kw.get("backward", False),
                                        first=kw.get("first", False), ck_write=[a.data_ptr() for a in ckw] if ckw else None,
                                        ck_due=[[a.data_ptr() for a in trip] for trip in due], merged=merged)
        assert bits(sums) == bits(ref_sums), name
        back = lambda a: a.cpu().numpy()
        assert bits(back(t["rho_s"])[:n]) == bits(host["rho_s"]) and np.all(back(t["rho_s"])[n:] == 7.0), name
        if ckw:
            for a, b in zip(ckw, host["ck_write"]):
                assert bits(back(a)[:n]) == bits(b) and np.all(back(a)[n:] == 7.0), name
        if merged:
            assert bits(back(mt["rho_next"])[:n]) == bits(host["merged"]["rho_next"]) and np.all(back(mt["rho_next"])[n:] == 7.0), name
        for a, src in [(t["p"], kw["p"])] + [(a, b) for trip, rt in zip(due, kw.get("ck_due", ())) for a, b in zip(trip, rt)]:
            assert bits(back(a)[:n]) == bits(src), name                                   # (what a leaf reads stays)
        ref, bound, _ = leaf_longdouble(kw)
        nq = 3 + 2 * len(due)
        assert np.all(np.abs(sums[:nq].astype(LD) - ref[:nq]) <= bound[:nq]) and np.all(sums[nq:] == 0.0), name


# ---- 2. replay ---------------------------------------------------------------------------------------------------------------------------
class Replay:
    """nuts_ref's one-step map on a context of its own: hmcmt_leapfrog_device(L = 1) from host states, the backward step on -p"""

    def __init__(self, P, mass, dt, lo=LO, hi=HI):
        import torch
        self.torch, self.P, self.dt, self.mass, self.lo, self.hi = torch, P, dt, mass, lo, hi
        self.ctx = context(P, mass)
        dev = torch.device("cuda", 0)
        self.d_m, self.d_p = (torch.zeros(P.n, dtype=torch.float64, device=dev) for _ in range(2))
        self.d_pred = torch.zeros(2 * self.ctx.nData, dtype=torch.float64, device=dev)
        self.d_s = torch.zeros(2, dtype=torch.float64, device=dev)

    def close(self):
        self.ctx.close()

    def minv(self, p):
        return self.P.invM * p if self.mass == "diagonal" else self.ctx.mass_apply(HMCMT_MASS_OP_INV, p)

    def state(self, m, p, D, Mn):
        x = self.minv(p)
        K = 0.5 * float(p @ x)
        return N.State(m, p, x, D + Mn + K, D=D, M=Mn, K=K)

    def leaf(self, s, forward):
        torch, sg = self.torch, (1.0 if forward else -1.0)
        self.d_m.copy_(torch.from_numpy(np.ascontiguousarray(s.m)))
        self.d_p.copy_(torch.from_numpy(np.ascontiguousarray(sg * s.p)))
        torch.cuda.synchronize()
        self.ctx.leapfrog_device(self.d_m.data_ptr(), self.d_p.data_ptr(), self.dt, 1, REG, self.lo, self.hi, 0, self.d_pred.data_ptr(),
                                 self.d_s.data_ptr(), self.d_s.data_ptr() + 8)
        self.ctx.wait()
        D, Mn = (float(v) for v in self.d_s.cpu().numpy())
        return self.state(self.d_m.cpu().numpy(), sg * self.d_p.cpu().numpy(), D, Mn)


def replay_chain(P, mass, seed, stream, nsamples, max_depth, dt=None, lo=LO, hi=HI):
    """nsamples NUTS samples of the device chain, each rebuilt by the reference from the chain's own start state and momentum.
    Returns [(record, model, reference result)]."""
    dt = DT[P.name] if dt is None else dt
    ctx, rp = context(P, mass), None
    try:
        rp = Replay(P, mass, dt, lo, hi)
        D, Mn = begin(ctx, P, seed, stream, dt=dt, lo=lo, hi=hi)
        m = P.start.copy()
        out = []
        for t in range(nsamples):
            rec, m1, _ = ctx.chain_nuts_sample(max_depth)
            p0 = ctx.chain_state()[1]                       # (the ends integrate in buffers of their own: the drawn momentum stays)
            start = rp.state(m, p0, D, Mn)
            ref = N.sample(start, rp.leaf, max_depth, lambda j: L.rng_nuts(seed, stream, t, 0, j), lambda l: L.rng_nuts(seed, stream, t, 1, l)[1])
            ref["H0"], ref["K0"] = start.H, start.K
            out.append((rec, m1, ref))
            m, D, Mn = m1, rec["D"], rec["M"]
        return out
    finally:
        ctx.close()
        if rp is not None:
            rp.close()


def alpha_bound(ref):
    """What the energies' tolerance allows alpha = mean_i min(1, exp(delta_i)) to differ by: delta_i = H0 - H_i is good to
    e = 2 TOL_H max(|H0|, 1) (two energies of that size), so leaf i's term lies between min(1, exp(delta_i - e)) and
    min(1, exp(delta_i + e)) -- nothing for a leaf well inside delta > 0, e exp(delta) for one below; a divergent leaf counts 0 in both."""
    e = 2.0 * TOL_H * max(abs(ref["H0"]), 1.0)
    delta = ref["H0"] - np.array(ref["energies"], dtype=float)
    live = np.isfinite(delta) & (-delta <= N.DIVERGENCE)
    with np.errstate(over="ignore"):
        width = np.minimum(1.0, np.exp(delta[live] + e)) - np.minimum(1.0, np.exp(delta[live] - e))
    return float(width.sum()) / len(delta) + 1e-12


def check_replay(rec, m1, ref, where):
    for key in NUTS_KEYS:
        assert rec[key] == ref[key], (where, key, {k: rec[k] for k in NUTS_KEYS}, {k: ref[k] for k in NUTS_KEYS})
    s = ref["state"]
    got, want = np.array([rec["K0"], rec["K1"], rec["D1"], rec["M1"]]), np.array([ref["K0"], s.K, s.D, s.M])
    assert hm_err(got, want) < TOL_H, (where, got, want)
    assert np.abs(m1 - s.m).max() <= TOL_M * max(np.abs(s.m).max(), 1.0), where
    assert abs(rec["alpha"] - ref["alpha"]) <= alpha_bound(ref), (where, rec["alpha"], ref["alpha"], alpha_bound(ref))
    assert rec["accepted"] == int(ref["selected"] != 0) and rec["nfevals"] >= rec["nleaves"]
    # the margins: a threshold is an exp of energy differences, each good to TOL_H max(|H|, 1); a cosine moves with the momenta, good to TOL_M
    assert ref["margin"] >= MARGIN * TOL_H * max(abs(ref["H0"]), 1.0), (where, ref["margin"], ref["H0"])
    assert ref["dot_margin"] >= MARGIN * TOL_M, (where, ref["dot_margin"])


@pytest.mark.parametrize("mass", ["diagonal", "lowrank"])
@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_replay_against_the_reference(name, mass):
    P = problem(name)
    seed, stream = REPLAY_SEEDS[(name, mass)]
    out = replay_chain(P, mass, seed, stream, NREPLAY, 4)
    print(f"\n[replay, {name}, {mass}] alpha differs by {max(abs(r['alpha'] - ref['alpha']) for r, _, ref in out):.2g}, bounds "
          f"{[float(f'{alpha_bound(ref):.2g}') for _, _, ref in out]}")
    print(f"[replay, {name}, {mass}] " + "; ".join(f"depth {r['depth']} leaves {r['nleaves']} stop {r['stop']} dirs {r['dirs']:b} sel {r['selected']} "
                                                    f"margin {ref['margin']:.2g} cos {ref['dot_margin']:.2g}" for r, _, ref in out))
    for t, (rec, m1, ref) in enumerate(out):
        check_replay(rec, m1, ref, (name, mass, t))
    assert any(r["selected"] != 0 for r, _, _ in out) and sum(r["nleaves"] for r, _, _ in out) >= 3 * NREPLAY
    assert len({r["dirs"] for r, _, _ in out}) > 1


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------------------
# what -> (seed, stream, max_depth, dt, samples, half width of the bounds around the start model or None): found by running the chain
# over seeds; each run is 12 samples or fewer on tiny.  Between the problem's own bounds no tree of 2500 turned inside a new subtree
# within depth 4; between bounds 0.05 around the start model the trajectories reflect, and every stop reason occurs
SHAPES = {"single leaf": (1, 0, 1, None, 4, None), "trees": (3, 0, 4, 0.008, 12, 0.05), "divergence": (1, 0, 4, 0.5, 3, None)}


def direction_changes(rec):
    """does the tree change direction forward-backward-forward (or the reverse) over its attempted doublings?"""
    n = rec["depth"] + (rec["stop"] in (1, 3))
    d = [(rec["dirs"] >> j) & 1 for j in range(n)]
    return any(d[j] != d[j + 1] and d[j + 1] != d[j + 2] for j in range(len(d) - 2))


def test_shapes_of_the_tree():
    P = problem("tiny")
    ctx = context(P)
    try:
        seed, stream, depth, dt, ns, _ = SHAPES["single leaf"]
        begin(ctx, P, seed, stream, dt=dt)
        recs, models, _ = ctx.chain_nuts_run(ns, depth)
        assert all(r["nleaves"] == 1 and r["depth"] <= 1 and abs(r["selected"]) <= 1 for r in recs)
        assert any(r["stop"] == 0 and r["depth"] == 1 for r in recs)
        seed, stream, depth, dt, ns, w = SHAPES["trees"]
        begin(ctx, P, seed, stream, dt=dt, lo=float(P.start[0]) - w, hi=float(P.start[0]) + w)
        recs, models, _ = ctx.chain_nuts_run(ns, depth)
        stops = [r["stop"] for r in recs]
        print(f"\n[shapes] stops {stops}, depths {[r['depth'] for r in recs]}, dirs {[bin(r['dirs']) for r in recs]}")
        assert {0, 1, 2} <= set(stops)
        assert any(direction_changes(r) for r in recs)                                   # (the gradient's hand-over, both ways)
        for r in recs:
            assert 1 <= r["nleaves"] <= 15 and r["depth"] <= 4 and (r["stop"] != 0 or (r["depth"] == 4 and r["nleaves"] == 15))
            assert r["stop"] not in (0, 2) or r["nleaves"] == 2 ** r["depth"] - 1
            assert -(2 ** r["depth"]) < r["selected"] < 2 ** r["depth"] and 0.0 <= r["alpha"] <= 1.0
        seed, stream, depth, dt, ns, _ = SHAPES["divergence"]
        begin(ctx, P, seed, stream, dt=dt)
        before = ctx.chain_state()[0]
        recs, models, _ = ctx.chain_nuts_run(ns, depth)
        for k, r in enumerate(recs):                        # the first leaf diverges: the model stays, the sample is committed as a repeat
            assert r["stop"] == 3 and r["nleaves"] == 1 and r["depth"] == 0 and r["selected"] == 0 and r["accepted"] == 0 and r["alpha"] == 0.0
            assert r["nsamples"] == k + 1 and r["hdif"] == 0.0 and bits(models[k]) == bits(before)
        assert ctx.chain_moments()[0] == ns and np.all(ctx.chain_moments()[2] == 0.0)
    finally:
        ctx.close()


# ---- 4. repeat and run -------------------------------------------------------------------------------------------------------------------
NRUN = 8


def nuts_run(P, how, mass="diagonal", adapt=None, accs=False, seed=5, stream=1, depth=3):
    ctx = context(P, mass)
    try:
        begin(ctx, P, seed, stream, burnin=0)
        if accs:
            begin_accumulators(ctx, P.n)
        if adapt is not None:
            ctx.chain_adapt_begin(**adapt)
        out = {"alpha_last": []}
        if how == "run":
            out["recs"], models, preds = ctx.chain_nuts_run(NRUN, depth)
            out["models"], out["preds"] = list(models), list(preds)
        else:
            out.update(recs=[], models=[], preds=[])
            for it in range(NRUN):
                rec, m, pred = ctx.chain_nuts_sample(depth)
                out["recs"].append(rec); out["models"].append(m); out["preds"].append(pred)
                if adapt is not None:
                    out["alpha_last"].append(ctx.chain_adapt_info()["alpha_last"])
        out["moments"] = ctx.chain_moments()
        out["rng"] = ctx.chain_rng_state()
        out["invM"] = ctx.chain_mass_diag() if mass == "diagonal" else None
        out["dt"] = ctx.chain_adapt_info()["dt"] if adapt is not None else None
        if accs:
            out["accs"] = read_accumulators(ctx)
        mx = Maxima()
        check_moments(mx, ctx, out["models"], NRUN)          # (tests/chain_ref.py's two-pass moments of the m_out sequence)
        return out
    finally:
        ctx.close()


def assert_same_run(a, b, accs=False):
    assert all_bits(a["recs"]) == all_bits(b["recs"])
    for key in ("models", "preds"):
        assert bits(np.array(a[key])) == bits(np.array(b[key])), key
    assert a["moments"][0] == b["moments"][0] and all(bits(x) == bits(y) for x, y in zip(a["moments"][1:], b["moments"][1:]))
    assert a["rng"] == b["rng"] and a["dt"] == b["dt"]
    if a["invM"] is not None:
        assert bits(a["invM"]) == bits(b["invM"])
    if accs:
        for key, got in a["accs"].items():
            assert all(bits(x) == bits(y) for x, y in zip(got, b["accs"][key])), key


@pytest.mark.parametrize("name,mass", [("tiny", "diagonal"), ("tiny", "lowrank"), ("ragged", "diagonal")])
def test_repeat_and_run_are_the_samples_bit_for_bit(name, mass):
    P = problem(name)
    single, again, whole = nuts_run(P, "samples", mass), nuts_run(P, "samples", mass), nuts_run(P, "run", mass)
    assert_same_run(single, again)
    assert_same_run(whole, single)
    recs = whole["recs"]
    assert whole["rng"] == (5, 1, NRUN) and [r["nsamples"] for r in recs] == list(range(1, NRUN + 1))
    assert [r["nfevals"] for r in recs] == [recs[0]["nleaves"] + 1] + [r["nleaves"] for r in recs[1:]]      # (one evaluation per leaf)
    assert any(r["selected"] != 0 for r in recs) and np.any(whole["moments"][2] > 0)


def test_run_with_accumulators_and_a_warm_up():
    """the histogram, acov, cov and data-moment accumulators and a warm-up of 7 steps with one mass window under 8 NUTS samples: the
    run equals the samples one by one, and the warm-up is fed the record's alpha"""
    P = problem("tiny")
    adapt = dict(nwarmup=7, **WINDOWS)
    single = nuts_run(P, "samples", adapt=adapt, accs=True)
    whole = nuts_run(P, "run", adapt=adapt, accs=True)
    assert_same_run(whole, single, accs=True)
    assert [bits(np.float64(a)) for a in single["alpha_last"][:7]] == [bits(np.float64(r["alpha"])) for r in single["recs"][:7]]
    assert single["dt"] != DT["tiny"] and bits(single["invM"]) != bits(P.invM)             # (the warm-up did adapt)
    plain = nuts_run(P, "samples")
    assert all_bits(plain["recs"])[0][0] == all_bits(single["recs"])[0][0] and all_bits(plain["recs"]) != all_bits(single["recs"])


# ---- 5. mixing with the fixed-length sample -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", ["diagonal", "lowrank"])
def test_a_fixed_length_sample_behind_a_nuts_sample(mass):
    """hmcmt_chain_sample behind two NUTS samples (it starts from the gradient the tree's selection left on the device) against the same
    draw on a fresh chain begun at that state with hmcmt_chain_set_energy (which evaluates its start gradient); and the reverse order"""
    P = problem("tiny")
    ctx, fresh = context(P, mass), context(P, mass)
    try:
        begin(ctx, P, 9, 2)
        recs = [ctx.chain_nuts_sample(3)[0] for _ in range(2)]
        assert any(r["selected"] != 0 for r in recs)
        m = ctx.chain_state()[0]
        rec, m1, pred1 = ctx.chain_sample(2, 3)
        assert rec["nfevals"] == L.rng_draw(9, 2, 2, 2, 3)[0]                             # (no evaluation of the start gradient)
        fresh.chain_begin(m, DT["tiny"], REG, LO, HI)
        fresh.chain_set_energy(recs[-1]["D"], recs[-1]["M"])
        fresh.chain_seed(9, 2)
        fresh.chain_rng_seek(2)
        ref, m2, pred2 = fresh.chain_sample(2, 3)
        assert ref["nfevals"] == rec["nfevals"] + 1 and ref["accepted"] == rec["accepted"]
        got, want = (np.array([r[k] for k in ("K0", "K1", "D1", "M1", "D", "M")]) for r in (rec, ref))
        assert rec["K0"] == ref["K0"] and hm_err(got, want) < TOL_H
        assert np.abs(m1 - m2).max() <= TOL_M * max(np.abs(m2).max(), 1.0)
        # ... and a NUTS sample behind the fixed-length one: the same on both chains
        a, ma, _ = ctx.chain_nuts_sample(3)
        b, mb, _ = fresh.chain_nuts_sample(3)
        assert a["nfevals"] == a["nleaves"] and tuple(a[k] for k in NUTS_KEYS) == tuple(b[k] for k in NUTS_KEYS)
        assert np.abs(ma - mb).max() <= TOL_M * max(np.abs(mb).max(), 1.0)
    finally:
        ctx.close()
        fresh.close()


# ---- 6. refusals and failures ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    P = problem("tiny")
    ctx = context(P)
    try:
        assert code_of(lambda: ctx.chain_nuts_sample(3)) == EINVAL                       # no chain
        ctx.chain_begin(P.start, DT["tiny"], REG, LO, HI)
        assert code_of(lambda: ctx.chain_nuts_sample(3)) == EINVAL                       # no seed
        assert code_of(lambda: ctx.chain_nuts_run(2, 3)) == EINVAL
        assert "hmcmt_chain_seed" in str(pytest.raises(L.HmcmtError, ctx.chain_nuts_sample, 3).value)
        ctx.chain_seed(3, 0)
        for depth in (0, -1, L.NUTS_DEPTH_MAX + 1):
            assert code_of(lambda: ctx.chain_nuts_sample(depth)) == EINVAL
            assert code_of(lambda: ctx.chain_nuts_run(2, depth)) == EINVAL
        assert code_of(lambda: ctx.chain_nuts_run(-1, 3)) == EINVAL
        assert ctx.lib.hmcmt_chain_nuts_sample(ctx.h, 3, None, None, None) == EINVAL     # NULL rec
        assert ctx.lib.hmcmt_chain_nuts_run(ctx.h, 2, 3, None, None, None, None) == EINVAL
        assert ctx.chain_rng_state() == (3, 0, 0)                                         # (a refused call draws nothing)
        assert ctx.chain_nuts_run(0, 3)[0] == [] and ctx.chain_rng_state() == (3, 0, 0)
        # between hmcmt_grad_device_async and hmcmt_wait
        dev = torch.device("cuda", 0)
        d_m = torch.from_numpy(P.start.copy()).to(dev)
        d_pred = torch.zeros(2 * ctx.nData, dtype=torch.float64, device=dev)
        d_g, d_s = torch.zeros(P.n, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert ctx.lib.hmcmt_grad_device_async(ctx.h, d_m.data_ptr(), d_pred.data_ptr(), d_s.data_ptr(), d_g.data_ptr()) == 0
        assert code_of(lambda: ctx.chain_nuts_sample(3)) == EINVAL
        ctx.wait()
        assert ctx.chain_rng_state() == (3, 0, 0)
        rec, _, _ = ctx.chain_nuts_sample(3)
        assert rec["nfevals"] == rec["nleaves"] + 1 and ctx.chain_rng_state() == (3, 0, 1)
    finally:
        ctx.close()
    wm = context(P, "wm")
    try:
        begin(wm, P, 3)
        assert code_of(lambda: wm.chain_nuts_sample(3)) == EINVAL                        # HMCMT_MASS_WM
        assert "HMCMT_MASS_WM" in str(pytest.raises(L.HmcmtError, wm.chain_nuts_sample, 3).value)
    finally:
        wm.close()


def test_a_failing_leaf_consumes_its_draw_and_leaves_the_chain():
    """the iteration-cap route of tests/test_gpu_chain.py: maxit = 2 is met by no solve on this mesh"""
    P = problem("tiny")
    ctx = context(P)
    try:
        begin(ctx, P, 4, 5, burnin=1)
        for _ in range(3):
            rec, _, _ = ctx.chain_nuts_sample(3)
        before = (ctx.chain_state()[0], ctx.chain_state()[2], ctx.chain_moments())
        maxit = ctx.opts.maxit
        ctx.set_options(maxit=2)
        assert code_of(lambda: ctx.chain_nuts_sample(3)) == ENOCONV
        assert ctx.chain_rng_state() == (4, 5, 4)                                         # t advanced by one
        recs, models, _, rc = ctx.chain_nuts_run(3, 3, check=False)
        assert rc == ENOCONV and recs == [] and len(models) == 0 and ctx.chain_rng_state() == (4, 5, 5)
        after = (ctx.chain_state()[0], ctx.chain_state()[2], ctx.chain_moments())
        assert bits(before[0]) == bits(after[0]) and bits(before[1]) == bits(after[1])
        assert before[2][0] == after[2][0] == 2 and all(bits(a) == bits(b) for a, b in zip(before[2][1:], after[2][1:]))
        ctx.set_options(maxit=maxit)
        rec2, _, _ = ctx.chain_nuts_sample(3)
        assert rec2["nsamples"] == rec["nsamples"] + 1 == 4 and ctx.chain_rng_state() == (4, 5, 6)
        assert rec2["nfevals"] == rec2["nleaves"] + 1                                     # (the start gradient is evaluated again)
    finally:
        ctx.close()


# ---- 7. the sampler --------------------------------------------------------------------------------------------------------------------------
def test_sampler_nuts_keyword():
    ns, burn = 8, 2
    hm, st, hd, moments, _ = run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 0), nuts={"max_depth": 3})
    hm2, st2, hd2, *_ = run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 0), nuts={"max_depth": 3}, verbose=True)
    assert bits(hm) == bits(hm2) and bits(hd) == bits(hd2)
    for f in ("nAccept", "nReject", "acceptstats", "hmstats", "moments", "rng"):
        assert same_bits(getattr(st, f), getattr(st2, f)), f
    nuts = st.nuts
    assert nuts["max_depth"] == 3 and all(len(nuts[k]) == ns for k in NUTS_KEYS + ("alpha",))
    assert all(np.array_equal(nuts[k], st2.nuts[k]) for k in NUTS_KEYS + ("alpha",))
    assert np.all((nuts["nleaves"] >= 1) & (nuts["nleaves"] <= 7) & (nuts["depth"] <= 3) & (nuts["alpha"] >= 0) & (nuts["alpha"] <= 1))
    assert np.array_equal(st.acceptstats, nuts["selected"] != 0) and st.nAccept == int((nuts["selected"] != 0).sum()) > 0
    assert st.rng == (7, 0, ns) and st.moments[0] == ns - burn and hm.shape[1] == ns
    assert np.all(np.isfinite(st.hmstats)) and np.array_equal(st.hmstats[3], st.hmstats[0] + st.hmstats[1] + st.hmstats[2])
    hm3, st3, *_ = run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 0))
    assert st3.nuts is None and not np.array_equal(hm3, hm)
    with pytest.raises(ValueError, match="nuts needs library_rng"):
        run("tiny", prior_of(ns, burn), device_chain=True, nuts={"max_depth": 3})
    with pytest.raises(ValueError, match="needs device_chain=True"):
        run("tiny", prior_of(ns, burn), library_rng=(7, 0), nuts={"max_depth": 3})
    for bad in ({"max_depth": 0}, {"max_depth": 11}, {"depth": 3}, 3):
        with pytest.raises(ValueError, match="nuts"):
            run("tiny", prior_of(ns, burn), device_chain=True, library_rng=(7, 0), nuts=bad)
    with pytest.raises(ValueError, match="nuts needs massType"):
        run("tiny", prior_of(ns, burn, "nondiagonal"), device_chain=True, library_rng=(7, 0), nuts={"max_depth": 3})
