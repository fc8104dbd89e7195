"""The leapfrog's position and momentum updates where they clamp and reflect, under every mass, against tests/leapfrog_ref.py:
lf_step_dm / lf_step_bound, k_lf_momentum_max, k_lf_step and the fused forms in k_sigma_rows and k_gradfinal (diagonal mass),
mass_x_bound -> k_mass_bound -> k_mass_step (M = Wm separable and by PCG, the low-rank mass), through hmcmt_leapfrog,
hmcmt_leapfrog_device and hmcmt_chain_step.

Every context is created with warm_start="cold" and HMCMT_SWEEPS=1: an evaluation depends on its model only.  The reference's data gradient is `grad` of
a sibling cold context at the models the device itself returned (a replay: leapfrog_ref.trajectory(models=...)); the predicted data of
the trajectory must equal the sibling's at the end model bit for bit, so the end gradient is the same evaluation and the momentum is
held in units of eps.  The momentum behind the half step is planted exactly, p0 = M x_target + (dt/2) g_total(m0), with ONE maximum
of |x_target| at least twice every other, so the test decides where the maximum sits and what the step bound is.

Asserted without a tolerance of their own: which elements were reflected and how often modulo two, the momentum of the others
untouched by the position update, one clamp factor for all elements, every model value within the bounds, nfevals = L + 1; and every
case fails if what it is about -- the planted maximum, the clamp, the reflections -- did not occur in the reference."""
import numpy as np
import pytest

from hmcmt2d_amd.lib import HipContext, HMCMT_MASS_WM
from tests import leapfrog_ref as R
from tests import mass_lowrank_ref
from tests.helpers import make_problem, ragged_problem

pytestmark = pytest.mark.gpu

LD = R.LD
LO, HI = float(np.log(1e-4)), 0.0
REG = 1.0
RHO = 100.0                                    # the homogeneous start: ln sigma = -4.6, more than 3 from either bound
WM_SOLVE = 1e-10                               # the bar of test_mass_apply_against_scipy on Wm^-1 x
FORCE = 1e12
MASSES = ["diagonal", "wm", "lowrank5"]


class Maxima:
    """the largest value seen of each checked quantity, in units of its bound (as in tests/test_gpu_chain_kernels.py)"""

    def __init__(self):
        self.v = {}

    def check(self, key, err, bound, what=""):
        err, bound = np.asarray(err, dtype=float), np.asarray(bound, dtype=float)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
        self.v[key] = max(self.v.get(key, 0.0), ratio)
        assert np.all(err <= bound), f"{key} {what}: {ratio:.3g} of its bound (element {int(np.argmax(err / np.maximum(bound, 1e-300)))})"

    def __str__(self):
        return ", ".join(f"{k} {v:.2g}" for k, v in self.v.items())


class Problem:
    def __init__(self, name):
        self.name = name
        self.mesh, self.data, self.inv, _ = ragged_problem(23, 17, 3, 3, 3, 4) if name == "ragged" else make_problem(name)
        inv = self.inv
        self.n = n = len(inv.strModel)
        self.Wm = inv.Wm
        ny, nz = self.mesh.gridSize
        ky, kz = inv.activeIdx % ny, inv.activeIdx // ny
        smooth = 0.2 * np.sin(2 * np.pi * ky / ny) * np.cos(np.pi * kz / nz) + 0.1 * kz / nz
        self.start = np.log(1.0 / RHO) + 0.05 * np.cos(np.arange(n) / 5.0)
        self.mref = np.log(1.0 / RHO) - smooth
        self.invM = np.random.default_rng(n).uniform(0.25, 4.0, n)
        self.dt = 0.02
        self.rows = R.Rows(self.Wm)

    def context(self):
        """cold starts and ONE smoother sweep whatever the last solve took (the default chooses per solve from the context's history,
        tests/test_gpu_parity.py): an evaluation then depends on its model only, bit for bit"""
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("HMCMT_SWEEPS", "1")                     # (read once, at hmcmt_create)
            return HipContext(self.mesh, self.data, self.inv, device_id=0, warm_start="cold")


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]


class Pair:
    """the context under test and its sibling, both cold; the sibling only ever evaluates `grad`"""

    def __init__(self, P):
        self.P = P
        self.ctx = P.context()
        try:
            self.sib = P.context()
        except Exception:
            self.ctx.close()
            raise

    def close(self):
        self.ctx.close()
        self.sib.close()

    def set_mass(self, kind, invM=None):
        """sets the prior and the mass on the context under test; returns (the reference's operator, the bar on the solver for x)"""
        P = self.P
        invM = P.invM if invM is None else invM
        self.ctx.set_prior(P.mref, P.Wm, invM)
        if kind == "diagonal":
            return R.DiagonalMass(invM), 0.0
        if kind == "wm":
            self.ctx.set_mass(HMCMT_MASS_WM)
            return R.WmMass(P.Wm), WM_SOLVE
        rank = int(kind[len("lowrank"):])
        s, U, lam, _ = mass_lowrank_ref.problem(P.n, rank)
        self.ctx.set_mass_lowrank(s, U, lam)
        return R.LowRankMass(s, U, lam), 0.0

    def gtot(self, m):
        """the sibling's total gradient at m, long double: (pred, data gradient, g + lam Wm (m - mref))"""
        pred, _, g = self.sib.grad(m)
        return pred, g, R._ld(g) + LD(REG) * self.P.rows.mul(R._ld(m) - R._ld(self.P.mref))


def velocity(n, seed, dt, mx, where, others):
    """x_target: dt |x| = mx at `where`, at most others * mx elsewhere (others <= 0.5: the planted maximum is twice every other)"""
    assert others <= 0.5
    v = others * mx * np.random.default_rng(seed).uniform(-1, 1, n)
    v[where] = mx
    return v / dt


def plant(pair, mass, m0, x_target, dt):
    """p0 = M x_target + (dt/2) g_total(m0): behind the half step the momentum is M x_target"""
    _, g0, gt0 = pair.gtot(m0)
    return np.asarray(mass.mul(R._ld(x_target)) + LD(0.5) * LD(dt) * gt0, dtype=np.float64), g0


def verify(mx, pair, mass, solve_rel, m0, p0, g0, dt, L, lo, hi, run, label):
    """Runs `run(l)` -> (model, momentum, pred, nfevals) for l = 1 .. L from (m0, p0), replays the reference from the models it returned
    with the sibling's gradients, and holds the last step to it.  Returns the reference's trajectory."""
    outs = [run(l) for l in range(1, L + 1)]
    models = [o[0] for o in outs]
    m_dev, p_dev, pred_dev, nf = outs[-1]
    assert nf == L + 1, (label, nf)
    for m in models:
        assert m.min() >= lo and m.max() <= hi, label
    sib = [pair.gtot(m) for m in models]
    # the precondition: the end model's evaluation on the sibling is the trajectory's own, bit for bit
    assert np.array_equal(pred_dev, sib[-1][0]), f"{label}: the trajectory's pred differs from the sibling's at the end model"
    grads = [g0] + [s[1] for s in sib]
    ref = R.trajectory(m0, p0, dt, L, REG, pair.P.mref, pair.P.Wm, lo, hi, mass, lambda k, m: grads[k], models=models)
    bm, bp = R.bars(ref, mass, solve_rel=solve_rel)
    for k, s in enumerate(ref["steps"]):
        # (the reference's own decisions are not within rounding of going the other way)
        assert abs(s["mx"] - R.MAX_STEP) > 1e-6 and np.all(s["margin"] > 8 * bm[k]), label
        mx.check("m", np.abs(models[k] - np.asarray(s["m"], dtype=float)), bm[k], f"{label}, step {k + 1}")
    mx.check("p", np.abs(p_dev - ref["p"]), bp[-1], label)
    # -- structure, from the last step --
    s, b_m, b_p = ref["steps"][-1], bm[-1], bp[-1]
    start = np.asarray(s["start"], dtype=float)
    landing = start + np.asarray(s["dm"], dtype=float)                          # where the step ends without a reflection
    reflected = s["count"] > 0
    assert np.array_equal(np.abs(m_dev - landing) > 4 * b_m, reflected), f"{label}: the set of reflected elements"
    # the momentum behind the position update, from the end momentum and the end model's own gradient
    p_pos = np.asarray(R._ld(p_dev) + LD(s["c"]) * LD(dt) * sib[-1][2], dtype=float)
    want = np.asarray(s["p_position"], dtype=float)
    before = np.asarray(s["p_before"], dtype=float)
    assert np.all(np.abs(want[reflected]) > 4 * b_p[reflected]), f"{label}: a reflected element's momentum is too small to show its sign"
    clear = np.abs(want) > 4 * b_p
    assert np.array_equal(np.sign(p_pos[clear]), (np.sign(before) * (-1.0) ** s["count"])[clear]), f"{label}: flip parity"
    mx.check("p unreflected", np.abs(p_pos - before)[~reflected], b_p[~reflected], label)
    # one clamp factor for all: the unreflected elements' steps over dt x
    dtx = np.asarray(LD(dt) * s["x"], dtype=float)
    sel = ~reflected & (np.abs(dtx) > 1e-3 * s["mx"])
    assert sel.sum() >= 2 or pair.P.n - reflected.sum() < 2, label
    mx.check("factor", np.abs((m_dev - start)[sel] / dtx[sel] - s["factor"]), (b_m / np.abs(dtx))[sel], label)
    ref["device"] = dict(m=m_dev, p=p_dev, p_position=p_pos)
    return ref


def host_run(pair, m0, p0, dt, lo, hi):
    """hmcmt_leapfrog, and hmcmt_leapfrog_device from the same start with the same bits"""
    import torch

    def run(l):
        m1, p1, pred, _, _, nf = pair.ctx.leapfrog(m0, p0, dt, l, REG, lo, hi)
        dm, dp = torch.from_numpy(m0.copy()).cuda(), torch.from_numpy(p0.copy()).cuda()
        dpred = torch.zeros(pair.ctx.nData, dtype=torch.complex128, device=dm.device)
        torch.cuda.synchronize()
        nfd = pair.ctx.leapfrog_device(dm.data_ptr(), dp.data_ptr(), dt, l, REG, lo, hi, d_pred=dpred.data_ptr())
        pair.ctx.wait()
        assert nfd == nf
        assert np.array_equal(dm.cpu().numpy(), m1) and np.array_equal(dp.cpu().numpy(), p1), "hmcmt_leapfrog_device: other bits"
        assert np.array_equal(dpred.cpu().numpy(), np.asarray(pred, dtype=np.complex128))
        return m1, p1, pred, nf
    return run


def planted_case(mx, pair, kind, m0, dtx, dt, L, lo=LO, hi=HI, label=""):
    """a trajectory whose half-step momentum is M (dtx / dt)"""
    mass, solve_rel = pair.set_mass(kind)
    p0, g0 = plant(pair, mass, m0, dtx / dt, dt)
    return verify(mx, pair, mass, solve_rel, m0, p0, g0, dt, L, lo, hi, host_run(pair, m0, p0, dt, lo, hi), label)


def report(label, P, mx, ref):
    print(f"\n[{label}, {P.name}] nAC {P.n}; mx {[round(s['mx'], 4) for s in ref['steps']]}, at {[s['imax'] for s in ref['steps']]}, "
          f"reflections {[int(s['count'].sum()) for s in ref['steps']]} (most {max(int(s['count'].max()) for s in ref['steps'])}); "
          f"largest error over its bound: {mx}")


def with_pair(name, body):
    P = problem(name)
    pair = Pair(P)
    try:
        body(P, pair)
    finally:
        pair.close()


CASES = [("tiny", k) for k in MASSES + ["lowrank32"]] + [("ragged", k) for k in MASSES]


# ---- A: no clamp.  B: the clamp, the maximum at index 0 and at the last element --------------------------------------------------------
@pytest.mark.parametrize("name,kind", CASES)
def test_no_clamp_just_below_three(name, kind):
    def body(P, pair):
        mx = Maxima()
        if kind == "wm":
            assert pair.set_mass(kind) and pair.ctx.mass_info()["separable"] == (name == "tiny")
        ref = planted_case(mx, pair, kind, P.start, velocity(P.n, 1, 1.0, 2.999, P.n // 3, 0.4), P.dt, 1, label="A")
        s = ref["steps"][0]
        assert not s["clamped"] and s["imax"] == P.n // 3 and abs(s["mx"] - 2.999) < 1e-6 and s["count"].sum() == 0
        report(f"A, {kind}", P, mx, ref)
    with_pair(name, body)


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("name,kind", CASES)
def test_clamp_with_the_maximum_at(name, kind, where):
    def body(P, pair):
        mx = Maxima()
        at = 0 if where == "first" else P.n - 1
        ref = planted_case(mx, pair, kind, P.start, velocity(P.n, 2, 1.0, -6.0 if where == "last" else 6.0, at, 0.4), P.dt, 1, label="B")
        s = ref["steps"][0]
        assert s["clamped"] and s["imax"] == at and abs(s["mx"] - 6.0) < 1e-6 and s["count"].sum() == 0
        assert abs(s["factor"] - 0.5) < 1e-6
        report(f"B, maximum at the {where} element, {kind}", P, mx, ref)
    with_pair(name, body)


# ---- C: reflection (tiny) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MASSES + ["lowrank32"])
def test_reflection_at_both_bounds_and_a_landing_on_one(kind):
    """the start within 0.01 of hi in one half and of lo in the other; the clamped step's maximum moves by 3 exactly (dm / mx = 1), from
    hi - 3 onto hi: no reflection there, and the momentum keeps its sign"""
    def body(P, pair):
        mx = Maxima()
        n, j = P.n, 3
        near = 0.01 * np.random.default_rng(3).random(n)
        m0 = np.where(np.arange(n) < n // 2, HI - near, LO + near)
        m0[j] = HI - 3.0
        assert m0[j] + 3.0 == HI
        ref = planted_case(mx, pair, kind, m0, velocity(n, 4, 1.0, 6.0, j, 0.4), P.dt, 1, label="C")
        s = ref["steps"][0]
        assert s["clamped"] and s["imax"] == j and s["count"][j] == 0 and float(s["m"][j]) == HI
        assert s["count"][:n // 2].sum() >= 2 and s["count"][n // 2:].sum() >= 2
        dev = ref["device"]
        assert dev["m"][j] == HI and np.sign(dev["p_position"][j]) == np.sign(float(s["p_before"][j]))
        report(f"C, both bounds, {kind}", P, mx, ref)
    with_pair("tiny", body)


@pytest.mark.parametrize("kind", MASSES + ["lowrank32"])
def test_reflection_between_bounds_0p7_apart(kind):
    """a clamped step of 3 between bounds 0.7 apart reflects four times and more; odd and even counts side by side"""
    def body(P, pair):
        mx = Maxima()
        lo, hi = -5.2, -4.5
        m0 = np.random.default_rng(5).uniform(lo + 0.05, hi - 0.05, P.n)
        ref = planted_case(mx, pair, kind, m0, velocity(P.n, 6, 1.0, 6.0, 0, 0.5), P.dt, 1, lo=lo, hi=hi, label="C 0.7")
        s = ref["steps"][0]
        assert s["clamped"] and s["imax"] == 0 and s["count"][0] >= 4
        assert (s["count"] % 2 == 0).any() and (s["count"] % 2 == 1).any() and len(set(s["count"])) >= 3
        report(f"C, bounds 0.7 apart, {kind}", P, mx, ref)
    with_pair("tiny", body)


# ---- D: two steps (tiny) -------------------------------------------------------------------------------------------------------------
def gradient_step(pair, mass, m0, target):
    """dt with dt^2 max|M^-1 g_total(m0)| = target: the inner momentum update then moves the second step's bound by that much"""
    gt0 = pair.gtot(m0)[2]
    return float(np.sqrt(target / float(np.abs(mass.inv(gt0)).max())))


@pytest.mark.parametrize("kind", MASSES + ["lowrank32"])
def test_two_steps_unclamped_then_clamped(kind):
    def body(P, pair):
        mx = Maxima()
        mass, _ = pair.set_mass(kind)
        dt = gradient_step(pair, mass, P.start, 5.0)
        ref = planted_case(mx, pair, kind, P.start, velocity(P.n, 7, 1.0, 0.05, 0, 0.4), dt, 2, label="D1")
        s1, s2 = ref["steps"]
        assert not s1["clamped"] and abs(s1["mx"] - 0.05) < 1e-6 and s2["clamped"] and s2["mx"] > 4.0
        report(f"D, unclamped then clamped, dt {dt:.3g}, {kind}", P, mx, ref)
    with_pair("tiny", body)


@pytest.mark.parametrize("kind", MASSES + ["lowrank32"])
def test_two_steps_clamped_twice(kind):
    """mx = 6 in the first step and another bound, off by more than 10 %, in the second: a bound that is not formed again shows at
    order one"""
    def body(P, pair):
        mx = Maxima()
        mass, _ = pair.set_mass(kind)
        dt = gradient_step(pair, mass, P.start, 20.0)
        ref = planted_case(mx, pair, kind, P.start, velocity(P.n, 8, 1.0, 6.0, 0, 0.4), dt, 2, label="D2")
        s1, s2 = ref["steps"]
        assert s1["clamped"] and abs(s1["mx"] - 6.0) < 1e-6 and s2["clamped"]
        assert abs(s2["mx"] - 6.0) > 0.6
        report(f"D, clamped twice, dt {dt:.3g}, {kind}", P, mx, ref)
    with_pair("tiny", body)


def second_step_planted(mx, pair, first_mx, second, candidates, label):
    """Diagonal mass, two steps, the SECOND step's bound planted -- it comes from k_gradfinal's partial maxima, which nothing but the
    inner momentum update forms: dm2 = dt x1 - dt^2 invM g_total(m1), and invM is the test's to choose.  Every element's gradient term
    is at most 0.3 but the one of element t (a candidate with a large gradient), whose invM makes its second step +-`second`.
    (first_mx > second needs x1[t] and g_total(m1)[t] of one sign, and m1 depends on that sign: candidates are tried until one fits.)"""
    P = pair.P
    n, dt = P.n, P.dt
    f = min(1.0, 3.0 / first_mx)
    at_start = np.abs(np.asarray(pair.gtot(P.start)[2], dtype=float))
    for t, sign in [(int(t), sign) for t in candidates[np.argsort(-at_start[candidates])][:4] for sign in (1.0, -1.0)]:
        dtx = 0.4 * first_mx * np.random.default_rng(9).uniform(-1, 1, n)
        dtx[t] = sign * first_mx
        m1 = P.start + f * dtx                                             # (more than 3 from either bound: no reflection)
        g1 = np.asarray(pair.gtot(m1)[2], dtype=float)
        if first_mx < second or np.sign(g1[t]) == sign:
            break
    else:
        pytest.fail(f"{label}: no candidate whose gradient has the sign of its step")
    assert abs(g1[t]) > 1e-3 * np.abs(g1).max()
    invM = 0.3 / (dt * dt * np.abs(g1).max()) * np.random.default_rng(10).uniform(0.25, 1.0, n)
    end = second * (sign if first_mx > second else -np.sign(g1[t]))        # dm2[t] wanted: dtx[t] - end has the sign of g1[t]
    invM[t] = abs(dtx[t] - end) / (dt * dt * abs(g1[t]))
    mass, solve_rel = pair.set_mass("diagonal", invM=invM)
    p0, g0 = plant(pair, mass, P.start, dtx / dt, dt)
    ref = verify(mx, pair, mass, solve_rel, P.start, p0, g0, dt, 2, LO, HI, host_run(pair, P.start, p0, dt, LO, HI), label)
    return ref, t


def test_two_steps_clamped_then_a_smaller_bound():
    """diagonal mass: mx = 6, then a step below 3 -- k_gradfinal collects its maxima with atomicMax into slots that k_bcsens_contract
    must have zeroed: a maximum left over from the first step would clamp the second"""
    def body(P, pair):
        mx = Maxima()
        ref, t = second_step_planted(mx, pair, 6.0, 2.0, np.arange(P.n), "D3")
        s1, s2 = ref["steps"]
        assert s1["clamped"] and s1["imax"] == t and abs(s1["mx"] - 6.0) < 1e-6
        assert not s2["clamped"] and 1.5 < s2["mx"] < 2.9
        report("D, clamped then a smaller bound, diagonal", P, mx, ref)
    with_pair("tiny", body)


# ---- E: the chain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["wm", "lowrank5"])
def test_chain_step_that_clamps_and_reflects(kind):
    """hmcmt_chain_step under the non-diagonal masses from a start within 0.01 of the bounds, dt such that dt max|M^-1 p| = 6 for the
    chain's own momentum (chain_state); the reference must report a clamped step and reflections"""
    def body(P, pair):
        mx = Maxima()
        n, ctx = P.n, pair.ctx
        rng = np.random.default_rng(61)
        near = 0.01 * rng.random(n)
        m0 = np.where(np.arange(n) < n // 2, HI - near, LO + near)
        mass, solve_rel = pair.set_mass(kind)
        D0, M0 = ctx.chain_begin(m0, P.dt, REG, LO, HI)
        ctx.chain_momentum(np.clip(1.5 * rng.standard_normal(n), -2.5, 2.5))
        p0 = ctx.chain_state()[1]
        dt = 6.0 / float(np.abs(mass.inv(R._ld(p0))).max())
        ctx.chain_set_dt(dt)
        ctx.chain_set_energy(D0 + FORCE, M0)
        g0 = pair.sib.grad(m0)[2]

        def run(l):
            rec, m_out, pred_out = ctx.chain_step(l, 0.5)
            assert rec["accepted"] == 1
            return m_out, ctx.chain_state()[1], pred_out, rec["nfevals"]

        ref = verify(mx, pair, mass, solve_rel, m0, p0, g0, dt, 1, LO, HI, run, "E")
        s = ref["steps"][0]
        assert s["clamped"] and s["count"].sum() >= 1
        report(f"E, chain step, dt {dt:.3g}, {kind}", P, mx, ref)
    with_pair("tiny", body)


# ---- the larger problems, each on one pair of contexts (last in the module: no other context of these tests lives beside them) ----------
@pytest.fixture(scope="module")
def cfg1_pair():
    pair = Pair(problem("cfg1"))
    yield pair
    pair.close()


def test_second_bound_from_the_last_workgroup_of_gradfinal(cfg1_pair):
    """cfg1, 4704 parameters, diagonal mass: k_gradfinal runs 294 workgroups of 16 parameters and folds their maxima into 64 slots
    (blockIdx.x & 63); the second step's maximum sits in the last workgroup, 293, slot 37, and clamps"""
    P = cfg1_pair.P
    assert P.n == 4704 and (P.n - 1) // 16 == 293
    mx = Maxima()
    ref, t = second_step_planted(mx, cfg1_pair, 0.01, 6.0, np.arange(P.n - 16, P.n), "B3")
    s1, s2 = ref["steps"]
    assert not s1["clamped"] and s2["clamped"] and s2["imax"] == t and t // 16 == 293 and 5.9 < s2["mx"] < 6.1
    report("B, the second step's maximum in k_gradfinal's last workgroup, diagonal", P, mx, ref)


@pytest.fixture(scope="module")
def cfg3_pair():
    pair = Pair(problem("cfg3"))
    yield pair
    pair.close()


@pytest.mark.parametrize("kind", MASSES)
def test_clamp_with_the_maximum_past_16384(cfg3_pair, kind):
    """cfg3, 20000 parameters: the step bound's second grid-stride pass (k_lf_momentum_max, k_mass_bound: 64 workgroups of 256)"""
    P = cfg3_pair.P
    at = 16384 + 1000
    assert P.n == 20000 and at >= 64 * 256
    mx = Maxima()
    ref = planted_case(mx, cfg3_pair, kind, P.start, velocity(P.n, 11, 1.0, 6.0, at, 0.02), P.dt, 1, label="B4")
    s = ref["steps"][0]
    assert s["clamped"] and s["imax"] == at and abs(s["mx"] - 6.0) < 1e-6
    report(f"B, maximum at {at}, {kind}", P, mx, ref)
