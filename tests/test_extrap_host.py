"""The weights of the initial-guess extrapolation (hmcmt_items.h: extrap_weights) on the host, without a GPU: the item
source instantiated by tests/emul/emul_extrap.cpp against the independent long-double reference tests/extrap_ref.py -- known answers,
a few thousand random histories on both sides of every threshold, and the ring arithmetic of the two histories.

Bars: extrap_ref.Result.weight_bar (derived: the inner products are fp64 sums of n products, so alpha and every g_j carry a relative
error of about n 2^-53; the weights formed again with those moved by +-4 n 2^-53, times four, plus 8 x 2^-53 max|w|).  Decisions (repeat
flag, number of points, count, heads) must be equal exactly; a case whose reference reports a decision margin within 1e-9 of its
threshold is undecided and skipped, and the share of such cases must stay below 1 %."""
import numpy as np
import pytest

from tests import extrap_ref as R
from tests.emul import emul_extrap_py as E

N = 12                                  # parameters of the host models


def _frame(rng, n=N):
    """a base model around ln(0.01) and two orthogonal unit directions"""
    base = -4.5 + 0.3 * rng.standard_normal(n)
    u = rng.standard_normal(n); u /= np.linalg.norm(u)
    v = rng.standard_normal(n); v -= (v @ u) * u; v /= np.linalg.norm(v)
    return base, u, v


def _dyadic_path(steps, n=N):
    """models base + cumulative steps along a fixed direction, every number a small dyadic rational: the kernel's sums are exact"""
    base = -4.5 + np.arange(n) / 16.0
    d = (1 + np.arange(n) % 3) / 64.0
    out, t = [base.copy()], 0.0
    for s in steps:
        t += s
        out.append(base + t * d)
    return out


def _run(models, adjoint=False, cap=6):
    st = E.State(len(models[0]), adjoint, cap)
    return [st.call(m) for m in models]


def _agree(got, ref, label=""):
    """decisions exactly, weights within the reference's bar; returns the largest weight error in units of the bar"""
    assert (got["keep"], got["count"], got["head"], got["model_head"]) == (ref.keep, ref.count, ref.head, ref.model_head), (label, got, ref)
    assert got["npoints"] == ref.npoints, (label, got, ref)
    bar = ref.weight_bar()
    err = np.abs(got["weights"].astype(R.LD) - ref.weights).astype(float)
    assert (err <= bar).all(), (label, got["weights"], ref.weights, err, bar)
    return float((err / np.where(bar > 0, bar, 1.0)).max())


def test_constants_are_the_references():
    k = E.constants()
    assert k["points"] == R.POINTS and k["state_len"] == R.POINTS + 4 and k["nsums"] == 2 * R.POINTS


@pytest.mark.parametrize("nsteps,cap,expect", [
    (6, 6, (6, -15, 20, -15, 6, -1)), (5, 6, (5, -10, 10, -5, 1, 0)), (4, 6, (4, -6, 4, -1, 0, 0)), (3, 6, (3, -3, 1, 0, 0, 0)),
    (2, 6, (2, -1, 0, 0, 0, 0)), (6, 3, (3, -3, 1, 0, 0, 0)), (6, 2, (2, -1, 0, 0, 0, 0)), (6, 5, (5, -10, 10, -5, 1, 0))])
def test_uniform_collinear_steps_give_the_binomial_weights(nsteps, cap, expect):
    """nsteps equal steps on a line (the last one is the new step): the extrapolation of the polynomial through nsteps equidistant
    points, capped at `cap` points -- six: (6, -15, 20, -15, 6, -1), three: (3, -3, 1), two: the linear (2, -1)."""
    for adjoint in (False, True):
        out = _run(_dyadic_path([1.0] * nsteps), adjoint, cap)[-1]
        want = np.array(expect, float)
        if adjoint and min(nsteps, cap) < 3:
            want[:] = 0
        assert out["keep"] == 0 and out["count"] == min(nsteps + 1, 6)
        assert np.abs(out["weights"] - want).max() <= 1e-13 * max(np.abs(want).max(), 1), (out, want)


def test_short_histories_kinks_clamps_and_repeats():
    base, u, v = _frame(np.random.default_rng(1))
    h = 0.05
    # count 0 and 1: the zero fill, then the previous solution
    out = _run([base, base + h * u])
    assert [o["weights"].tolist() for o in out] == [[1, 0, 0, 0, 0, 0]] * 2 and [o["count"] for o in out] == [1, 2]
    assert [(o["head"], o["model_head"]) for o in out] == [(4, 6), (3, 5)]
    # ... and nothing at all for the adjoint solve, up to and including the linear guess
    out = _run([base, base + h * u, base + 2 * h * u], adjoint=True)
    assert all(not o["weights"].any() for o in out) and [o["count"] for o in out] == [1, 2, 3]
    # a kink after a straight stretch: the linear guess with the projection of the new step, whatever the history holds
    straight = [base + j * h * u for j in range(4)]
    alpha = 0.7 * 0.5                                                   # a step of 0.7 h at cos 0.5
    out = _run(straight + [straight[-1] + 0.7 * h * (0.5 * u + np.sqrt(0.75) * v)])[-1]
    assert np.abs(out["weights"] - [1 + alpha, -alpha, 0, 0, 0, 0]).max() < 1e-12 and out["npoints"] == 2
    # alpha is clamped to [-1, 2]
    back = _run(straight + [straight[-1] - 3 * h * u])[-1]
    assert np.abs(back["weights"] - [0, 1, 0, 0, 0, 0]).max() == 0
    far = _run(straight + [straight[-1] + 5 * h * u])[-1]
    assert np.abs(far["weights"] - [3, -2, 0, 0, 0, 0]).max() == 0
    # a repeat keeps everything: weight 1 on the previous solution for both kinds, count and heads as they were
    for adjoint in (False, True):
        st = E.State(N, adjoint)
        for m in straight:
            before = st.call(m)
        hist = st.hist.copy()
        again = st.call(straight[-1].copy())
        assert again["keep"] == 1 and again["weights"].tolist() == [1, 0, 0, 0, 0, 0]
        assert (again["count"], again["head"], again["model_head"]) == (before["count"], before["head"], before["model_head"])
        live = [(again["model_head"] + j) % 7 for j in range(again["count"])]
        assert np.array_equal(st.hist[live], hist[live])                # (the spare slot in front of the head took the repeat)
        nxt = st.call(straight[-1] + h * u)                             # ... and the next new model extrapolates at full order
        assert np.abs(nxt["weights"] - [4, -6, 4, -1, 0, 0]).max() < 1e-9 and nxt["keep"] == 0


def _random_history(rng):
    """seven models: step 1 (the one every later call measures against is always the previous one, so every step takes that role in
    turn) of length h, the others of length ratio 0.3..3 and cosine 0.8..1 against a common direction"""
    base, u, _ = _frame(rng)
    h = 0.05
    models = [base]
    for j in range(6):
        w = rng.standard_normal(N); w -= (w @ u) * u; w /= np.linalg.norm(w)
        c = rng.uniform(0.8, 1.0)
        ratio = np.exp(rng.uniform(np.log(0.3), np.log(3.0)))
        # (half of the steps stay close to the line and to the common length, so that long point lists occur often enough)
        if rng.random() < 0.7:
            c, ratio = rng.uniform(0.97, 1.0), rng.uniform(0.7, 1.5)
        models.append(models[-1] + h * ratio * (c * u + np.sqrt(1 - c * c) * w))
    return models


def test_random_histories_agree_with_the_reference():
    """count 0..6, length ratios over (0.3, 3), cosines over (0.8, 1), both kinds, every cap 2..6: keep, points, count, heads exactly,
    weights within the bar.  Undecided cases (a margin within 1e-9 of its threshold) are skipped; they must be rare."""
    rng = np.random.default_rng(2024)
    cases = undecided = 0
    worst, points_seen = 0.0, set()
    for adjoint in (False, True):
        for cap in range(2, 7):
            for trial in range(60):
                models = _random_history(rng)
                st, ref = E.State(N, adjoint, cap), R.KindHistory(adjoint, cap)
                for k, m in enumerate(models):
                    got, want = st.call(m), ref.call(m)
                    assert want.count == min(k + 1, 6)
                    cases += 1
                    if not want.decided(1e-9):
                        undecided += 1
                        break                                           # (the two histories may have parted: this one ends here)
                    worst = max(worst, _agree(got, want, (adjoint, cap, trial, k)))
                    points_seen.add((adjoint, want.npoints))
    print(f"[host] {cases} calls, {undecided} undecided, worst weight error {worst:.3f} of its bar")
    assert cases >= 3000 and undecided <= 0.01 * cases
    assert {p for a, p in points_seen if not a} == {1, 2, 3, 4, 5, 6} and {p for a, p in points_seen if a} == {0, 3, 4, 5, 6}


def test_the_generator_alone_keeps_its_margins_away_from_the_thresholds():
    """the same generator through the reference only: the share of undecided calls is far below the 1 % the test above allows"""
    rng = np.random.default_rng(7)
    calls = near = 0
    for trial in range(300):
        ref = R.KindHistory(False, 6)
        for m in _random_history(rng):
            r = ref.call(m)
            calls += 1
            near += not r.decided(1e-9)
    assert near <= 0.001 * calls, (near, calls)


def test_ring_heads_follow_the_plain_list_over_many_calls_and_repeats():
    """20 new models with repeats in between (and two in a row), a reset in the middle: count, both heads and the models the ring
    holds -- slot (head + j) mod 7 = the model j calls back -- against the reference's list."""
    rng = np.random.default_rng(3)
    base, u, v = _frame(rng)
    for adjoint in (False, True):
        st, ref = E.State(N, adjoint), R.KindHistory(adjoint)
        m, new = base.copy(), 0
        heads = set()
        for k in range(20):
            m = m + 0.05 * rng.uniform(0.8, 1.2) * (u + 0.05 * rng.standard_normal(N))
            for rep in range(1 + (k % 4 == 2) + (k == 10)):              # a repeat after every fourth model, two after the eleventh
                got, want = st.call(m.copy()), ref.call(m)
                assert want.decided(1e-9)
                _agree(got, want, (adjoint, k, rep))
                assert want.keep == int(rep > 0)
                for j in range(want.count):
                    assert np.array_equal(st.hist[(got["model_head"] + j) % 7], ref.models[j].astype(float)), (k, rep, j)
            heads.add((got["head"], got["model_head"]))
            if k == 12:
                st.reset(); ref.reset()
        assert len({h for h, _ in heads}) == 5 and len({mh for _, mh in heads}) == 7     # (both rings went all the way round)
