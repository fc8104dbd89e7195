"""The initial-guess extrapolation (k_extrap_prepare, extrap_weights, k_extrap) on the device against the independent
long-double reference tests/extrap_ref.py.  Every case drives a context with warm_start = "extrapolate" along a constructed model path
with the guess capture on and, after every evaluation, reads the extrapolation state (hmcmt_debug_extrap), the captured guesses
(hmcmt_debug_guess) and the converged fields (hmcmt_get_fields: the stored doubles, so the test knows the ring's contents exactly):

  (a) repeat flag, count, both ring heads, number of points: equal to the reference's on the actual model history; weights within
      Result.weight_bar -- the partial sums, their ticketed reduction and the weights;
  (b) the captured guess on interior nodes = sum_j w_ref,j x_{k-j} of the fields the test fetched after the earlier evaluations,
      within extrap_ref.guess_bar -- the ring slots of k_extrap, the store of the outgoing solution, the interior mask; pad nodes
      (and, for the adjoint, boundary nodes) untouched.  A repeat's guess is the previous solution bit for bit.

Bars (derived, extrap_ref.py): weights 4 x (change under alpha, g_j -> (1 +- 4 nAC 2^-53)) + 8 x 2^-53 max|w|; guess
sum_j (dw_j + 8 x 2^-53 |w_j|) |x_{k-j}|.  Decisions must be equal exactly, and every path keeps the reference's margins away from
the thresholds (asserted: cosines by 0.02, length ratios by 0.05), so a failure is never a rounding tie.

Sizes: tiny (96 active cells: one block of the partial-sum pass, a partial wave), cfg2 (1250: five blocks, a ragged last one), a
120 x 72 mesh (8640: a second grid-stride pass of the 32 x 256 threads and a ragged tail).
Measured on an MI355X, largest weight error absolute and in units of its bar | largest guess error relative to max|x_k|
and in units of its bar: tiny 2.9e-14, 1.9e-3 | 9.5e-15, 2.1e-2; cfg2 1.5e-14, 1.3e-4 | 1.3e-14, 2.2e-2; 120 x 72 1.7e-14, 1.2e-5 |
2.2e-14, 1.4e-5.  The bars grow with nAC (they bound the worst case of an nAC-term sum), the errors do not.
The file takes about a second on the GPU (the first device-pointer case also pays torch's start-up when nothing before it has)."""
import numpy as np
import pytest

from hmcmt2d_amd import synthetic as S, invsetup as I
from hmcmt2d_amd.lib import HipContext, HmcmtError
from tests import extrap_ref as R
from tests.helpers import make_problem, start_sigma

pytestmark = pytest.mark.gpu

_ENV = ("HMCMT_EXTRAP_POINTS", "HMCMT_SWEEPS", "HMCMT_PERSIST", "HMCMT_SIDE_IT")
_problems = {}


def _problem(name):
    """(mesh, data, inv, m): tiny, cfg2, or the 120 x 72 mesh with two frequencies and five receivers"""
    if name not in _problems:
        if name == "wide":
            mesh = S.make_mesh(120, 72)
            data = S.make_data_layout([10.0, 0.3], [-2100.0, -700.0, 300.0, 1500.0, 2600.0])
            n = len(data.rxID)
            obs = np.full(n, 0.02 + 0.02j) * np.where(data.dtID == 1, 1.0, -1.0)
            mesh.sigma = start_sigma(mesh)
            inv = I.setupInverseDataModel(mesh, [S.SIG_AIR], 0.0, 0.0, obs, np.full(n, 1e-3))
            _problems[name] = (mesh, data, inv, S.rough_state(len(inv.strModel)))
        else:
            _problems[name] = make_problem(name)
    return _problems[name]


NAC = {"tiny": 96, "cfg2": 1250, "wide": 8640}


def _frame(n, seed=17):
    """two orthogonal directions of length sqrt(n): a step h u moves every parameter by about h"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(n); u *= np.sqrt(n) / np.linalg.norm(u)
    v = rng.standard_normal(n); v -= (v @ u) / (u @ u) * u; v *= np.sqrt(n) / np.linalg.norm(v)
    return u, v


def _models(m0, steps):
    out = [np.array(m0, dtype=np.float64)]
    for s in steps:
        out.append(out[-1] + s)
    return out


class Drive:
    """A context, the reference beside it, and the fields fetched so far (per kind, newest first, padded layout)."""

    def __init__(self, monkeypatch, name, cap=None, capture=True):
        for k in _ENV:
            monkeypatch.delenv(k, raising=False)
        if cap is not None:
            monkeypatch.setenv("HMCMT_EXTRAP_POINTS", str(cap))
        self.mesh, self.data, self.inv, self.m0 = _problem(name)
        self.ctx = HipContext(self.mesh, self.data, self.inv, warm_start="extrapolate")
        assert self.ctx.nAC == NAC[name]
        self.ref = R.ExtrapRef(cap or R.POINTS)
        self.fields = {0: [], 1: []}
        self.worst_w = self.worst_g = 0.0
        self.seen = {0: [], 1: []}                  # number of points of every call, per kind
        self.dev = None
        if capture:
            self.ctx.debug_guess_capture(True)

    def close(self):
        self.ctx.close()

    # -- layout --
    def padded(self, adjoint):
        """the converged fields of the last evaluation in the padded layout (S, NZP, NYP) of the guess; pad nodes zero"""
        c = self.ctx
        e, h = c.fields(adjoint=adjoint)
        out = np.zeros((c.S, c.NZP, c.NYP), dtype=np.complex128)
        for mode, a in enumerate((e, h)):
            out[mode * c.nFreq:(mode + 1) * c.nFreq, :c.nz + 1, :c.ny + 1] = a.T.reshape(c.nFreq, c.nz + 1, c.ny + 1)
        return out

    def interior(self, a):
        return a[:, 1:self.ctx.nz, 1:self.ctx.ny]

    # -- events --
    def reset(self, forward=True, adjoint=True):
        self.ref.reset(forward, adjoint)
        if forward:
            self.fields[0] = []
        if adjoint:
            self.fields[1] = []

    def evaluate(self, m, entry="host"):
        """one gradient evaluation at m through the host or the device-pointer entry point, checked against the reference"""
        c = self.ctx
        want = self.ref.evaluate(m, grad=True, entry=entry)
        assert want is not None, "the path revisits a model the host entry points answer from their memo"
        if entry == "host":
            out = c.grad(m)
        else:
            import torch
            if self.dev is None:
                z = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
                self.dev = (z(c.nAC), z(2 * c.nData), z(1), z(c.nAC))
            self.dev[0].copy_(torch.from_numpy(np.ascontiguousarray(m)))
            torch.cuda.synchronize()
            c.grad_device(*(t.data_ptr() for t in self.dev))
            out = None
        assert c.stats()["status"] == 0
        for kind in (0, 1):
            self.check(kind, want[kind])
        return out, want

    def check(self, kind, want):
        c = self.ctx
        for name, val in want.margins.items():
            away = 0.02 if name.startswith("cos") else (0.5 if name == "repeat" else 0.05)
            assert abs(float(val)) > away, f"the path comes within {away} of the threshold {name}: {float(val):.3g}"
        got = c.debug_extrap(adjoint=bool(kind))
        w = got["weights"]
        npoints = int(np.flatnonzero(w).max() + 1) if w.any() else 0
        label = f"kind {kind} call {len(self.seen[kind])}"
        # (a) decisions exactly, weights within the bar
        assert (got["keep"], got["count"], got["head"], got["model_head"]) == (want.keep, want.count, want.head, want.model_head), (label, got, want)
        assert npoints == want.npoints, (label, got, want)
        wbar = want.weight_bar()
        werr = np.abs(w.astype(R.LD) - want.weights).astype(float)
        print(f"[gpu] {label}: keep {want.keep} points {want.npoints} weight error {werr.max():.2e} (bar {wbar.max():.2e})")
        assert (werr <= wbar).all(), (label, w, want.weights, werr, wbar)
        self.worst_w = max(self.worst_w, float((werr / np.where(wbar > 0, wbar, 1.0)).max()))
        # (b) the guess the solve started from
        guess = c.debug_guess(adjoint=bool(kind))
        assert np.isfinite(guess).all()
        hist = self.fields[kind]
        outside = guess.copy()
        if kind == 0:
            outside[:, :c.nz + 1, :c.ny + 1] = 0                     # (the forward boundary nodes belong to the boundary-value kernel)
            assert not outside.any(), f"{label}: pad nodes of the forward guess were written"
        else:
            self.interior(outside)[...] = 0
            prev = hist[0] if hist else np.zeros_like(guess)
            prev = prev.copy(); self.interior(prev)[...] = 0
            assert np.array_equal(outside, prev), f"{label}: boundary or pad nodes of the adjoint guess were written"
        gi = self.interior(guess)
        if not hist:
            assert not gi.any(), f"{label}: a cold start does not begin from zero"
        elif want.keep:
            assert np.array_equal(gi, self.interior(hist[0])), f"{label}: a repeat does not start from the previous solution"
        else:
            xs = [self.interior(x) for x in hist[:R.POINTS]]
            re, im = R.combine(want.weights, xs)
            gbar = R.guess_bar(want.weights, wbar, xs)
            gerr = np.maximum(np.abs(gi.real.astype(R.LD) - re), np.abs(gi.imag.astype(R.LD) - im)).astype(float)
            ok = gerr <= gbar
            scale = max(np.abs(xs[0]).max(), 1e-300)
            print(f"[gpu] {label}: guess error {gerr.max() / scale:.2e} of max|x| (bar {gbar.max() / scale:.2e})")
            assert ok.all(), (label, f"{(~ok).sum()} of {ok.size} interior nodes off, worst {gerr.max():.3e} against {gbar[np.unravel_index(gerr.argmax(), gerr.shape)]:.3e}",
                              want.weights, w)
            if gbar.max() > 0:
                self.worst_g = max(self.worst_g, float((gerr[gbar > 0] / gbar[gbar > 0]).max()))
            if want.npoints == 0:
                assert not gi.any(), f"{label}: the adjoint's cold-unless-smooth guess is not zero"
        # the outgoing solution: what the next call will find as x_k (a repeat's re-solve takes the place of the previous one)
        x = self.padded(bool(kind))
        if want.keep and hist:
            hist[0] = x
        else:
            hist.insert(0, x)
            del hist[R.POINTS:]
        self.seen[kind].append(want.npoints)

    def report(self, what):
        print(f"[gpu] {what}: worst weight error {self.worst_w:.2e} of its bar, worst guess error {self.worst_g:.2e} of its bar")


RAMP = (1.0, 1.3, 1.1, 1.6, 1.2, 1.8, 1.05, 1.5, 1.25, 1.7, 1.15, 1.4)      # unequal lengths, every ratio of two inside (0.55, 1.8)


@pytest.mark.parametrize("name", ["tiny", "cfg2", "wide"])
def test_ramp_up_on_a_straight_path_with_unequal_steps(monkeypatch, name):
    """A straight stretch of unequal steps: orders two to six are reached one by one and then held while the field ring (5 slots)
    and the model ring (7) wrap; only unequal steps expose an error in the times tau_j.  The adjoint solve starts from zero until
    three points exist and from the reference's weights from then on, its outgoing fields stored all the while."""
    d = Drive(monkeypatch, name)
    try:
        u, _ = _frame(d.ctx.nAC)
        lengths = RAMP if name != "wide" else RAMP[:8]
        for m in _models(d.m0, [0.02 * L * u for L in lengths]):
            d.evaluate(m)
        want_f = [1, 1, 2, 3, 4, 5] + [6] * (len(lengths) - 5)
        assert d.seen[0] == want_f and d.seen[1] == [p if p >= 3 else 0 for p in want_f], d.seen
        d.report(f"ramp {name}")
    finally:
        d.close()


def _threshold_steps(which, u, v):
    h = 0.02
    if which == "length":
        # a step of 0.4 and one of 2.5 times the last in the middle of a stretch: that point and all older ones drop out
        return [h * L * u for L in (1, 1, 1, 1, 0.4, 1, 1, 1, 1, 2.5, 1, 1, 1)], \
               [1, 1, 2, 3, 4, 2, 2, 2, 3, 4, 2, 2, 2, 3]
    if which == "collinear":
        # a step at cos 0.99 against the last one is used (and so are the straight ones behind it, seen from it); at cos 0.90 it is
        # not, and the stretch behind the bend is invisible from the new direction
        t99 = 0.99 * u + np.sqrt(1 - 0.99 ** 2) * v
        t90 = 0.90 * u + np.sqrt(1 - 0.90 ** 2) * v
        return [h * s for s in (u, u, u, t99, u, u, t90, t90, t90, t90)], [1, 1, 2, 3, 4, 5, 6, 2, 2, 3, 4]
    if which == "clamp":
        # a new step of +5 and one of -3 times the last: alpha clamped to 2 and to -1
        h = 0.004
        return [h * L * u for L in (1, 1, 1, 5, -15, -9, -6, -5)], [1, 1, 2, 3, 2, 2, 2, 3, 3]
    raise KeyError(which)


@pytest.mark.parametrize("which,name", [(w, n) for w in ("length", "collinear", "clamp") for n in ("tiny", "cfg2")] + [("collinear", "wide")])
def test_thresholds_are_taken_from_the_side_the_path_approaches_them(monkeypatch, name, which):
    """Length exclusion, collinearity and the clamp of alpha, each approached from a known side: the number of points of every call
    is the one written down beside the path, and state and guess are the reference's.  (The bent path also runs on the 120 x 72 mesh:
    on a straight path every step is a multiple of one vector, so alpha, every g_j and every cosine come out the same from ANY subset
    of the parameters -- a block left out of the reduction or cells summed twice by a wrong grid stride show only where the steps
    are not parallel, and only on a mesh whose 32nd block and second pass have work.)"""
    d = Drive(monkeypatch, name)
    try:
        u, v = _frame(d.ctx.nAC)
        steps, points = _threshold_steps(which, u, v)
        wants = [d.evaluate(m)[1] for m in _models(d.m0, steps)]
        assert d.seen[0] == points, (d.seen[0], points)
        assert d.seen[1] == [p if p >= 3 else 0 for p in points]
        if which == "clamp":                                              # (the reference's own clamp, which the device was held to)
            assert wants[4][0].alpha > 4.9 and wants[4][0].weights[:2].tolist() == [3, -2]
            assert wants[5][0].alpha < -2.9 and wants[5][0].weights[:2].tolist() == [0, 1]
        d.report(f"{which} {name}")
    finally:
        d.close()


@pytest.mark.parametrize("name", ["tiny", "cfg2"])
def test_repeat_through_the_device_entry_point(monkeypatch, name):
    """The same model again through hmcmt_grad_device (the host entry points answer repeats from their memo and never reach the
    kernel): keep = 1, heads and count unmoved, a guess that is the previous solution bit for bit -- twice in a row -- and the next
    new model still extrapolates at full order."""
    d = Drive(monkeypatch, name)
    try:
        u, _ = _frame(d.ctx.nAC)
        path = _models(d.m0, [0.02 * L * u for L in RAMP[:7]])
        for m in path[:7]:
            d.evaluate(m, entry="device")
        before = [d.ctx.debug_extrap(adjoint=k) for k in (False, True)]
        for _ in range(2):
            _, want = d.evaluate(path[6].copy(), entry="device")
            assert want[0].keep == 1 and want[1].keep == 1
            after = [d.ctx.debug_extrap(adjoint=k) for k in (False, True)]
            for b, a in zip(before, after):
                assert (a["keep"], a["count"], a["head"], a["model_head"]) == (1, b["count"], b["head"], b["model_head"])
            assert d.ctx.stats()["iters_fwd_max"] <= 3 and d.ctx.stats()["iters_adj_max"] <= 3
        d.evaluate(path[7], entry="device")
        assert d.seen[0][-1] == 6 and d.seen[1][-1] == 6
        d.report(f"repeat {name}")
    finally:
        d.close()


def test_point_cap_of_three(monkeypatch):
    """HMCMT_EXTRAP_POINTS = 3: never more than three fields, whatever the path allows."""
    d = Drive(monkeypatch, "cfg2", cap=3)
    try:
        u, _ = _frame(d.ctx.nAC)
        for m in _models(d.m0, [0.02 * L * u for L in RAMP[:8]]):
            d.evaluate(m)
        assert d.seen[0] == [1, 1, 2] + [3] * 6 and d.seen[1] == [0, 0, 0] + [3] * 6
        d.report("cap 3 cfg2")
    finally:
        d.close()


@pytest.mark.parametrize("event", ["failed", "verify", "jacobian", "products"])
def test_resets_and_borrowers_between_two_evaluations(monkeypatch, event):
    """What comes between two evaluations of a straight stretch and what it does to the history, per the code: an evaluation that
    fails (maxit = 2) and a round trip through options.verify empty both histories -- the next evaluation starts cold, from zero --;
    the explicit Jacobian (at another model) leaves everything as it found it; hmcmt_linearize, here at the current model, starts the
    FORWARD history again at its own model (it is a forward evaluation from a zero guess) and leaves the adjoint's alone, and the
    products behind it touch neither."""
    d = Drive(monkeypatch, "cfg2")
    try:
        c = d.ctx
        u, _ = _frame(c.nAC)
        path = _models(d.m0, [0.02 * L * u for L in RAMP[:10]])
        for m in path[:6]:
            d.evaluate(m)
        assert d.seen[0][-1] == 5
        state = lambda: [c.debug_extrap(adjoint=k) for k in (False, True)]
        same = lambda a, b: all(np.array_equal(x["weights"], y["weights"]) and [x[k] for k in ("keep", "count", "head", "model_head")] ==
                                [y[k] for k in ("keep", "count", "head", "model_head")] for x, y in zip(a, b))
        before = state()
        if event == "failed":
            maxit = c.opts.maxit
            c.set_options(maxit=2)
            with pytest.raises(HmcmtError):
                c.grad(path[6])
            c.set_options(maxit=maxit)
            d.reset()
        elif event == "verify":
            c.set_options(verify=1)
            c.forward(path[6])
            c.set_options(verify=0)
            d.reset()
        elif event == "jacobian":
            x0 = [d.padded(False), d.padded(True)]
            J = c.jacobian(path[6], rows=(0, 3))
            assert np.isfinite(J).all()
            assert same(before, state())
            assert np.array_equal(x0[0], d.padded(False)) and np.array_equal(x0[1], d.padded(True))
        else:
            c.linearize(path[5])
            jv = c.jvp(u / np.sqrt(c.nAC))
            assert np.isfinite(jv).all()
            d.reset(forward=True, adjoint=False)
            want = d.ref.kinds[0].call(path[5])
            after = state()
            assert same(before[1:], after[1:])                             # the adjoint history: untouched
            assert (after[0]["count"], after[0]["head"], after[0]["model_head"], after[0]["weights"].tolist()) == \
                   (want.count, want.head, want.model_head, [1, 0, 0, 0, 0, 0])
            assert not d.interior(c.debug_guess()).any()                   # (the linearisation's forward solve started from zero)
            d.fields[0] = [d.padded(False)]
        for m in path[7:] if event in ("failed", "verify") else path[6:]:
            d.evaluate(m)
        expect = {"failed": ([1, 1, 2, 3], [0, 0, 0, 3]), "verify": ([1, 1, 2, 3], [0, 0, 0, 3]), "jacobian": ([6, 6, 6, 6], [6, 6, 6, 6]),
                  "products": ([2, 3, 4, 5], [6, 6, 6, 6])}[event]
        assert d.seen[0][-4:] == expect[0] and d.seen[1][-4:] == expect[1], d.seen
        d.report(f"event {event}")
    finally:
        d.close()


def test_capture_changes_no_result(monkeypatch):
    """The same path in two fresh contexts, guess capture on and off: predicted data, misfit and gradient bitwise equal, iteration
    counts identical."""
    runs = []
    for capture in (True, False):
        d = Drive(monkeypatch, "cfg2", capture=capture)
        try:
            u, _ = _frame(d.ctx.nAC)
            out = []
            for m in _models(d.m0, [0.02 * L * u for L in RAMP[:8]]):
                pred, mis, grad = d.ctx.grad(m)
                out.append((pred, mis, grad, d.ctx.iters().copy()))
            if not capture:
                with pytest.raises(HmcmtError):
                    d.ctx.debug_guess()
            runs.append(out)
        finally:
            d.close()
    for (p1, f1, g1, i1), (p2, f2, g2, i2) in zip(*runs):
        assert np.array_equal(p1, p2) and f1 == f2 and np.array_equal(g1, g2) and np.array_equal(i1, i2)
