"""Independent reference of the initial-guess extrapolation (options.warm_start of include/hmcmt.h), numpy long double
throughout.  Written from the description, not from the kernels: it keeps the models an evaluation stream has seen as a plain Python
list per solve kind (newest first) and decides, for every new model, what the extrapolation must do.

The rule.  With m_new the model of the call and m_k, m_{k-1}, ... the earlier ones of the kind (count of them, at most POINTS):
  * count = 0 (first call, or the history was reset): the guess is the solver's zero fill -- weight 1 on it for the forward solve,
    all weights 0 for the adjoint solve ("cold unless smooth").
  * a repeat, |m_new - m_k|^2 <= 1e-28 |m_k|^2: the previous solution, weight 1, for both kinds; nothing is stored, nothing moves.
  * count = 1: the previous solution (forward), zero (adjoint).
  * count >= 2: steps d_0 = m_new - m_k, d_j = m_{k-j+1} - m_{k-j}; alpha = <d_0,d_1>/<d_1,d_1> clamped to [-1, 2]; the linear guess
    (1 + alpha) x_k - alpha x_{k-1}.  If d_0 is collinear with d_1 (cos > 0.95) and of comparable length (0.5 < alpha < 2), every
    further step d_j, j = 2, 3, ..., that exists (count >= j + 1), is collinear with d_1 (cos > 0.95) and of comparable length
    (0.5 < g_j = <d_j,d_1>/<d_1,d_1> < 2) adds the point x_{k-j} at the "time" tau_j = tau_{j-1} - g_j (tau_0 = 0, tau_1 = -1); the
    first step that fails ends the list.  The points are capped at `cap` (HMCMT_EXTRAP_POINTS, 2..6).  With three or more points
    the weights are the Lagrange basis polynomials over tau_0..tau_{np-1} at alpha.  The adjoint solve takes zero weights unless
    there are at least three points.
  * unless the call was a repeat the model is stored (count <- min(count + 1, POINTS)) and both ring heads move back by one: the
    field ring has POINTS - 1 slots, the model ring POINTS + 1.
A forward-only evaluation moves the forward history alone.  A reset (a failed evaluation, a change of options) empties the histories
and puts the heads back to 0."""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
POINTS = 6                     # fields of the extrapolation: the current one and five earlier ones
FIELD_SLOTS, MODEL_SLOTS = POINTS - 1, POINTS + 1
COS_MIN, LEN_MIN, LEN_MAX = LD("0.95"), LD("0.5"), LD(2)
ALPHA_MIN, ALPHA_MAX = LD(-1), LD(2)
REPEAT_REL = LD("1e-28")
EPS = LD(2.0) ** -53           # unit roundoff of the fp64 sums the kernels form


def _dot(a, b):
    return np.dot(np.asarray(a, dtype=LD), np.asarray(b, dtype=LD))


def lagrange_weights(alpha, g, npoints):
    """Weights of x_k, x_{k-1}, ..., x_{k-5} (long double [POINTS]) for `npoints` >= 2 points: alpha = the new step in units of the
    last one, g = (g_2, g_3, ...) the earlier steps in the same unit."""
    alpha = LD(alpha)
    w = np.zeros(POINTS, dtype=LD)
    if npoints == 2:
        w[0], w[1] = 1 + alpha, -alpha
        return w
    tau = [LD(0), LD(-1)]
    for j in range(2, npoints):
        tau.append(tau[-1] - LD(g[j - 2]))
    for i in range(npoints):
        l = LD(1)
        for j in range(npoints):
            if j != i:
                l *= (alpha - tau[j]) / (tau[i] - tau[j])
        w[i] = l
    return w


@dataclass
class Result:
    """What one call did for one solve kind."""
    keep: int                          # 1: the model was a repeat
    npoints: int                       # fields with a weight (0: the adjoint's cold start)
    weights: np.ndarray                # long double [POINTS], of x_k, x_{k-1}, ...
    count: int                         # models in the history after the call
    head: int                          # head of the field ring after the call
    model_head: int                    # head of the model ring after the call
    margins: dict = field(default_factory=dict)   # every decision taken: name -> distance from its threshold (sign = outcome)
    alpha: LD = LD(0)                  # unclamped
    g: tuple = ()                      # g_2 .. of the points used
    nAC: int = 0
    npoints_path: int = 0              # points the path allowed before the adjoint rule zeroed the weights

    def decided(self, away=1e-9):
        return all(abs(float(v)) > away for v in self.margins.values())

    def weight_bar(self):
        """First-order error bound of the weights, [POINTS] float: the kernel's inner products are plain fp64 sums of nAC products
        and, for the points used, cos > 0.95, so alpha and every g_j carry a relative error of at most about nAC 2^-53 / 0.95.  The
        weights are formed again with alpha and every g_j of the points used moved by +-4 nAC 2^-53 (relative) in all sign patterns;
        bar = 4 x the largest change per weight + 8 x 2^-53 max|w|."""
        w = self.weights
        base = 8 * EPS * np.abs(w).max()
        if self.npoints < 2 or self.keep:              # (1 or 0 exactly: nothing was computed)
            return np.full(POINTS, float(base))
        rel = 4 * self.nAC * EPS
        used = self.npoints
        ng = used - 2
        change = np.zeros(POINTS, dtype=LD)
        for signs in itertools.product((-1, 1), repeat=1 + ng):
            a = min(ALPHA_MAX, max(ALPHA_MIN, self.alpha * (1 + signs[0] * rel)))
            gp = [self.g[i] * (1 + signs[1 + i] * rel) for i in range(ng)]
            wp = lagrange_weights(a, gp, used)
            change = np.maximum(change, np.abs(wp - w))
        return (4 * change + base).astype(float)


class KindHistory:
    """The history of one solve kind: models newest first."""

    def __init__(self, adjoint, cap=POINTS):
        assert 2 <= cap <= POINTS
        self.adjoint, self.cap = bool(adjoint), int(cap)
        self.reset()

    def reset(self):
        self.models = []               # newest first, at most POINTS
        self.moves = 0                 # non-repeat calls since the reset

    def call(self, m_new):
        m_new = np.asarray(m_new, dtype=LD)
        count = len(self.models)
        margins = {}
        w = np.zeros(POINTS, dtype=LD)
        alpha, gs, npts, keep = LD(0), [], 0, 0
        if count >= 1:
            d0 = m_new - self.models[0]
            # (|dm|^2 - 1e-28 |m|^2 in units of 1e-28 |m|^2: an exact repeat reports -1, not a number the size of the threshold)
            thr = REPEAT_REL * _dot(self.models[0], self.models[0])
            margins["repeat"] = (_dot(d0, d0) - thr) / thr
            keep = int(margins["repeat"] <= 0)
        if keep:
            w[0], npts = 1, 1
        elif count <= 1:
            npts = 1
        else:
            d1 = self.models[0] - self.models[1]
            d1d1 = _dot(d1, d1)
            alpha = _dot(d0, d1) / d1d1
            npts = 2
            if count >= 3 and self.cap >= 3:
                cos0 = _dot(d0, d1) / np.sqrt(_dot(d0, d0) * d1d1)
                margins.update({"cos0": cos0 - COS_MIN, "alpha_lo": alpha - LEN_MIN, "alpha_hi": LEN_MAX - alpha})
                if cos0 > COS_MIN and LEN_MIN < alpha < LEN_MAX:
                    for j in range(2, min(count, self.cap)):
                        dj = self.models[j - 1] - self.models[j]
                        pj = _dot(dj, d1)
                        cj, gj = pj / np.sqrt(_dot(dj, dj) * d1d1), pj / d1d1
                        margins.update({f"cos{j}": cj - COS_MIN, f"g{j}_lo": gj - LEN_MIN, f"g{j}_hi": LEN_MAX - gj})
                        if not (cj > COS_MIN and LEN_MIN < gj < LEN_MAX):
                            break
                        gs.append(gj)
                        npts = j + 1
        path_points = npts
        if not keep:
            if npts >= 2:
                w = lagrange_weights(min(ALPHA_MAX, max(ALPHA_MIN, alpha)), gs, npts)
            elif not self.adjoint:
                w[0] = 1
            if self.adjoint and npts <= 2:
                w[:] = 0
                npts = 0
            self.models.insert(0, m_new.copy())
            del self.models[POINTS:]
            self.moves += 1
        return Result(keep=keep, npoints=npts, weights=w, count=len(self.models), head=(-self.moves) % FIELD_SLOTS,
                      model_head=(-self.moves) % MODEL_SLOTS, margins=margins, alpha=alpha, g=tuple(gs[:max(path_points - 2, 0)]),
                      nAC=m_new.size, npoints_path=path_points)


class ExtrapRef:
    """Both kinds of one context, fed with the events of its evaluation stream."""

    def __init__(self, cap=POINTS):
        self.kinds = (KindHistory(False, cap), KindHistory(True, cap))
        self.memo = []                 # the last two distinct models of the host entry points: (bytes, has gradient)

    def reset(self, forward=True, adjoint=True):
        """a failed evaluation, a change of options (both kinds); a new linearisation point (forward)"""
        if forward:
            self.kinds[0].reset()
        if adjoint:
            self.kinds[1].reset()
        self.memo = []

    def evaluate(self, m, grad=True, entry="device"):
        """(forward Result, adjoint Result or None); None when a host entry point answers a repeat from its memo and the kernels
        never see the call.  entry: "host" (hmcmt_grad / hmcmt_forward) or "device" (the device-pointer entry points)."""
        assert entry in ("host", "device")
        key = np.asarray(m, dtype=np.float64).tobytes()
        if entry == "host":
            for k, has_grad in self.memo:
                if k == key and (has_grad or not grad):
                    return None
            self.memo = [(k, g) for k, g in self.memo if k != key]
            self.memo.insert(0, (key, bool(grad)))
            del self.memo[2:]
        else:
            self.memo = []
        return self.kinds[0].call(m), (self.kinds[1].call(m) if grad else None)


def combine(weights, fields):
    """sum_j w_j x_{k-j} in long double: fields = [x_k, x_{k-1}, ...] (complex arrays; fewer than POINTS when the history is short:
    the missing ones must carry a zero weight)."""
    re = np.zeros(np.shape(fields[0]), dtype=LD)
    im = np.zeros(np.shape(fields[0]), dtype=LD)
    for j in range(POINTS):
        wj = LD(weights[j])
        if j >= len(fields):
            assert wj == 0, f"weight {j} is {wj} but the history holds {len(fields)} fields"
            continue
        if wj != 0:
            re += wj * np.asarray(fields[j].real, dtype=LD)
            im += wj * np.asarray(fields[j].imag, dtype=LD)
    return re, im


def guess_bar(weights, wbar, fields):
    """Elementwise bound of |guess - combine(weights, fields)|: sum_j (wbar_j + 8 x 2^-53 |w_j|) |x_{k-j}| (float array)."""
    out = np.zeros(np.shape(fields[0]))
    for j in range(min(POINTS, len(fields))):
        out += (float(wbar[j]) + 8 * float(EPS) * abs(float(weights[j]))) * np.abs(fields[j])
    return out
