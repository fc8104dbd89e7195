"""A reference of the device chain's No-U-turn sampler (hmcmt_chain_nuts_sample, include/hmcmt.h): multinomial NUTS grown leaf by leaf
without recursion, in plain Python over a caller-supplied one-step map.  It is written from the header's description and uses nothing
of the library's; its draws come from tests/rng_ref.py's Philox at the header's counters (or from the caller).

A state is any object with the attributes p (momentum, forward-time sign), x (= M^-1 p) and H (the Hamiltonian); `leaf(state, forward)`
returns the state one leapfrog step further in the direction named (backward: the same map applied to -p, the caller's business)."""
import math

import numpy as np

from tests import rng_ref as R

C0_LEAF, C0_DIR = 0x80000000, 0xC0000000
DIVERGENCE = 1000.0


def rng_nuts(seed, stream, t, kind, index):
    """(forward, u): kind 0, doubling `index`; kind 1, the sample's index-th leaf (forward is 0)"""
    x = R.block(seed, stream, t, (C0_DIR if kind == 0 else C0_LEAF) + index)
    return (x[2] >> 31) if kind == 0 else 0, R.u52(x[0], x[1])


def philox_draws(seed, stream, t):
    return (lambda j: rng_nuts(seed, stream, t, 0, j)), (lambda l: rng_nuts(seed, stream, t, 1, l)[1])


def logaddexp(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    return a + math.log1p(math.exp(b - a)) if a > b else b + math.log1p(math.exp(a - b))


def due_checkpoints(i):
    """the checkpoint slots an odd leaf i checks, in order: popcount(i >> 1) downwards, one per trailing one of i"""
    k = bin(i >> 1).count("1")
    ones = 0
    while (i >> ones) & 1:
        ones += 1
    return [k - c for c in range(ones)]


def _cosine(dot, a, b):
    return abs(dot) / max(float(np.linalg.norm(a)) * float(np.linalg.norm(b)), 1e-300)


def sample(start, leaf, max_depth, draw_dir, draw_leaf, use_weights=True):
    """One sample from `start`.  Returns a dict: depth, nleaves, stop, dirs, selected (signed time index), alpha, state (the selected
    one), energies (H of every leaf, in the order taken), times (their signed time indices), margin (the smallest |u - threshold| / threshold
    of the sample's uniform tests: a threshold is an exp, so an error e of its energies moves it by threshold * e), dot_margin (the
    smallest |cosine| of its U-turn tests: |x.span| / (|x| |span|)).  use_weights=False selects uniformly among the leaves (delta counts as 0 in every weight): a deliberately wrong sampler."""
    H0 = start.H
    ends = {0: start, 1: start}                      # [0] backward, [1] forward
    t_end = {0: 0, 1: 0}
    rho = np.array(start.p, dtype=float)
    logW = 0.0
    sel_state, selected = start, 0
    depth = nleaves = 0
    dirs = 0
    stop = None
    alpha_sum = 0.0
    energies, times = [], []
    margin, dot_margin = math.inf, math.inf
    l = 0
    while stop is None:
        forward, uj = draw_dir(depth)
        if forward:
            dirs |= 1 << depth
        d = 1 if forward else 0
        logWs = -math.inf
        rho_s = np.zeros_like(rho)
        ck = {}
        sub_state, sub_sel = None, 0
        state = ends[d]
        for i in range(1 << depth):
            state = leaf(state, forward)
            u = draw_leaf(l)
            l += 1
            nleaves += 1
            tm = t_end[d] + (i + 1 if forward else -(i + 1))
            energies.append(state.H)
            times.append(tm)
            delta = H0 - state.H
            if not math.isfinite(delta) or -delta > DIVERGENCE:
                stop = 3
                break
            alpha_sum += 1.0 if delta > 0 else math.exp(delta)
            dw = delta if use_weights else 0.0
            logWs = logaddexp(logWs, dw)
            thr = math.exp(dw - logWs)
            if i > 0 and thr > 0.0:
                margin = min(margin, abs(u - thr) / thr)
            if i == 0 or u < thr:
                sub_state, sub_sel = state, tm
            rho_s = rho_s + state.p
            if i % 2 == 0:
                ck[bin(i >> 1).count("1")] = (np.array(state.p, dtype=float), np.array(state.x, dtype=float), rho_s.copy())
            else:
                for k in due_checkpoints(i):
                    pk, xk, rk = ck[k]
                    span = rho_s - rk + pk
                    a, b = float(np.dot(xk, span)), float(np.dot(state.x, span))
                    dot_margin = min(dot_margin, _cosine(a, xk, span), _cosine(b, state.x, span))
                    if not a > 0 or not b > 0:
                        stop = 1
                        break
                if stop is not None:
                    break
        if stop is not None:
            break
        dl = logWs - logW
        thr = math.exp(min(0.0, dl))
        if 0.0 < thr < 1.0:
            margin = min(margin, abs(uj - thr) / thr)
        if uj < thr:
            sel_state, selected = sub_state, sub_sel
        logW = logaddexp(logW, logWs)
        rho = rho + rho_s
        ends[d] = state
        t_end[d] += (1 << depth) if forward else -(1 << depth)
        depth += 1
        a, b = float(np.dot(ends[0].x, rho)), float(np.dot(ends[1].x, rho))
        dot_margin = min(dot_margin, _cosine(a, ends[0].x, rho), _cosine(b, ends[1].x, rho))
        if not a > 0 or not b > 0:
            stop = 2
        elif depth == max_depth:
            stop = 0
    return dict(depth=depth, nleaves=nleaves, stop=stop, dirs=dirs, selected=selected, alpha=alpha_sum / nleaves, state=sel_state,
                energies=energies, times=times, margin=margin, dot_margin=dot_margin)


class State:
    def __init__(self, m, p, x, H, **extra):
        self.m, self.p, self.x, self.H = m, p, x, H
        self.__dict__.update(extra)


class Gaussian:
    """A zero-mean Gaussian target with precision matrix A and a diagonal inverse mass: the plain leapfrog as the one-step map."""

    def __init__(self, A, inv_m, dt):
        self.A, self.inv_m, self.dt = np.asarray(A, dtype=float), np.asarray(inv_m, dtype=float), float(dt)

    def state(self, m, p):
        m, p = np.asarray(m, dtype=float), np.asarray(p, dtype=float)
        x = self.inv_m * p
        return State(m, p, x, 0.5 * float(m @ (self.A @ m)) + 0.5 * float(p @ x))

    def leaf(self, s, forward):
        sg = 1.0 if forward else -1.0
        p = sg * s.p
        p = p - 0.5 * self.dt * (self.A @ s.m)
        m = s.m + self.dt * (self.inv_m * p)
        p = p - 0.5 * self.dt * (self.A @ m)
        return self.state(m, sg * p)
