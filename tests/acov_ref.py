"""Pure-numpy reference of the chain's autocovariance accumulator (hmcmt_chain_acov_*, hmcmt_chain_ess; include/hmcmt.h): the
two-pass estimator, the streamed state and its read-out, Geyer's initial positive sequence, the multi-chain rule from full
histories, and the error bounds the tests hold the library to.  Chains are x[ntarget, N]: rows = targets, columns = counted commits."""
import math

import numpy as np

U = 2.0 ** -53


def two_pass(x, K):
    """c_k = (1/N) sum_{t=k}^{N-1} (x_t - xbar)(x_{t-k} - xbar), k = 0 .. K, [K + 1, ntarget]; 0 for k >= N.  Sums by math.fsum."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nt, N = x.shape
    out = np.zeros((K + 1, nt))
    for j in range(nt):
        d = x[j] - math.fsum(x[j]) / N
        for k in range(min(K, N - 1) + 1):
            out[k, j] = math.fsum(d[k:] * d[:N - k]) / N
    return out


def streamed_state(x, K):
    """What the device holds after the N commits x: x0, tot (serial adds), H_k (serial adds of the first k values y), the ring
    (slot t mod (K + 1) = y_t), S_k by math.fsum of the rounded products, and absS_k = sum |y_t y_{t-k}| for the bounds."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    nt, N = x.shape
    x0 = x[:, 0].copy()
    y = x - x0[:, None]                                   # one subtraction
    tot = np.zeros(nt)
    cum = np.zeros((N + 1, nt))
    for t in range(N):
        tot = tot + y[:, t]
        cum[t + 1] = tot
    H = np.array([cum[min(k, N)] for k in range(K + 1)])
    ring = np.zeros((K + 1, nt))
    for t in range(N):
        ring[t % (K + 1)] = y[:, t]
    S, absS = np.zeros((K + 1, nt)), np.zeros((K + 1, nt))
    for k in range(min(K, N - 1) + 1):
        p = y[:, k:] * y[:, :N - k]
        S[k] = [math.fsum(r) for r in p]
        absS[k] = [math.fsum(np.abs(r)) for r in p]
    return {"x0": x0, "tot": tot, "H": H, "ring": ring, "S": S, "absS": absS, "y": y, "N": N, "K": K}


def readout(st, S=None):
    """The read-out formula on the reference's own sums (S: another S_k to put through it): (mean, acov, c_bound).  T_k is added
    newest first, as the library adds it.  c_bound_k = [S_bound_k + 16 u (|S_k| + |ybar| (|A_k| + |B_k|) + (N - k) ybar^2)] / N with
    S_bound_k = (N + 4) u absS_k."""
    N, K, y = st["N"], st["K"], st["y"]
    S = st["S"] if S is None else S
    nt = y.shape[0]
    ybar = st["tot"] / N
    acov, bound = np.zeros((K + 1, nt)), np.zeros((K + 1, nt))
    T = np.zeros(nt)
    for k in range(min(K, N - 1) + 1):
        if k > 0:
            T = T + y[:, N - k]
        A, B = st["tot"] - st["H"][k], st["tot"] - T
        acov[k] = (S[k] - ybar * (A + B) + (N - k) * (ybar * ybar)) / N
        bound[k] = (s_bound(st)[k] + 16 * U * (np.abs(S[k]) + np.abs(ybar) * (np.abs(A) + np.abs(B)) + (N - k) * ybar * ybar)) / N
    return st["x0"] + ybar, acov, bound


def s_bound(st):
    """|S_k - ref| <= (N + 4) u sum |y_t y_{t-k}|: the fma chain's N roundings and the reference's rounded products"""
    return (st["N"] + 4) * U * st["absS"]


def geyer(acov, N):
    """(tau, ess, window, gammas): the initial positive sequence per target; gammas[j] = the Gamma_m looked at, the stopping one
    included."""
    acov = np.asarray(acov, dtype=np.float64)
    K, nt = acov.shape[0] - 1, acov.shape[1]
    lg = max(1.0, math.log10(N))
    tau, ess, window, gammas = np.empty(nt), np.empty(nt), np.zeros(nt, dtype=np.int32), []
    kmax = min(K, N - 1)
    npairs = (kmax - 1) // 2 + 1 if kmax >= 1 else 0
    for j in range(nt):
        c0 = acov[0, j]
        g = []
        if not c0 > 0.0:
            tau[j], ess[j], window[j] = N, 1.0, 0
            gammas.append(g)
            continue
        s, M, ended = 0.0, 0, False
        for m in range(npairs):
            G = (acov[2 * m, j] + acov[2 * m + 1, j]) / c0
            g.append(G)
            if not G > 0.0:
                ended = True
                break
            s += G
            M += 1
        tau[j] = -1.0 + 2.0 * s
        window[j] = M if ended else -M
        ess[j] = N * lg if (tau[j] <= 1.0 / lg or N / tau[j] > N * lg) else N / tau[j]
        gammas.append(g)
    return tau, ess, window, gammas


def tau_bound(acov, cbound, gammas):
    """The bound of tau that follows from the bounds of c_k: per pair looked at, (b_2m + b_2m+1) / c_0 + |Gamma_m| b_0 / c_0; tau
    holds 2 sum Gamma_m, and the whole is doubled."""
    nt = acov.shape[1]
    out = np.zeros(nt)
    for j in range(nt):
        c0 = acov[0, j]
        for m, G in enumerate(gammas[j]):
            out[j] += (cbound[2 * m, j] + cbound[2 * m + 1, j]) / c0 + abs(G) * cbound[0, j] / c0
    return 2.0 * 2.0 * out


def tie_free(gammas, eps=1e-9):
    """False for the targets whose stop could fall either way: some |Gamma_m| looked at is below eps"""
    return np.array([all(abs(G) >= eps for G in g) for g in gammas])


def multi_chain(chains, K):
    """The BDA3 / Stan effective sample size of C chains x[ntarget, N] of equal N from their full histories:
    (tau, ess, window, rho[K + 1, ntarget])."""
    chains = [np.atleast_2d(np.asarray(c, dtype=np.float64)) for c in chains]
    C, (nt, N) = len(chains), chains[0].shape
    chat = np.array([two_pass(c, K) for c in chains]) * (N / (N - 1.0))
    means = np.array([c.mean(axis=1) for c in chains])
    W = chat[:, 0].mean(axis=0)
    BN = means.var(axis=0, ddof=1) if C > 1 else np.zeros(nt)
    varp = W * (N - 1.0) / N + BN
    rho = 1.0 - (W - chat.mean(axis=0)) / varp
    tau, ess, window = np.empty(nt), np.empty(nt), np.zeros(nt, dtype=np.int32)
    kmax = min(K, N - 1)
    npairs = (kmax - 1) // 2 + 1 if kmax >= 1 else 0
    n = C * N
    lg = max(1.0, math.log10(n))
    for j in range(nt):
        s, M, ended = 0.0, 0, False
        for m in range(npairs):
            G = rho[2 * m, j] + rho[2 * m + 1, j]
            if not G > 0.0:
                ended = True
                break
            s += G
            M += 1
        tau[j] = -1.0 + 2.0 * s
        window[j] = M if ended else -M
        ess[j] = n * lg if (tau[j] <= 1.0 / lg or n / tau[j] > n * lg) else n / tau[j]
    return tau, ess, window, rho


def ar1(rng, phi, N, offset=-4.0, scale=0.3):
    """planted AR(1) cells x[len(phi), N] around `offset` (a ln sigma), stationary start"""
    phi = np.asarray(phi, dtype=np.float64)
    x = np.empty((len(phi), N))
    x[:, 0] = rng.standard_normal(len(phi)) / np.sqrt(1.0 - phi * phi)
    for t in range(1, N):
        x[:, t] = phi * x[:, t - 1] + rng.standard_normal(len(phi))
    return offset + scale * x
