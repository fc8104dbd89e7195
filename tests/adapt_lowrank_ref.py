"""numpy reference of the low-rank mass adaptation (hmcmt_chain_adapt_lowrank, include/hmcmt.h):

    W = [Zd; Zg],  Zd = (X - mean X) / s / sqrt(n - 1),  Zg = (G - mean G) s / sqrt(n - 1),  K = W W'
    K = V D V' (D_i > 1e-10 D_max kept), T = D^-1/2 V',  Pd = T K[:, :n], Pg = T K[:, n:],  Cd = Pd Pd' + gamma I, Cg = Pg Pg' + gamma I
    Sigma = Cg^-1/2 (Cg^1/2 Cd Cg^1/2)^1/2 Cg^-1/2 = Y Theta Y',  U = (T' Y_sel)' W

Two forms.  `estimate` is the estimator with an eigensolver of its own, a round-robin Jacobi in longdouble (the library's is cyclic Jacobi
in double; eig="lapack": numpy.linalg.eigh, which is six digits short on these graded matrices -- see eigh_ld).
`means`, `w_rows`, `gram`, `lift`, `fix_signs` are the device kernels' arithmetic in the kernels' order (hmcmt_items.h: item_adapt_lr_*)
with the exact array fma of tests/mass_lowrank_ref.py, so the host instantiation of those functions (tests/emul/emul_adapt_lowrank.cpp)
must give the same bits; the `_ld` forms carry the same sums in longdouble.  `schedule` is the window bookkeeping in plain Python."""
import numpy as np

from tests.mass_lowrank_ref import fma

NMIN, NMAX = 4, 128


# ---- the estimator ----------------------------------------------------------------------------------------------------------------
# Its eigenproblems are graded: Cg and Cd have an (n - 1)-fold eigenvalue gamma beside eigenvalues of order 1 to 100, and Sigma divides
# by Cg's square roots.  LAPACK's eigh returns small eigenvalues to eps |A|, not to eps of themselves, which at gamma = 1e-5 costs the
# estimate six digits (measured against the long-double form on the planted problem: 1.5e-6 in theta).  The reference's own solver
# is therefore a Jacobi method, which is accurate relative to each eigenvalue of such matrices, carried in numpy's longdouble -- in
# round-robin order with all disjoint rotations of a round applied at once, so independent of the library's cyclic double-precision one
# in ordering, precision and code.  eig="lapack" keeps numpy.linalg.eigh for comparison.
LD = np.longdouble


def eigh_ld(A, max_sweeps=60, start=True):
    """(d ascending, V columns) of a symmetric A, in longdouble: parallel-order (round-robin) Jacobi.  start: LAPACK's eigenvectors V0
    first, then Jacobi on V0' A V0, which is nearly diagonal and takes two or three sweeps instead of ten (V0 is orthogonal to 1e-15,
    and a congruence that close to orthogonal moves every eigenvalue by that much of ITSELF -- Ostrowski -- so the grading survives)"""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    if n > 2 and start:
        V0 = np.linalg.eigh(np.asarray(A, dtype=np.float64))[1].astype(LD)
        d, V1 = eigh_ld(V0.T @ A @ V0, max_sweeps, start=False)
        return d, V0 @ V1
    V = np.eye(n, dtype=LD)
    if n == 1:
        return A[0].copy(), V
    eps = np.finfo(LD).eps
    floor = LD(1e-60) * np.sqrt((A * A).sum())
    players = list(range(n + n % 2))
    for _ in range(max_sweeps):
        rotated = 0
        for _round in range(len(players) - 1):
            half = len(players) // 2
            pairs = [(min(players[i], players[-1 - i]), max(players[i], players[-1 - i])) for i in range(half)]
            pairs = [(i, j) for i, j in pairs if j < n]
            players = [players[0]] + [players[-1]] + players[1:-1]
            p, q = np.array([i for i, _ in pairs]), np.array([j for _, j in pairs])
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            on = (np.abs(apq) > eps * np.sqrt(np.abs(app * aqq))) & (np.abs(apq) > floor)
            if not on.any():
                continue
            rotated += int(on.sum())
            safe = np.where(on, apq, LD(1))
            theta = (aqq - app) / (2 * safe)
            t = np.where(theta >= 0, LD(1), LD(-1)) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            c = np.where(on, 1 / np.sqrt(t * t + 1), LD(1))
            sn = np.where(on, t * c, LD(0))
            Ap, Aq = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * Ap - sn[:, None] * Aq, sn[:, None] * Ap + c[:, None] * Aq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c[None, :] * Ap - sn[None, :] * Aq, sn[None, :] * Ap + c[None, :] * Aq
            A[p[on], q[on]] = 0
            A[q[on], p[on]] = 0
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c[None, :] * Vp - sn[None, :] * Vq, sn[None, :] * Vp + c[None, :] * Vq
        if rotated == 0:
            break
    d = np.diag(A).copy()
    order = np.argsort(d, kind="stable")
    return d[order], V[:, order]


def _eig(A, eig):
    return eigh_ld(A) if eig == "ld" else np.linalg.eigh(np.asarray(A, dtype=np.float64))


def sym_pow(C, p, eig="lapack"):
    w, v = _eig(C, eig)
    return (v * w ** p) @ v.T


def scaled_rows(X, G, invM):
    """W [2n, nAC] in plain numpy"""
    X, G = np.asarray(X, dtype=np.float64), np.asarray(G, dtype=np.float64)
    n = X.shape[0]
    s = np.sqrt(np.asarray(invM, dtype=np.float64))
    return np.vstack([(X - X.mean(0)) / s / np.sqrt(n - 1.0), (G - G.mean(0)) * s / np.sqrt(n - 1.0)])


def select(theta, rank, cutoff):
    """indices of the directions kept: theta > cutoff or theta < 1 / cutoff, by |ln theta| descending (stable), at most rank"""
    order = np.argsort(-np.abs(np.log(theta)), kind="stable")
    return [int(i) for i in order if theta[i] > cutoff or theta[i] < 1.0 / cutoff][:rank]


def estimate_from_gram(K, n, rank=8, cutoff=2.0, gamma=1e-5, geometric=True, eig="ld"):
    """(B [2n, r], theta_sel, theta_all ascending) from K = W W'; geometric=False: the arithmetic mean (Cd + Cg^-1) / 2 in Sigma's place.
    eig="ld" (longdouble throughout, results rounded to double at the end) or "lapack" (double, numpy.linalg.eigh)"""
    ft = LD if eig == "ld" else np.float64
    K = np.asarray(K, dtype=ft)
    # (K's eigenvalues span four decades and only fix a basis of the rows' span, and Sigma's theta span two: LAPACK serves both; the
    # graded ones are Cg and the matrix under the square root)
    d, V = (a.astype(ft) for a in np.linalg.eigh(np.asarray(K, dtype=np.float64)))
    keep = d > 1e-10 * d.max()
    d, V = d[keep], V[:, keep]
    T = (V / np.sqrt(d)).T
    Pd, Pg = T @ K[:, :n], T @ K[:, n:]
    m = len(d)
    Cd, Cg = Pd @ Pd.T + ft(gamma) * np.eye(m, dtype=ft), Pg @ Pg.T + ft(gamma) * np.eye(m, dtype=ft)
    if geometric:
        # in the eigenbasis of Cg, where its powers are diagonal scalings (a dense Cg^+-1/2 would round the eigenvalues near gamma away)
        g, Q = _eig(Cg, eig)
        sg = np.sqrt(g)
        Cq = Q.T @ Cd @ Q
        mid = sg[:, None] * (0.5 * (Cq + Cq.T)) * sg[None, :]
        Sig = Q @ (sym_pow(mid, ft(0.5), eig) / sg[:, None] / sg[None, :]) @ Q.T
    else:
        Sig = 0.5 * (Cd + np.linalg.inv(np.asarray(Cg, dtype=np.float64)).astype(ft))
    th, Y = (a.astype(ft) for a in np.linalg.eigh(np.asarray(0.5 * (Sig + Sig.T), dtype=np.float64)))
    sel = select(th, rank, cutoff)
    return np.asarray(T.T @ Y[:, sel], dtype=np.float64), np.asarray(th[sel], dtype=np.float64), np.asarray(th, dtype=np.float64)


def fix_signs(U):
    """each row's entry of largest magnitude positive, the lowest index among equals (np.argmax returns the first)"""
    U = np.array(U, dtype=np.float64)
    for k in range(U.shape[0]):
        if U[k, np.argmax(np.abs(U[k]))] < 0:
            U[k] = -U[k]
    return U


def estimate(X, G, invM, rank=8, cutoff=2.0, gamma=1e-5, geometric=True, eig="ld"):
    """(U [r, nAC] with the sign convention, lambda [r], theta_all [m] ascending)"""
    W = scaled_rows(X, G, invM)
    B, lam, th = estimate_from_gram(W @ W.T, np.asarray(X).shape[0], rank, cutoff, gamma, geometric, eig)
    return fix_signs(B.T @ W), lam, th


def window_invM(X_window):
    """the diagonal rule of the adaptation on ALL n_w samples of a window (not the thinned rows): var w + f"""
    Xw = np.asarray(X_window, dtype=np.float64)
    nw = Xw.shape[0]
    return Xw.var(0, ddof=1) * (nw / (nw + 5.0)) + 1e-3 * 5.0 / (nw + 5.0)


# ---- the kernels' order ---------------------------------------------------------------------------------------------------------------
def means(R):
    """a cell's mean over the stored rows: the rows added upwards, one division"""
    R = np.asarray(R, dtype=np.float64)
    acc = np.zeros(R.shape[1])
    for i in range(R.shape[0]):
        acc = acc + R[i]
    return acc / float(R.shape[0])


def w_rows(X, G, invM, rows=None):
    """W[rows] as item_adapt_lr_w forms it: ((x - mean) / s) / sq and ((g - mean) s) / sq, s = sqrt(invM), sq = sqrt(n - 1)"""
    X, G = np.asarray(X, dtype=np.float64), np.asarray(G, dtype=np.float64)
    n = X.shape[0]
    s, sq = np.sqrt(np.asarray(invM, dtype=np.float64)), np.sqrt(float(n - 1))
    mx, mg = means(X), means(G)
    rows = range(2 * n) if rows is None else rows
    return np.array([((X[i] - mx) / s) / sq if i < n else ((G[i - n] - mg) * s) / sq for i in rows])


def gram_pairs(W, pairs):
    """K[i][j] for the given (i, j): ONE fma chain over the cells upwards from 0 (k_adapt_lr_gram's thread)"""
    pi, pj = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    acc = np.zeros(len(pairs))
    A, B = np.ascontiguousarray(W[pi].T), np.ascontiguousarray(W[pj].T)      # [nAC, npairs]: a step of the chain is one row
    for a in range(W.shape[1]):
        acc = fma(A[a], B[a], acc)
    return acc


def gram(W):
    N2 = W.shape[0]
    pairs = [(i, j) for i in range(N2) for j in range(N2)]
    return gram_pairs(W, pairs).reshape(N2, N2)


def lift(W, B):
    """U[k][a] = sum_i B[i][k] W[i][a], i upwards by fma"""
    r = B.shape[1]
    acc = np.zeros((r, W.shape[1]))
    for i in range(W.shape[0]):
        acc = fma(B[i][:, None], W[i][None, :], acc)
    return acc


def gram_ld(W, pairs=None):
    """the same sums in longdouble, with the absolute-summand sums sum_a |w_i[a] w_j[a]| the error bars scale with"""
    Wl = np.asarray(W, dtype=np.longdouble)
    if pairs is None:
        return Wl @ Wl.T, np.abs(Wl) @ np.abs(Wl).T
    pi, pj = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    return (Wl[pi] * Wl[pj]).sum(1), (np.abs(Wl[pi]) * np.abs(Wl[pj])).sum(1)


def w_rows_ld(X, G, invM):
    X, G = np.asarray(X, dtype=np.longdouble), np.asarray(G, dtype=np.longdouble)
    n = X.shape[0]
    s, sq = np.sqrt(np.asarray(invM, dtype=np.longdouble)), np.sqrt(np.longdouble(n - 1))
    return np.vstack([(X - X.mean(0)) / s / sq, (G - G.mean(0)) * s / sq])


# ---- problems ---------------------------------------------------------------------------------------------------------------------
def planted(seed, nAC=390, n=100, lam0=(60.0, 15.0, 0.04)):
    """(X, G, invM, U0 [nAC, 3]): draws of N(0, S B S), B = I + U0 (lam0 - I) U0', scales exp(U(-2, 1)); G = (S B S)^-1 X;
    invM = the draws' sample variances (the estimated scales, not the true ones)"""
    rng = np.random.default_rng(seed)
    lam0 = np.asarray(lam0)
    U0, _ = np.linalg.qr(rng.standard_normal((nAC, len(lam0))))
    s0 = np.exp(rng.uniform(-2, 1, nAC))
    Binv = np.eye(nAC) + (U0 * (1 / lam0 - 1)) @ U0.T
    F = np.eye(nAC) + (U0 * (np.sqrt(lam0) - 1)) @ U0.T
    X = (F @ rng.standard_normal((nAC, n))).T * s0
    G = ((Binv @ (X / s0).T).T) / s0
    return X, G, X.var(0, ddof=1), U0


def rows_problem(nAC, n, seed=None):
    """(X, G, invM) for the kernels: correlated rows with offsets, so that the centring matters"""
    rng = np.random.default_rng(7000 + 13 * nAC + n if seed is None else seed)
    X = 1.5 + rng.standard_normal((n, nAC)) * rng.uniform(0.1, 2.0, nAC)
    G = -0.7 + rng.standard_normal((n, nAC)) * rng.uniform(0.5, 5.0, nAC) + 0.3 * X
    return X, G, rng.uniform(0.25, 4.0, nAC)


# ---- the window bookkeeping ---------------------------------------------------------------------------------------------------------
def stride_of(length, max_samples):
    return 1 if length <= max_samples else -(-length // max_samples)


def windows_of(nwarmup, init_buffer, term_buffer, base_window):
    """[(first step, last step)] of Stan's schedule (hmcmt.h, hmcmt_chain_adapt_begin 4.)"""
    out, start, end, size = [], init_buffer, init_buffer + base_window - 1, base_window
    last = nwarmup - term_buffer - 1
    while True:
        out.append((start, end))
        if end == last:
            return out
        size *= 2
        nxt = end + size
        if nxt != last and nxt + 2 * size >= nwarmup - term_buffer:
            nxt = last
        start, end = end + 1, nxt


def schedule(nwarmup, init_buffer, term_buffer, base_window, max_samples):
    """per window: dict(first, last, stride, steps stored (absolute step indices), fallback (fewer than NMIN pairs))"""
    out = []
    for first, last in windows_of(nwarmup, init_buffer, term_buffer, base_window):
        st = stride_of(last - first + 1, max_samples)
        steps = [c for c in range(first, last + 1) if (c - first) % st == 0]
        out.append({"first": first, "last": last, "stride": st, "steps": steps, "fallback": len(steps) < NMIN})
    return out
