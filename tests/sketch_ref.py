"""Plain-numpy restatement of the row sketch of the device chain (hmcmt_chain_sketch_*, hmcmt_chain_pca; include/hmcmt.h): the
frequent-directions sketch, the Gram-route principal components and the merge, with numpy.linalg.eigh in place of the library's
Jacobi.  Rows are models: X[N, n].  Written from the header's text, independent of hmcmt2d_amd.sampler."""
import numpy as np


def shrink_T(K, ell):
    """(T[ell, 2 ell], delta) of a Gram matrix K[2 ell, 2 ell]: d descending, delta = max(d[ell], 0),
    c_i = sqrt((d_i - delta) / d_i) if d_i > delta else 0, T[i][j] = c_i V[j][i]"""
    d, V = np.linalg.eigh(K)
    d, V = d[::-1], V[:, ::-1]
    delta = max(d[ell], 0.0)
    T = np.zeros((ell, 2 * ell))
    for i in range(ell):
        if d[i] > delta:
            T[i] = np.sqrt((d[i] - delta) / d[i]) * V[:, i]
    return T, delta


def sketch(X, ell, pivot=None):
    """the sketch of the rows of X[N, n]: dict count, ell, fill, shrinks, Delta, x0, tot, q, rows[fill, n], A (the rows y_t)"""
    X = np.asarray(X, dtype=np.float64)
    N, n = X.shape
    x0 = X[0].copy() if pivot is None else np.asarray(pivot, dtype=np.float64).copy()
    B = np.zeros((2 * ell, n))
    tot, q = np.zeros(n), np.zeros(n)
    fill = shrinks = 0
    Delta = 0.0
    for t in range(N):
        y = X[t] - x0
        tot = tot + y
        q = q + y * y
        B[fill] = y
        fill += 1
        if fill == 2 * ell:
            T, delta = shrink_T(B @ B.T, ell)
            B[:ell] = T @ B
            B[ell:] = 0.0
            Delta += delta
            shrinks += 1
            fill = ell
    return {"count": N, "ell": ell, "fill": fill, "shrinks": shrinks, "Delta": Delta, "pivot_given": int(pivot is not None), "x0": x0,
            "tot": tot, "q": q, "rows": B[:fill].copy(), "A": X - x0[None, :]}


def pca(sk, rank):
    """(lam[r], U[r, n], err) by the Gram route of hmcmt_chain_pca"""
    N = sk["count"]
    ybar = sk["tot"] / N
    W = np.vstack([sk["rows"], np.sqrt(float(N)) * ybar])
    lamG, Q = np.linalg.eigh(W @ W.T)
    keep = lamG > 1e-10 * lamG[-1]
    lamG, Q = lamG[keep], Q[:, keep]
    J = np.ones(W.shape[0])
    J[-1] = -1.0
    S = np.sqrt(lamG)[:, None] * (Q.T @ (J[:, None] * Q)) * np.sqrt(lamG)[None, :]
    th, Z = np.linalg.eigh(0.5 * (S + S.T))
    order = [i for i in np.argsort(-th, kind="stable") if th[i] > 0][:rank]
    U = ((Q / np.sqrt(lamG)[None, :]) @ Z[:, order]).T @ W
    for k in range(len(order)):
        if U[k, np.argmax(np.abs(U[k]))] < 0:
            U[k] = -U[k]
    return th[order] / N, U, sk["Delta"] / N


def merge(sketches):
    """the merged sketch of sketches with one pivot: rows stacked and shrunk, tot, q, N and Delta added"""
    ell, x0 = sketches[0]["ell"], sketches[0]["x0"]
    n = x0.size
    B = np.zeros((2 * ell, n))
    tot, q = np.zeros(n), np.zeros(n)
    fill = shrinks = N = 0
    Delta = 0.0
    for s in sketches:
        assert s["ell"] == ell and s["x0"].tobytes() == x0.tobytes()
        tot, q, N, Delta, shrinks = tot + s["tot"], q + s["q"], N + s["count"], Delta + s["Delta"], shrinks + s["shrinks"]
        for row in s["rows"]:
            B[fill] = row
            fill += 1
            if fill == 2 * ell:
                T, delta = shrink_T(B @ B.T, ell)
                B[:ell] = T @ B
                B[ell:] = 0.0
                Delta += delta
                shrinks += 1
                fill = ell
    return {"count": N, "ell": ell, "fill": fill, "shrinks": shrinks, "Delta": Delta, "pivot_given": 1, "x0": x0.copy(), "tot": tot, "q": q,
            "rows": B[:fill].copy(), "A": np.vstack([s["A"] for s in sketches])}


def centred_cov(A):
    """the exact biased covariance of the rows of A"""
    d = A - A.mean(axis=0)[None, :]
    return d.T @ d / A.shape[0]


def guarantee(sk, A=None):
    """the figures of the guarantee for a sketch against its rows A[N, n]: lmin, lmax of E = A'A - B'B, |A|_F^2, and the bound
    min_k |A - A_k|_F^2 / (ell - k)"""
    A = sk["A"] if A is None else A
    E = A.T @ A - sk["rows"].T @ sk["rows"]
    w = np.linalg.eigvalsh(0.5 * (E + E.T))
    sv2 = np.linalg.svd(A, compute_uv=False) ** 2
    tail = np.concatenate([np.cumsum(sv2[::-1])[::-1], [0.0]])       # tail[k] = |A - A_k|_F^2
    ell = sk["ell"]
    bound = min(tail[min(k, len(tail) - 1)] / (ell - k) for k in range(ell))
    return {"lmin": float(w[0]), "lmax": float(w[-1]), "frob2": float(sv2.sum()), "bound": float(bound)}


def synthetic_chain(n, N, modes=3, seed=0, repeats=0.3):
    """a chain X[N, n] with `modes` strong spatial modes over small noise, and repeats of the previous row (rejections)"""
    rng = np.random.default_rng(seed)
    a = np.arange(n) / n
    P = np.array([np.sin((k + 1) * np.pi * a + 0.3 * k) for k in range(modes)])
    amp = 2.0 / (1.0 + np.arange(modes))
    X = np.empty((N, n))
    base = -2.0 + 0.1 * rng.standard_normal(n)
    for t in range(N):
        if t > 0 and rng.random() < repeats:
            X[t] = X[t - 1]
        else:
            X[t] = base + (amp * rng.standard_normal(modes)) @ P + 0.02 * rng.standard_normal(n)
    return X
