"""Longdouble reference of the chain's covariance accumulator (hmcmt_chain_cov_*, hmcmt_chain_corr; include/hmcmt.h): the two-pass
estimator, and the error bounds the tests hold the library to, derived from the library's summation order.  Histories are
x[nparam, N]: rows = cells, columns = counted commits; rows = the cells rho of the matrix's rows (None: every cell).

The bounds.  u = 2^-53, gamma_k = k u / (1 - k u).  The device forms y_t = fl(x_t - x0) (one rounding: y_t = (x_t - x0)(1 + d), |d| <= u),
then   tot = serial sum of y   |tot - sum y| <= gamma_(N-1) sum|y|,   S = fma chain   |S - sum y_rho y_a| <= gamma_N sum|y_rho y_a|
(q is S with rho = a), and reads out  p = fl(tot_rho tot_a), c = fl(p / N), d = fl(S - c), cov = fl(d / N).  With the rounding of y
itself (2 u on every product, u on every term of tot) that gives, for Y_a = sum|x_a - x0_a|, P = sum|(x_rho - x0_rho)(x_a - x0_a)|,
T the exact sums and e_a = gamma_(N+1) Y_a:
    |cov - exact| <= [ gamma_(N+2) P + (|T_rho| e_a + |T_a| e_rho + e_rho e_a) / N + 2 u |T_rho T_a| / N + u |S - c| ] / N + u |cov|
    |mean - exact| <= e_a / N + u |T_a| / N + u |mean|
The covariance does not depend on the pivot, so `exact` is the two-pass value.  The reference's own error (longdouble) is added.  Every
bound carries a factor 1 + 1e-6 for the products of two roundings left out above (they are below N^2 u^2 relative to a term kept)."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
ULD = float(np.finfo(LD).eps) / 2
SLACK = 1.0 + 1e-6


def gamma(k):
    return k * U / (1.0 - k * U)


def two_pass(x, rows=None):
    """(mean[n], var[n], cov[nrow, n], corr[nrow, n]) in longdouble: cov = (1/N) sum (x_rho - xbar_rho)(x_a - xbar_a); corr is 0 where a
    variance is not positive"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n, N = x.shape
    r = np.arange(n) if rows is None else np.asarray(rows)
    mean = x.sum(axis=1) / LD(N)
    d = x - mean[:, None]
    var = (d * d).sum(axis=1) / LD(N)
    cov = (d[r] @ d.T) / LD(N)
    ok = (var[r][:, None] > 0) & (var[None, :] > 0)
    den = np.sqrt(np.where(ok, var[r][:, None] * var[None, :], LD(1)))
    corr = np.where(ok, cov / den, LD(0))
    return mean, var, cov, corr


def bounds(x, rows=None):
    """(bmean[n], bvar[n], bcov[nrow, n]) for the library's results on the history x (module docstring)"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n, N = x.shape
    r = np.arange(n) if rows is None else np.asarray(rows)
    y = x - x[:, :1]                                       # exact pivot differences (longdouble holds them to 2^-64)
    ay = np.abs(y)
    T, Y = y.sum(axis=1), ay.sum(axis=1)
    e = gamma(N + 1) * Y
    mean, var, cov, _ = two_pass(x, rows)
    d = x - mean[:, None]
    ad = np.abs(d)

    def b(P, Tr, Ta, er, ea, val, Pd):
        dev = (gamma(N + 2) * P + (np.abs(Tr) * ea + np.abs(Ta) * er + er * ea) / N + 2 * U * np.abs(Tr * Ta) / N
               + U * np.abs(val * N)) / N + U * np.abs(val)       # (S - c = N cov)
        ref = 4 * (N + 4) * ULD * Pd / N                   # (the reference: rounded deviations, products and sums in longdouble)
        return ((dev + ref) * SLACK).astype(np.float64)

    bcov = b(ay[r] @ ay.T, T[r][:, None], T[None, :], e[r][:, None], e[None, :], cov, ad[r] @ ad.T)
    bvar = b((ay * ay).sum(axis=1), T, T, e, e, var, (ad * ad).sum(axis=1))
    bmean = ((e / N + U * np.abs(T) / N + U * np.abs(mean) + 4 * N * ULD * np.abs(x).sum(axis=1) / N) * SLACK).astype(np.float64)
    return bmean, bvar, bcov


def corr_bound(cov, var, bcov, bvar, rows=None):
    """the bound of corr = cov / sqrt(var_rho var_a) that follows from the bounds of cov and var: with rel = bvar_rho / var_rho +
    bvar_a / var_a < 1/2, the denominator D = sqrt(var_rho var_a) moves by at most D rel / (1 - rel), so
        |dcorr| <= (bcov / D + |corr| rel) / (1 - rel) + 4 u   (product, square root, division, and the reference's own)
    -- inf where rel >= 1/2 (an ill-conditioned denominator); 0 where the reference's variance is not positive and the library's
    bound says the library's is not either (both give 0.0).  The clamp into [-1, 1] moves a value towards the reference."""
    n = len(var)
    r = np.arange(n) if rows is None else np.asarray(rows)
    var, cov = np.asarray(var, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    vr, va, br, ba = var[r][:, None], var[None, :], bvar[r][:, None], bvar[None, :]
    ok = (vr > 0) & (va > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ok, br / vr + ba / va, 0.0)
        D = np.sqrt(np.where(ok, vr * va, 1.0))
        out = (bcov / D + np.abs(cov / D) * rel) / (1.0 - rel) + 4 * U
    out = np.where(rel >= 0.5, np.inf, out)
    # a cell whose exact variance is zero never moved: the library's sums for it are exact zeros (contract), so is its corr
    return np.where(ok, out * SLACK, 0.0)


def covof_bound(x, rows=None):
    """(bmean, bvar, bcov) for the float64 two-pass estimator of sampler.covOf: the mean by a (pairwise or serial) sum, error at most
    gamma_N sum|x| / N =: em; the deviations rounded (u each) and moved by em; the products summed in any order, gamma_N:
        |cov - exact| <= [ gamma_(N+2) sum|d_rho d_a| + em_rho sum|d_a| + em_a sum|d_rho| + N em_rho em_a ] / N + u |cov|"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n, N = x.shape
    r = np.arange(n) if rows is None else np.asarray(rows)
    mean, var, cov, _ = two_pass(x, rows)
    ad = np.abs(x - mean[:, None])
    D1 = ad.sum(axis=1)
    em = gamma(N) * np.abs(x).sum(axis=1) / N + U * np.abs(mean)

    def b(P, er, ea, Dr, Da, val):
        return (((gamma(N + 2) * P + er * Da + ea * Dr + N * er * ea) / N + U * np.abs(val) + 4 * (N + 4) * ULD * P / N) * SLACK).astype(np.float64)

    return (em * SLACK).astype(np.float64), b((ad * ad).sum(axis=1), em, em, D1, D1, var), \
        b(ad[r] @ ad.T, em[r][:, None], em[None, :], D1[r][:, None], D1[None, :], cov)


def histories(rng, n=40, N=50):
    """synthetic histories x[n, N] around ln sigma = -4 with what the tests ask for: correlated cells (a few shared factors), a far-off
    pivot (the first sample several units away from the mean), constant cells (0, 7), two identical cells (3, 11)"""
    f = rng.standard_normal((4, N))
    load = rng.standard_normal((n, 4))
    x = -4.0 + 0.3 * (load @ f) + 0.2 * rng.standard_normal((n, N))
    x[:, 0] += 5.0                                          # the pivot lies far off
    x[0] = -4.0
    x[7] = 1.25
    x[11] = x[3]
    return x
