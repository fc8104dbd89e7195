"""A plain reference of what the device-resident HMC chain (hmcmt_chain_*) computes per sample: pure numpy, every sum in
np.longdouble, no GPU, no ctypes and nothing of the library's.  tests/test_chain_host.py holds it to the host instantiation of
the item functions (tests/emul), tests/test_gpu_chain_kernels.py holds the kernels to it."""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
ZCLIP = 2.5                                    # getMomentumVector clips the normals at +-2.5


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def momentum(z, invM):
    """(p, K): p = clip(z, +-2.5) / sqrt(invM) rounded to float64 once, K = 0.5 sum p^2 invM of the unrounded p"""
    zc = np.clip(np.asarray(z, dtype=np.float64), -ZCLIP, ZCLIP)
    w = _ld(invM)
    p = zc.astype(LD) / np.sqrt(w)
    return p.astype(np.float64), float(0.5 * (p * p * w).sum())


def kinetic(p, invM=None, x=None):
    """0.5 sum p (invM p) for the diagonal mass, or 0.5 sum p x with x = M^-1 p given"""
    if (invM is None) == (x is None):
        raise ValueError("kinetic: one of invM and x")
    p = _ld(p)
    return float(0.5 * (p * (_ld(invM) * p if x is None else _ld(x))).sum())


def mnorm(m, mref, Wm, lam):
    """(0.5 lam d'Wm d, S) with d = m - mref and S = 0.5 lam sum_a |d_a| sum_j |Wm_aj| |d_j|, the scale of the sum's rounding error.
    Wm: a scipy sparse matrix (anything with tocoo()) or a dense array."""
    d = _ld(m) - _ld(mref)
    if hasattr(Wm, "tocoo"):
        coo = Wm.tocoo()
        row, col, val = np.asarray(coo.row), np.asarray(coo.col), _ld(coo.data)
    else:
        dense = np.asarray(Wm, dtype=np.float64)
        row, col = np.nonzero(dense)
        val = _ld(dense[row, col])
    terms = d[row] * val * d[col]
    half = LD(0.5) * LD(lam)
    return float(half * terms.sum()), float(abs(half) * np.abs(terms).sum())


def misfit(pred, inv):
    """sampler.compDataMisfit's formula: 0.5 sum |dataW (pred - obs)|^2"""
    res = np.asarray(pred, dtype=np.complex128).astype(CLD) - np.asarray(inv.obsData, dtype=np.complex128).astype(CLD)
    w = _ld(inv.dataW)
    return float(0.5 * (w * w * (res.real * res.real + res.imag * res.imag)).sum())


def moments(samples):
    """Two-pass (count, mean, m2) of the columns of samples [nparam, nsamples] (the layout of hmcmodel); m2 = sum of squared
    deviations from the mean"""
    x = _ld(samples)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("moments: samples [nparam, nsamples] with at least one sample")
    count = x.shape[1]
    mean = x.sum(axis=1) / LD(count)
    dev = x - mean[:, None]
    return count, mean.astype(np.float64), (dev * dev).sum(axis=1).astype(np.float64)


def moments_bounds(mean_ref, m2_ref, count):
    """(bound on |mean - mean_ref|, bound on |m2 / count - var_ref| per parameter) of float64 Welford against a two-pass reference:
    the mean to 4 eps of the largest mean, the variance to 16 eps max(|mean| / std, 1) relative -- the update subtracts the running
    mean from a sample, which cancels |mean| / std digits.  Measured on the host (n = 20000, ten samples with repeats, moves of
    0.02): 1.1 eps and a factor of 1.5; the flat 1e-12 var of test_welford_item_against_two_pass_numpy breaks there (2.8e-12)."""
    var = m2_ref / count
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(var > 0, np.maximum(np.abs(mean_ref) / np.sqrt(var), 1.0), 1.0)
    return 4 * np.finfo(np.float64).eps * np.abs(mean_ref).max(), 16 * np.finfo(np.float64).eps * cond * var


def decision(D, M, K0, D1, K1, M1, u):
    """(hdif, accepted) in float64, in hmcmt_chain_step's order of operations"""
    D, M, K0, D1, K1, M1 = (np.float64(v) for v in (D, M, K0, D1, K1, M1))
    hdif = (D + M + K0) - (D1 + K1 + M1)
    with np.errstate(over="ignore", under="ignore"):
        accepted = bool(hdif > 0 or np.float64(u) < np.exp(hdif))
    return float(hdif), accepted
