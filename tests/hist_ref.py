"""An independent restatement of the chain's histogram contract (include/hmcmt.h: hmcmt_chain_hist_*), for the host and the GPU
tests: plain loops over rows and bins, nothing shared with hmcmt_items.h or sampler.histQuantiles."""
import numpy as np


def bin_of(m, nbins, lo, hi):
    """numpy's bits of the header's rule: t = (m - lo) * scale with scale = nbins / (hi - lo), clamped into the edge bins"""
    scale = np.float64(nbins) / (np.float64(hi) - np.float64(lo))
    t = (np.asarray(m, dtype=np.float64) - np.float64(lo)) * scale
    b = np.where(t < 0, 0, np.where(t >= nbins, nbins - 1, np.trunc(np.clip(t, 0, nbins)).astype(np.int64)))
    return b.astype(np.int64)


def counts_of(committed, targets, nbins, lo, hi):
    """committed: a list of models [nAC] -> counts[ntarget, nbins] int64"""
    targets = np.asarray(targets, dtype=np.int64)
    counts = np.zeros((len(targets), nbins), dtype=np.int64)
    for m in committed:
        b = bin_of(np.asarray(m)[targets], nbins, lo, hi)
        for r in range(len(targets)):
            counts[r, b[r]] += 1
    return counts


def quantile_row(row, N, nbins, lo, hi, q):
    """(bin, value) of one row: the first bin with a count whose inclusive cumulative count reaches x = q * N"""
    x = np.float64(q) * np.float64(N)
    w = (np.float64(hi) - np.float64(lo)) / np.float64(nbins)
    cum = 0
    for b in range(nbins):
        c = int(row[b])
        if c > 0 and np.float64(cum + c) >= x:
            return b, float(np.float64(lo) + w * (np.float64(b) + (x - np.float64(cum)) / np.float64(c)))
        cum += c
    raise AssertionError("the row holds fewer than q * N counts")


def quantiles(counts, N, lo, hi, q):
    """(values[nq, ntarget], bins[nq, ntarget])"""
    counts = np.asarray(counts)
    nt, nbins = counts.shape
    q = np.atleast_1d(q)
    vals, bins = np.empty((len(q), nt)), np.empty((len(q), nt), dtype=np.int64)
    for i, qi in enumerate(q):
        for r in range(nt):
            bins[i, r], vals[i, r] = quantile_row(counts[r], N, nbins, lo, hi, qi)
    return vals, bins


def quantile_bound(lo, hi):
    """five roundings, each at most one ulp of a quantity no larger than max(|lo|, |hi|), doubled for a contracted against an
    uncontracted last step"""
    return 8 * 2.0 ** -52 * max(abs(lo), abs(hi))
