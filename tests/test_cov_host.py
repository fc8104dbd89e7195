"""The chain's covariance accumulator without a GPU (hmcmt_chain_cov_*, hmcmt_chain_corr): the item bodies of hmcmt_items.h through
their test-only host instantiation (tests/emul/emul_cov.cpp) against the longdouble two-pass reference and the derived bounds of
tests/cov_ref.py; batch and visit-order independence bit for bit; the exact equalities of the contract; the Python helpers covOf,
mergeCov, fileio.getCorrelationModel; the ABI's new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd import sampler
from tests import cov_ref as R
from tests.conftest import ROOT
from tests.emul import emul_cov_py as E

ROWSETS = [None, [5, 5, 39, 0], [3, 11, 7]]


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def results(x, rows, batch, reverse=False):
    st = E.accumulate(x, rows, batch, reverse=reverse)
    mean, var, cov = E.readout(st)
    return mean, var, cov, E.corr(st)


@pytest.fixture(scope="module")
def hist():
    return R.histories(np.random.default_rng(5))


def test_constants_are_the_headers():
    c = E.constants()
    header = open(os.path.join(ROOT, "include", "hmcmt.h")).read()
    assert c["batch_max"] == L.COV_BATCH_MAX == 16 == int(re.search(r"#define HMCMT_COV_BATCH_MAX (\d+)", header).group(1))
    assert c["batch_default"] == 8 and "0: the default, 8" in header
    # the GPU test's shapes (96 and 390 cells) meet every tile edge only for tiles of at most 256 cells by 195 rows
    assert c["tile_cols"] <= 256 and c["tile_rows"] <= 195 and c["tile_cols"] % 64 == 0


@pytest.mark.parametrize("N", [1, 2, 3, 50])
@pytest.mark.parametrize("rows", ROWSETS)
def test_values_against_the_longdouble_reference(hist, rows, N):
    """far-off pivot, constant cells (0, 7), identical cells (3, 11), N = 1 and 2"""
    x = hist[:, :N]
    mean, var, cov, corr = results(x, rows, 8)
    rmean, rvar, rcov, rcorr = R.two_pass(x, rows)
    bmean, bvar, bcov = R.bounds(x, rows)
    em, ev, ec = np.abs(mean - rmean).astype(float), np.abs(var - rvar).astype(float), np.abs(cov - rcov).astype(float)
    worst = max(np.max(e[b > 0] / b[b > 0], initial=0.0) for e, b in ((em, bmean), (ev, bvar), (ec, bcov)))
    print(f"\n[rows {rows}, N {N}] largest error over its bound {worst:.3g}")
    assert np.all(em <= bmean) and np.all(ev <= bvar) and np.all(ec <= bcov)
    assert N < 50 or abs(float(rmean[1]) - x[1, 0]) > 4.0     # (the pivot is far off the mean)
    # correlations under the propagated bound; ill-conditioned denominators (bound > 0.5) left out, at most 1 %
    bcorr = R.corr_bound(rcov.astype(float), rvar.astype(float), bcov, bvar, rows)
    keep = bcorr <= 0.5
    assert (~keep).mean() <= 0.01, f"{(~keep).sum()} of {keep.size} correlations left out"
    assert np.all(np.abs(corr - rcorr).astype(float)[keep] <= bcorr[keep])
    assert np.all(np.abs(corr) <= 1.0)
    if N == 1:
        assert np.all(var == 0.0) and np.all(cov == 0.0) and np.all(corr == 0.0) and np.array_equal(mean, x[:, 0])


@pytest.mark.parametrize("rows", ROWSETS)
def test_batch_length_and_a_read_out_inside_a_batch_change_no_bit(hist, rows):
    ref = results(hist, rows, 1)
    for B in (3, 8, 16, 0):
        assert same(results(hist, rows, B), ref), B
    for B, cut in ((8, 13), (16, 5), (3, 49)):
        st = E.commit(E.begin(hist.shape[0], rows, B), hist[:, :cut], flush=True)      # a read-out with a partly filled batch ...
        early = E.readout(st) + (E.corr(st),)
        assert same(early, results(hist[:, :cut], rows, 1))
        E.commit(st, hist[:, cut:], flush=True)                                          # ... changes no later bit
        assert same(E.readout(st) + (E.corr(st),), ref), (B, cut)


def test_row_tiles_in_another_order_change_no_bit():
    rng = np.random.default_rng(11)
    n = 2 * E.constants()["tile_rows"] + 5                                               # three row tiles, the last one partial
    x = -4.0 + 0.3 * rng.standard_normal((n, 20))
    for rows in (None, rng.integers(0, n, n + 3)):
        assert same(results(x, rows, 3, reverse=True), results(x, rows, 3))
        assert same(results(x, rows, 8, reverse=True), results(x, rows, 1))


def test_the_exact_equalities_of_the_contract(hist):
    n = hist.shape[0]
    mean, var, cov, corr = results(hist, None, 8)
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()                        # symmetric bit for bit
    assert np.array_equal(np.diag(cov), var)
    for c in (0, 7):                                                                     # a cell that never moved
        assert np.all(cov[c] == 0.0) and np.all(cov[:, c] == 0.0) and var[c] == 0.0 and np.all(corr[c] == 0.0) and np.all(corr[:, c] == 0.0)
    moved = var > 0
    assert moved.sum() == n - 2 and np.all(np.diag(corr)[moved] == 1.0)
    assert np.array_equal(cov[3], cov[11]) and corr[3, 11] == 1.0                        # identical cells
    rows = np.array([5, 5, n - 1, 0])
    mean2, var2, cov2, corr2 = results(hist, rows, 3)
    assert same((mean2, var2), (mean, var)) and np.array_equal(cov2, cov[rows]) and np.array_equal(corr2, corr[rows])
    assert np.array_equal(cov2[0], cov2[1]) and all(cov2[i, r] == var[r] for i, r in enumerate(rows))
    assert corr2[0, 5] == 1.0 and corr2[2, n - 1] == 1.0 and corr2[3, 0] == 0.0


def test_the_reference_itself_keeps_its_correlations_well_conditioned(hist):
    """the share of entries the propagated bound cannot hold to 0.5 stays within 1 % for the histories the tests use"""
    for N in (2, 3, 22, 50):
        x = hist[:, :N]
        _, rvar, rcov, _ = R.two_pass(x)
        _, bvar, bcov = R.bounds(x)
        b = R.corr_bound(rcov.astype(float), rvar.astype(float), bcov, bvar)
        assert (b > 0.5).mean() <= 0.01 and np.all(b[[0, 7]] == 0.0)


@pytest.mark.parametrize("rows", ROWSETS)
def test_covOf_is_the_reference(hist, rows):
    c = sampler.covOf(hist, rows)
    rmean, rvar, rcov, rcorr = R.two_pass(hist, rows)
    bmean, bvar, bcov = R.covof_bound(hist, rows)
    assert c["count"] == hist.shape[1] and np.array_equal(c["rows"], np.arange(hist.shape[0]) if rows is None else rows)
    assert np.all(np.abs(c["mean"] - rmean) <= bmean) and np.all(np.abs(c["var"] - rvar) <= bvar) and np.all(np.abs(c["cov"] - rcov) <= bcov)
    bcorr = R.corr_bound(rcov.astype(float), rvar.astype(float), bcov, bvar, rows)
    keep = bcorr <= 0.5
    assert (~keep).mean() <= 0.01 and np.all(np.abs(c["corr"] - rcorr).astype(float)[keep] <= bcorr[keep])
    with pytest.raises(ValueError):
        sampler.covOf(hist[0])


@pytest.mark.parametrize("rows", ROWSETS)
def test_mergeCov_of_a_split_history_is_the_unsplit_one(hist, rows):
    """pooled from the emulated accumulator's halves, against the reference of the whole, under the parts' bounds pooled the same way
    plus the merge's own roundings: the means' errors reach cov through d_c, every sum and product of the merge costs a few u"""
    cut = 19
    N = hist.shape[1]
    r = np.arange(hist.shape[0]) if rows is None else np.asarray(rows)
    rmean, rvar, rcov, rcorr = R.two_pass(hist, rows)
    parts, pb = [], []
    for x in (hist[:, :cut], hist[:, cut:]):
        st = E.accumulate(x, rows, 8)
        mean, var, cov = E.readout(st)
        parts.append({"count": x.shape[1], "rows": r, "mean": mean, "var": var, "cov": cov, "corr": E.corr(st)})
        pb.append(R.bounds(x, rows))
    w = [p["count"] / N for p in parts]
    bm = sum(wc * b[0] for wc, b in zip(w, pb)) + 8 * R.U * np.abs(rmean).astype(float)        # the pooled mean
    bsum_v, bsum_c = 0.0, 0.0
    for wc, p, b in zip(w, parts, pb):
        d = np.abs(p["mean"] - rmean.astype(float))
        ed = b[0] + bm + 2 * R.U * d                                                     # the error of d_c = xbar_c - xbar
        dd = lambda da, db, ea, eb: da * eb + db * ea + ea * eb                          # ... and of a product of two of them
        bsum_v = bsum_v + wc * (b[1] + dd(d, d, ed, ed) + 16 * R.U * (np.abs(p["var"]) + d * d))
        bsum_c = bsum_c + wc * (b[2] + dd(d[r][:, None], d[None, :], ed[r][:, None], ed[None, :])
                                + 16 * R.U * (np.abs(p["cov"]) + d[r][:, None] * d[None, :]))
    m = sampler.mergeCov(parts)
    assert m["count"] == N and m["nchains"] == 2 and np.array_equal(m["rows"], r)
    assert np.all(np.abs(m["mean"] - rmean) <= bm)
    assert np.all(np.abs(m["var"] - rvar) <= bsum_v) and np.all(np.abs(m["cov"] - rcov) <= bsum_c)
    bcorr = R.corr_bound(rcov.astype(float), rvar.astype(float), bsum_c, bsum_v, rows)
    keep = bcorr <= 0.5
    assert (~keep).mean() <= 0.01 and np.all(np.abs(m["corr"] - rcorr).astype(float)[keep] <= bcorr[keep])
    with pytest.raises(ValueError):
        sampler.mergeCov([parts[0], dict(parts[1], rows=r[::-1].copy())])
    with pytest.raises(ValueError):
        sampler.mergeCov([])


def test_getCorrelationModel_round_trips_through_its_reader(tmp_path):
    from hmcmt2d_amd import fileio
    from tests.helpers import make_problem
    mesh, data, inv, m = make_problem("tiny")
    n = len(inv.activeIdx)
    x = -4.0 + 0.3 * np.random.default_rng(2).standard_normal((n, 30))
    c = sampler.covOf(x, [4, n - 1])
    path = str(tmp_path / "corr.model")
    row = fileio.getCorrelationModel(path, c, 1, mesh, inv)
    assert np.array_equal(row, c["corr"][1]) and row[n - 1] == 1.0
    back = fileio.readCorrelationModel(path, inv)
    assert back.shape == (n,) and np.all(np.abs(back - row) <= 0.5e-2 * np.abs(row) + 1e-12)      # (%4.2e: three digits)
    assert np.array_equal(fileio.getCorrelationModel(path, c, 0, mesh, inv, write=False), c["corr"][0])
    for bad in (2, -1):
        with pytest.raises(ValueError):
            fileio.getCorrelationModel(path, c, bad, mesh, inv)


def test_abi_of_the_new_symbols():
    """declared, exported, in the Python mirror; NULL context -> HMCMT_EINVAL before anything else"""
    so = ctypes.CDLL(L.build_library())
    header = open(os.path.join(ROOT, "include", "hmcmt.h")).read()
    for sym in ("hmcmt_chain_cov_begin", "hmcmt_chain_cov", "hmcmt_chain_corr"):
        assert re.search(r"extern int %s\(" % sym, header) and sym in L.CHAIN_COV_SYMBOLS and sym in L.PRODUCT_SYMBOLS and hasattr(so, sym)
    lib = L.load_library()
    assert lib.hmcmt_chain_cov_begin(None, 0, None, 0) == -1 and lib.hmcmt_chain_cov(None, None, None, None, None, 0) == -1
    assert lib.hmcmt_chain_corr(None, None, 0) == -1
    assert lib.hmcmt_debug_chain_cov_time(None, -1, None, None) == -1 and "hmcmt_debug_chain_cov_time" in L.DEBUG_SYMBOLS
    for name in ("chain_cov_begin", "chain_cov", "chain_cov_device", "chain_corr", "chain_cov_count", "chain_cov_timing"):
        assert callable(getattr(L.HipContext, name))
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    for name in ("chainCovBegin!", "chainCov", "chainCorr", "chain_cov!"):
        assert re.search(r"^function %s\(" % re.escape(name), jl, flags=re.M) and name in jl.split("const libhmcmt")[0]


def test_sampler_refuses_cov_without_the_device_chain_and_unknown_keys():
    from hmcmt2d_amd.structs import HMCPrior
    prior = HMCPrior(totalsamples=2, burninsamples=0, dt=0.01, timestep=[1, 1], sigBounds=[1e-4, 1.0], regParam=1.0)
    with pytest.raises(ValueError, match="cov needs device_chain"):
        sampler.runHMCSampler(None, None, None, prior, cov={})
    with pytest.raises(ValueError, match="cov has no key"):
        sampler.runHMCSampler(None, None, None, prior, device_chain=True, cov={"row": [1]})
