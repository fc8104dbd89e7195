"""Marginal posteriors from the device chain, without a GPU: the bin rule and the quantile scan of hmcmt_items.h on the host
(tests/emul/emul_hist.cpp) against numpy and tests/hist_ref.py, the helpers of sampler.py and fileio.py around them, the ABI of the
five new symbols, and runHMCSampler(device_chain=True, hist=..., data_moments=True) on an oracle-backed stand-in context."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from hmcmt2d_amd import fileio, sampler
from hmcmt2d_amd import lib as L
from hmcmt2d_amd.structs import HMCPrior
from tests.conftest import ROOT
from tests import hist_ref as H
from tests.emul import emul_hist_py as E
from tests.helpers import make_problem, ragged_problem
from tests.test_chain_host import OracleChainContext, _moments

NEW = ["hmcmt_chain_hist_begin", "hmcmt_chain_hist", "hmcmt_chain_hist_quantiles", "hmcmt_chain_data_moments_begin",
       "hmcmt_chain_data_moments"]
QS = [0.0, 0.05, 0.25, 0.5, 0.95, 1.0]


# ---- the bin item ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [1, 2, 300, 4096])
@pytest.mark.parametrize("lo,hi", [(float(np.log(1e-4)), 0.0), (0.0, 3.0), (-2.5, 7.25)])
def test_bin_item_against_numpy(nbins, lo, hi):
    """t = (m - lo) * scale, one subtraction then one product: numpy's bits, so the bins are compared for equality.  Planted: m == lo,
    m == hi, every interior edge that is cheap to reach and one ulp either side of it, values below lo and above hi, -0.0."""
    rng = np.random.default_rng(nbins)
    w = (hi - lo) / nbins
    ks = np.unique(np.concatenate([[1, nbins // 2, nbins - 1], rng.integers(1, max(nbins, 2), 40)]))
    ks = ks[(ks >= 1) & (ks < nbins)]
    edges = lo + w * ks
    m = np.concatenate([[lo, hi, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
                         lo - 1.0, lo - 1e300, hi + 1.0, hi + 1e300, -0.0, 0.0],
                        edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), rng.uniform(lo - 1.0, hi + 1.0, 2000)])
    got, ref = E.bins(m, nbins, lo, hi), H.bin_of(m, nbins, lo, hi)
    assert np.array_equal(got, ref)
    assert got.min() == 0 and got.max() == nbins - 1
    assert got[0] == 0 and got[1] == nbins - 1                       # m == lo: the first bin; m == hi: t == nbins clamps
    assert np.all(got[6:8] == 0) and np.all(got[8:10] == nbins - 1)   # beyond the range: the edge bins
    if lo == 0.0:
        assert got[10] == got[11] == 0                               # -0.0: t = -0.0 is not < 0, (int)-0.0 = 0
    if nbins > 1:
        assert len(np.unique(got)) > 1


def test_histogram_item_counts_equal_numpys():
    """k_chain_hist's body over a few committed models: repeats in the target list are rows of their own, every row sums to the number
    of commits, counts equal the reference's exactly"""
    rng = np.random.default_rng(2)
    n, ns = 390, 9
    lo, hi = float(np.log(1e-4)), 0.0
    S = rng.uniform(lo - 0.5, hi + 0.5, (n, ns))
    S[:, 4] = S[:, 3]                                                # a rejection's repeat
    S[7, :] = lo; S[8, :] = hi
    for targets in (np.arange(n), np.array([5, 5, 389, 0, 7, 8, 5]), np.array([200])):
        for nbins in (1, 2, 300, 4096):
            c = E.accumulate(S, targets, nbins, lo, hi)
            assert c.dtype == np.uint32 and np.array_equal(c, H.counts_of(list(S.T), targets, nbins, lo, hi))
            assert np.all(c.sum(axis=1) == ns)
    c = E.accumulate(S, np.array([7, 8]), 300, lo, hi)
    assert c[0, 0] == ns and c[1, 299] == ns


# ---- the quantile item -------------------------------------------------------------------------------------------------------------
def _quantile_rows(nbins):
    rng = np.random.default_rng(nbins + 11)
    N = 97
    rows = []
    r = np.zeros(nbins, dtype=np.int64); r[rng.integers(0, nbins)] = N; rows.append(r)                # everything in one bin
    r = rng.multinomial(N, np.ones(nbins) / nbins); rows.append(r)                                    # spread (empty bins when nbins > N)
    if nbins >= 8:
        r = np.zeros(nbins, dtype=np.int64)                                                           # full bins with empty ones between
        idx = np.sort(rng.choice(nbins, 4, replace=False))
        r[idx] = [20, 30, 40, 7]; rows.append(r)
        r = np.zeros(nbins, dtype=np.int64); r[0] = 50; r[-1] = 47; rows.append(r)                    # bimodal at the two edges
    return np.array(rows), N


@pytest.mark.parametrize("nbins", [1, 2, 8, 300, 4096])
def test_quantile_item_against_the_reference(nbins):
    """The bin must agree exactly (both sides form q * N once and compare the same integers with it); the value within
    8 * 2^-52 * max(|lo|, |hi|): five roundings of at most one ulp of a quantity no larger than that, doubled for a contracted
    against an uncontracted last step."""
    lo, hi = float(np.log(1e-4)), 0.5
    counts, N = _quantile_rows(nbins)
    assert np.all(counts.sum(axis=1) == N)
    vals, bins = E.quantiles(counts, N, lo, hi, QS)
    rv, rb = H.quantiles(counts, N, lo, hi, QS)
    assert np.array_equal(bins, rb)
    assert np.abs(vals - rv).max() <= H.quantile_bound(lo, hi)
    w = (hi - lo) / nbins
    first = np.array([np.flatnonzero(r)[0] for r in counts]); last = np.array([np.flatnonzero(r)[-1] for r in counts])
    assert np.array_equal(bins[0], first) and np.array_equal(bins[-1], last)          # q = 0 / q = 1: the occupied ends
    assert np.abs(vals[0] - (lo + w * first)).max() <= H.quantile_bound(lo, hi)
    assert np.abs(vals[-1] - (lo + w * (last + 1))).max() <= H.quantile_bound(lo, hi)
    assert np.all(np.diff(vals, axis=0) >= -H.quantile_bound(lo, hi))                 # monotone in q
    assert np.all(counts[np.arange(len(counts))[None, :], bins] > 0)                  # never an empty bin
    # the numpy helper of the package states the same definition
    hv = sampler.histQuantiles((N, counts, (nbins, lo, hi), np.arange(len(counts))), QS)
    assert np.abs(hv - rv).max() <= H.quantile_bound(lo, hi)


def test_quantile_item_on_a_single_sample_and_a_one_bin_row():
    lo, hi = -3.0, 5.0
    counts = np.zeros((1, 16), dtype=np.int64); counts[0, 5] = 1                      # a single sample
    vals, bins = E.quantiles(counts, 1, lo, hi, QS)
    rv, rb = H.quantiles(counts, 1, lo, hi, QS)
    assert np.all(bins == 5) and np.array_equal(bins, rb) and np.abs(vals - rv).max() <= H.quantile_bound(lo, hi)
    assert np.abs(vals[:, 0] - (lo + 0.5 * (5 + np.array(QS)))).max() <= H.quantile_bound(lo, hi)      # linear inside the bin
    one = np.array([[12]])                                                            # one bin: the quantile walks from lo to hi
    vals, bins = E.quantiles(one, 12, lo, hi, QS)
    assert np.all(bins == 0) and np.abs(vals[:, 0] - (lo + (hi - lo) * np.array(QS))).max() <= H.quantile_bound(lo, hi)


# ---- the Python helpers ------------------------------------------------------------------------------------------------------------
def _brute_force_target(mesh, inv, y, z):
    """the active index of the earth cell whose centre is nearest in y, then in z; the lower index on a tie; None if it is not active"""
    yN = np.concatenate([[0.0], np.cumsum(mesh.yLen)]) - mesh.origin[0]
    zN = np.concatenate([[0.0], np.cumsum(mesh.zLen)]) - mesh.origin[1]
    ny, nz, nair = len(mesh.yLen), len(mesh.zLen), len(mesh.airLayer)
    best = None
    for iz in range(nair, nz):
        for iy in range(ny):
            key = (abs(0.5 * (yN[iy] + yN[iy + 1]) - y), abs(0.5 * (zN[iz] + zN[iz + 1]) - z), iz * ny + iy)
            if best is None or key[:2] < best[:2]:
                best = key
    hit = np.flatnonzero(np.asarray(inv.activeIdx) == best[2])
    return int(hit[0]) if len(hit) else None


def test_site_targets_against_brute_force_on_a_ragged_active_set():
    mesh, data, inv, _ = ragged_problem(23, 17, 3, 3, 3, 4)
    ny, nair = len(mesh.yLen), len(mesh.airLayer)
    assert len(inv.activeIdx) == 390 < ny * (len(mesh.zLen) - nair)                   # one earth cell is fixed
    yN = np.concatenate([[0.0], np.cumsum(mesh.yLen)]) - mesh.origin[0]
    zN = np.concatenate([[0.0], np.cumsum(mesh.zLen)]) - mesh.origin[1]
    yC, zC = 0.5 * (yN[:-1] + yN[1:]), 0.5 * (zN[:-1] + zN[1:])
    # a tie in y: the node between two cells of equal width is as far from one centre as from the other
    j = next(i for i in range(8, ny - 1) if mesh.yLen[i] == mesh.yLen[i + 1] and abs(yC[i] - yN[i + 1]) == abs(yC[i + 1] - yN[i + 1]))
    ys = np.array([yN[j + 1], yC[2] + 1.0, yC[ny - 1] + 5e4, -350.0, 133.7])
    zs = np.array([zN[nair] - 200.0, zC[nair + 1], zC[nair + 3] + 3.0, zN[-1] + 1e4])   # the first one lies in the air
    assert zs[0] < zN[nair] and 5 not in [int(np.argmin(np.abs(yC - y))) for y in ys]
    got = sampler.sitePPDTargets(mesh, inv, ys, zs)
    assert got.dtype == np.int64 and got.shape == (len(ys) * len(zs),)
    ref = [_brute_force_target(mesh, inv, y, z) for y in ys for z in zs]              # depth fastest
    assert got.tolist() == ref
    cells = np.asarray(inv.activeIdx)[got].reshape(len(ys), len(zs))
    assert np.all(cells[0] % ny == j)                                                 # the tie went to the lower index
    assert np.all(cells[:, 0] // ny == nair) and np.all(cells[:, -1] // ny == len(mesh.zLen) - 1)    # air -> first earth row; below -> last
    # the fixed cell (first earth row, column 5) is named
    assert _brute_force_target(mesh, inv, yC[5], zC[nair]) is None
    with pytest.raises(ValueError, match="not active") as e:
        sampler.sitePPDTargets(mesh, inv, [yC[0], yC[5]], [zC[nair + 1], zC[nair]])
    assert "%g" % yC[5] in str(e.value) and "%g" % zC[nair] in str(e.value)


def _hist(rng, nt=6, nbins=10, N=40, lo=-9.0, hi=0.0, targets=None):
    counts = np.array([rng.multinomial(N, rng.dirichlet(np.ones(nbins))) for _ in range(nt)]).astype(np.uint32)
    return N, counts, (nbins, lo, hi), np.arange(nt) if targets is None else targets


def test_merge_histograms_and_their_quantiles():
    rng = np.random.default_rng(5)
    a, b, c = _hist(rng), _hist(rng, N=25), _hist(rng, N=1)
    N, counts, bins, targets = sampler.mergeHistograms([a, b, c])
    assert N == 66 and bins == (10, -9.0, 0.0) and np.array_equal(targets, np.arange(6))
    assert np.array_equal(counts, a[1].astype(np.int64) + b[1] + c[1]) and np.all(counts.sum(axis=1) == N)
    big = (10 * 2 ** 31, np.full((6, 10), 2 ** 31, dtype=np.uint32), (10, -9.0, 0.0), np.arange(6))
    assert np.all(sampler.mergeHistograms([big, big, big])[1] == 3 * 2 ** 31)   # (the sum leaves uint32)
    hv = sampler.histQuantiles((N, counts, bins, targets), QS)
    rv, _ = H.quantiles(counts, N, -9.0, 0.0, QS)
    assert hv.shape == (len(QS), 6) and np.abs(hv - rv).max() <= H.quantile_bound(-9.0, 0.0)
    assert np.array_equal(sampler.mergeHistograms([a])[1], a[1])
    for other in (_hist(rng, nbins=11), _hist(rng, lo=-8.0), _hist(rng, hi=1.0), _hist(rng, targets=np.arange(6)[::-1]), _hist(rng, nt=5)):
        with pytest.raises(ValueError):
            sampler.mergeHistograms([a, other])
    with pytest.raises(ValueError):
        sampler.mergeHistograms([])
    with pytest.raises(ValueError):
        sampler.histQuantiles((0, a[1] * 0, a[2], a[3]), [0.5])
    with pytest.raises(ValueError):
        sampler.histQuantiles(a, [1.5])


def test_histogram_in_log10_resistivity():
    rng = np.random.default_rng(6)
    lo, hi = float(np.log(1e-4)), float(np.log(1.0))
    h = _hist(rng, nbins=8, lo=lo, hi=hi)
    edges, counts = sampler.histToLog10Rho(h)
    assert edges.shape == (9,) and np.all(np.diff(edges) > 0)
    assert abs(edges[0] - 0.0) < 1e-15 and abs(edges[-1] - 4.0) < 1e-14          # sigma 1 .. 1e-4 S/m = 1 .. 1e4 Ohm-m
    assert np.array_equal(counts, h[1][:, ::-1])
    # a value's bin in ln sigma is the mirrored bin of its log10 rho
    m = rng.uniform(lo, hi, 200)
    b = H.bin_of(m, 8, lo, hi)
    br = np.searchsorted(edges, -m / np.log(10.0), side="right") - 1
    inside = np.abs((m - lo) / (hi - lo) * 8 - np.round((m - lo) / (hi - lo) * 8)) > 1e-9
    assert np.array_equal(br[inside], 7 - b[inside])


def test_site_ppd_file_round_trip(tmp_path):
    rng = np.random.default_rng(7)
    ys, zs = np.array([-350.0, 0.0, 1234.5]), np.array([50.0, 500.0, 5000.0, 12345.0])
    lo, hi = float(np.log(1e-4)), 0.0
    h = _hist(rng, nt=12, nbins=300, N=99999, lo=lo, hi=hi)
    path = str(tmp_path / "sitePPD.dat")
    fileio.writeSitePPD(path, ys, zs, h)
    y, z, edges, counts = fileio.readSitePPD(path)
    e0, c0 = sampler.histToLog10Rho(h)
    assert np.array_equal(y, ys) and np.array_equal(z, zs)
    assert edges.shape == (301,) and np.abs(edges - e0).max() <= 5e-6 * np.abs(e0).max()      # %6g
    assert counts.shape == (3, 4, 300) and np.array_equal(counts.reshape(12, 300), c0)
    lines = open(path).read().split("\n")
    assert lines[0] == "y coordinate:     3" and lines[2] == "z coordinate:     4" and lines[4] == "log10 rho edges:   301"
    assert lines[6 + 4] == "" and lines[6 + 9] == "" and len(lines[6]) == 6 * 300       # a blank line behind every site; %5d and a blank
    with pytest.raises(ValueError):
        fileio.writeSitePPD(path, ys, zs[:3], h)


def test_quantile_models_need_an_all_cells_histogram(tmp_path):
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    rng = np.random.default_rng(8)
    h = _hist(rng, nt=n, nbins=30, N=50, lo=float(np.log(1e-4)), hi=0.0)
    models = fileio.getPosteriorQuantileModels(h, [0.05, 0.5, 0.95], copy.deepcopy(mesh), inv, outdir=str(tmp_path))
    assert models.shape == (3, n) and np.all(np.diff(models, axis=0) >= 0)
    assert sorted(os.listdir(tmp_path)) == ["p05Model.model", "p50Model.model", "p95Model.model"]
    back = fileio.readEMModel2D(str(tmp_path / "p50Model.model"))
    ref = inv.bgModel.copy(); ref[inv.activeIdx] += np.exp(models[1])
    assert np.abs(back.sigma - ref)[inv.activeIdx].max() <= 6e-3 * ref[inv.activeIdx].max()        # the model file prints %4.2e
    with pytest.raises(ValueError, match="every active cell"):
        fileio.getPosteriorQuantileModels((h[0], h[1][:5], h[2], np.arange(5)), [0.5], mesh, inv, write=False)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hmcmt.h")).read(), flags=re.S)
    protos = {m.group(1): [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
              for m in re.finditer(r"^\s*(?:extern\s+)?int\s+(hmcmt_chain_[a-z_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)}
    so = ctypes.CDLL(L.build_library())
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    ctype = {"hmcmt_ctx*": "Ptr{Cvoid}", "int64_t": "Int64", "int32_t": "Int32", "double": "Float64", "const int64_t*": "Ptr{Int64}",
             "int64_t*": "Ref{Int64}", "uint32_t*": "Ptr{UInt32}", "const double*": "Ptr{Float64}", "double*": "Ptr{Float64}"}
    expect = {"hmcmt_chain_hist_begin": ["hmcmt_ctx*", "int64_t", "const int64_t*", "int32_t", "double", "double"],
              "hmcmt_chain_hist": ["hmcmt_ctx*", "int64_t*", "uint32_t*", "int32_t"],
              "hmcmt_chain_hist_quantiles": ["hmcmt_ctx*", "int32_t", "const double*", "double*", "int32_t"],
              "hmcmt_chain_data_moments_begin": ["hmcmt_ctx*"],
              "hmcmt_chain_data_moments": ["hmcmt_ctx*", "int64_t*", "double*", "double*", "int32_t"]}
    for sym in NEW:
        assert sym in protos and sym in L.CHAIN_HIST_SYMBOLS and sym in L.PRODUCT_SYMBOLS and hasattr(so, sym)
        types = [p.rsplit(" ", 1)[0].strip() for p in protos[sym]]
        assert types == expect[sym], (sym, types)
        fn = getattr(L.load_library(), sym)
        assert len(fn.argtypes) == len(types) and fn.restype is ctypes.c_int
        m = re.search(r"@ccall libhmcmt\.%s\((.*?)\)::Cint" % sym, jl, flags=re.S)
        assert m, f"{sym} is not bound in julia/HMCMTHip.jl"
        assert re.findall(r"::\s*([A-Za-z0-9{}]+)", m.group(1)) == [ctype[t] for t in types], sym
    assert L.HIST_MAXBINS == E.maxbins() == 4096 and "nbins <= 4096" in open(os.path.join(ROOT, "include", "hmcmt.h")).read()
    assert "chain_hist!" in jl


# ---- the sampler on a stand-in context ---------------------------------------------------------------------------------------------
class OracleHistContext(OracleChainContext):
    """OracleChainContext plus the accumulators of the commit as the library runs them: a chain_begin ends them, a begin call counts
    the later commits behind the burn-in only; the histogram is the item functions' (tests/emul/emul_hist.cpp) over those commits,
    the data moments numpy's."""

    def chain_begin(self, *a, **kw):
        self.hist_from = self.dmom_from = None
        self.preds = []
        return super().chain_begin(*a, **kw)

    def chain_step(self, L, u, outputs=True):
        out = super().chain_step(L, u, outputs)
        self.preds.append(np.asarray(self.chain["pred"]).copy())
        return out

    def _seen(self, start):
        return max(start, self.chain["burnin"])

    def chain_hist_begin(self, targets, nbins, lo, hi):
        assert self.chain is not None and self.chain["p"] is None, "behind the begin, in front of the first momentum"
        self.hist_from, self.hist_args = len(self.chain["committed"]), (np.asarray(targets).copy(), int(nbins), float(lo), float(hi))
        self.hist_begins = getattr(self, "hist_begins", 0) + 1

    def chain_hist(self):
        assert self.hist_from is not None, "no histogram"
        post = np.array(self.chain["committed"][self._seen(self.hist_from):]).T
        return post.shape[1], E.accumulate(post, *self.hist_args)

    def chain_data_moments_begin(self):
        assert self.chain is not None and self.chain["p"] is None
        self.dmom_from = len(self.chain["committed"])

    def chain_data_moments(self):
        assert self.dmom_from is not None, "no data moments"
        post = np.array(self.preds[self._seen(self.dmom_from):]).T          # m2: real and imaginary parts apart, as the library holds them
        return post.shape[1], post.mean(axis=1), _moments(post.real)[2] + 1j * _moments(post.imag)[2]


def test_device_chain_loop_with_histogram_and_data_moments():
    """The keywords change neither draws nor decisions, the begin calls come behind the second chain_begin (which would end them) and in
    front of the first momentum, and the histogram is the one built from the kept samples."""
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    prior = HMCPrior(totalsamples=5, burninsamples=2, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0])
    lo, hi = float(np.log(1e-4)), 0.0
    run = lambda ctx, **kw: sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), copy.deepcopy(prior),
                                                  np.random.default_rng(21), ctx=ctx, device_chain=True, **kw)
    hm0, st0, hd0 = run(OracleChainContext(mesh, data, inv))
    assert st0.hist is None and st0.dataMoments is None and set(st0.acceptstats.tolist()) == {True, False}
    ctx = OracleHistContext(mesh, data, inv)
    hm1, st1, hd1 = run(ctx, hist={}, data_moments=True)
    assert np.array_equal(hm1, hm0) and np.array_equal(hd1, hd0) and np.array_equal(st1.hmstats, st0.hmstats)
    assert np.array_equal(st1.acceptstats, st0.acceptstats) and np.array_equal(st1.moments[1], st0.moments[1])
    count, counts, bins, targets = st1.hist
    assert count == 3 and bins == (300, lo, hi) and np.array_equal(targets, np.arange(n)) and ctx.hist_begins == 1
    kept = list(hm0[:, 2:].T)
    assert counts.shape == (n, 300) and np.array_equal(counts, H.counts_of(kept, targets, 300, lo, hi))
    assert np.all(counts.sum(axis=1) == 3)
    dc, dmean, dm2 = st1.dataMoments
    post = hd0[:, 3:]                                                # (column 0 is the start's)
    assert dc == 3 and np.allclose(dmean, post.mean(axis=1), rtol=1e-13, atol=0)
    dev = post - post.mean(axis=1, keepdims=True)
    assert np.allclose(dm2.real, (dev.real ** 2).sum(axis=1), rtol=1e-10, atol=0) and np.allclose(dm2.imag, (dev.imag ** 2).sum(axis=1), rtol=1e-10, atol=0)
    assert (dm2.real > 0).all()
    # chosen targets and bins, without the samples
    t2 = np.array([3, 3, n - 1, 0])
    hm2, st2, hd2 = run(OracleHistContext(mesh, data, inv), hist={"targets": t2, "nbins": 17, "lo": -6.0, "hi": -3.5}, keep_samples=False)
    assert hm2.shape == (n, 0) and st2.dataMoments is None and np.array_equal(st2.hmstats, st0.hmstats)
    assert st2.hist[2] == (17, -6.0, -3.5) and np.array_equal(st2.hist[3], t2)
    assert np.array_equal(st2.hist[1], H.counts_of(kept, t2, 17, -6.0, -3.5))
    # the files from the result
    q = fileio.getPosteriorQuantileModels(st1.hist, [0.05, 0.5, 0.95], mesh, inv, write=False)
    assert np.abs(q - H.quantiles(counts, 3, lo, hi, [0.05, 0.5, 0.95])[0]).max() <= H.quantile_bound(lo, hi)
    assert np.all(q[0] <= np.min(kept, axis=0) + (hi - lo) / 300) and np.all(q[2] >= np.max(kept, axis=0) - (hi - lo) / 300)
    with pytest.raises(ValueError, match="device_chain"):
        sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(1), ctx=OracleChainContext(mesh, data, inv), hist={})
    with pytest.raises(ValueError, match="no key"):
        run(OracleHistContext(mesh, data, inv), hist={"bins": 3})
