"""Effective sample size from the device chain, without a GPU: the autocovariance items of hmcmt_items.h on the host
(tests/emul/emul_acov.cpp) against tests/acov_ref.py, the numpy restatements of sampler.py and fileio.py, the ABI of the three new
symbols, and runHMCSampler(device_chain=True, ess=...) on an oracle-backed stand-in context."""
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
from tests import acov_ref as R
from tests.emul import emul_acov_py as E
from tests.helpers import make_problem
from tests.test_chain_host import OracleChainContext

NEW = ["hmcmt_chain_acov_begin", "hmcmt_chain_acov", "hmcmt_chain_ess"]
NS = [1, 2, 3, 7, 8, 9, 40]
KS = [1, 3, 7, 8, 70]


def planted(N, seed=0, nt=24):
    """AR(1) cells around ln sigma = -4 with a repeated sample (a rejection) planted, one constant cell"""
    rng = np.random.default_rng(1000 * seed + N)
    x = R.ar1(rng, rng.uniform(-0.3, 0.9, nt), N)
    if N > 3:
        x[:, 3] = x[:, 2]
    x[5, :] = x[5, 0]
    return x


# ---- the items against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_streamed_state_and_lagged_sums(N, K):
    """x0, tot, H_k and the ring are single subtractions and serial adds: equality.  S_k within (N + 4) 2^-53 sum |y_t y_{t-k}|:
    the fma chain's roundings plus the reference's products.  N <= K and N = K + 1 are among the cases."""
    x = planted(N)
    ref = R.streamed_state(x, K)
    for targets in (None, np.array([5, 5, 23, 0]), np.array([7])):
        got = E.accumulate(x, targets, K)
        sel = slice(None) if targets is None else targets
        for key in ("x0", "tot"):
            assert np.array_equal(got[key], ref[key][sel]), key
        for key in ("H", "ring"):
            assert np.array_equal(got[key], ref[key][:, sel]), key
        bound = R.s_bound(ref)[:, sel]
        assert np.all(np.abs(got["S"] - ref["S"][:, sel]) <= bound)
        assert np.all(got["S"][min(K, N - 1) + 1:] == 0.0)               # no lag beyond the samples
    assert np.all(E.accumulate(x, None, K)["S"][:, 5] == 0.0)            # the constant cell


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_read_out_against_the_formula_on_the_reference_sums(N, K):
    x = planted(N, seed=1)
    ref = R.streamed_state(x, K)
    mean_ref, acov_ref, cbound = R.readout(ref)
    mean, acov = E.readout(E.accumulate(x, None, K), N)
    assert np.all(np.abs(acov - acov_ref) <= cbound)
    assert np.all(acov[N:] == 0.0) and np.all(acov[:, 5] == 0.0)         # c_k = 0 for k >= N; a cell that never moved: exact zeros
    assert np.abs(mean - mean_ref).max() <= 4 * R.U * np.abs(mean_ref).max() and mean[5] == x[5, 0]
    if N > 1:
        assert np.all(acov[0, np.arange(len(x)) != 5] > 0)


@pytest.mark.parametrize("K", KS + [63])
@pytest.mark.parametrize("N", NS + [200, 500])
def test_the_streamed_form_is_the_two_pass_estimator(N, K):
    """the reference's streamed read-out against its own two-pass estimator: the rule is the textbook one"""
    x = planted(N, seed=2)
    _, acov, _ = R.readout(R.streamed_state(x, K))
    two = R.two_pass(x, K)
    assert np.all(np.abs(acov - two) <= 1e-13 * two[0][None, :])
    assert np.abs(sampler.acovOf(x, K) - two).max() <= 1e-13 * two[0].max()


# ---- tau, ess, window --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(22, 7), (200, 63), (200, 8)])
def test_tau_ess_window_on_planted_ar1_cells(N, K):
    """390 AR(1) cells, phi uniform in [-0.3, 0.9]: window equal, tau within the bound that follows from the bounds of c_k through
    Gamma_m, doubled; a cell is left out only if some reference |Gamma_m| up to its stop is below 1e-9, at most 1 % of them."""
    rng = np.random.default_rng(390 + N + K)
    x = R.ar1(rng, rng.uniform(-0.3, 0.9, 390), N)
    ref = R.streamed_state(x, K)
    _, acov_ref, cbound = R.readout(ref)
    tau_ref, ess_ref, win_ref, gammas = R.geyer(acov_ref, N)
    _, acov = E.readout(E.accumulate(x, None, K), N)
    tau, ess, win = E.ess(acov, N)
    keep = R.tie_free(gammas)
    left_out = int((~keep).sum())
    smallest = min(abs(G) for g in gammas for G in g)
    print(f"\n[N {N}, K {K}] left out {left_out} of 390; smallest |Gamma_m| {smallest:.3g}; "
          f"largest tau error over its bound {np.max(np.abs(tau - tau_ref)[keep] / R.tau_bound(acov_ref, cbound, gammas)[keep]):.3g}")
    assert left_out <= 3, f"{left_out} cells left out"
    assert np.array_equal(win[keep], win_ref[keep])
    assert np.all(np.abs(tau - tau_ref)[keep] <= R.tau_bound(acov_ref, cbound, gammas)[keep])
    # ess = N / tau under the cap: its error follows tau's
    rel = R.tau_bound(acov_ref, cbound, gammas) / np.abs(tau_ref) + 4 * R.U
    assert np.all(np.abs(ess - ess_ref)[keep] <= (rel * ess_ref)[keep] + 8 * R.U * ess_ref[keep])
    assert (win < 0).any() or K > 8                                      # a short window runs out of lags for the slow cells
    # the numpy restatement of the package states the same rule
    t2, e2, w2 = sampler.essFromAcov(acov, N)
    assert np.array_equal(w2, win) and np.allclose(t2, tau, rtol=1e-13, atol=0) and np.allclose(e2, ess, rtol=1e-13, atol=0)


def test_planted_constant_antithetic_and_slow_cells():
    N, K = 400, 7
    rng = np.random.default_rng(7)
    x = R.ar1(rng, np.array([0.5, -0.95, 0.995]), N)
    x[0, :] = -4.25                                                      # a constant cell
    _, acov = E.readout(E.accumulate(x, None, K), N)
    tau, ess, win = E.ess(acov, N)
    lg = np.log10(N)
    assert tau[0] == N and ess[0] == 1.0 and win[0] == 0 and np.all(acov[:, 0] == 0.0)
    assert tau[1] < 1.0 / lg and abs(ess[1] - N * lg) <= 4 * R.U * N * lg          # antithetic: the cap, tau reported raw
    assert win[2] == -4 and tau[2] > 6 and abs(ess[2] - N / tau[2]) <= 4 * R.U * N   # slowly mixing, K too small: the lags ran out
    t_ref, e_ref, w_ref, _ = R.geyer(R.readout(R.streamed_state(x, K))[1], N)
    assert np.array_equal(w_ref, win) and np.allclose(t_ref, tau, rtol=1e-12) and np.allclose(e_ref, ess, rtol=1e-12)
    # a single sample is a constant cell; two samples have one pair
    _, a1 = E.readout(E.accumulate(x[:, :1], None, K), 1)
    t1, e1, w1 = E.ess(a1, 1)
    assert np.all(t1 == 1.0) and np.all(e1 == 1.0) and np.all(w1 == 0)
    _, a2 = E.readout(E.accumulate(x[:, :2], None, K), 2)
    t2, e2, w2 = E.ess(a2, 2)
    assert np.all(np.abs(w2[1:]) <= 1) and t2[0] == 2.0


# ---- the numpy restatements --------------------------------------------------------------------------------------------------------
def _ess_stats(x, K, targets=None):
    N = x.shape[1]
    acov = sampler.acovOf(x, K)
    tau, ess, window = sampler.essFromAcov(acov, N)
    return {"count": N, "maxlag": K, "targets": np.arange(len(x)) if targets is None else targets, "mean": x.mean(axis=1),
            "acov": acov, "tau": tau, "ess": ess, "window": window}


def test_numpy_restatements_against_the_reference_on_four_chains():
    rng = np.random.default_rng(11)
    phi = rng.uniform(-0.3, 0.9, 30)
    N, K = 300, 40
    chains = [R.ar1(rng, phi, N, offset=-4.0 + 0.02 * c) for c in range(4)]
    for x in chains:
        acov = sampler.acovOf(x, K)
        two = R.two_pass(x, K)
        assert acov.shape == (K + 1, 30) and np.abs(acov - two).max() <= 1e-13 * two[0].max()
        assert np.array_equal(sampler.acovOf(x[3], K), acov[:, 3])       # a single chain: a vector
        t, e, w, _ = R.geyer(acov, N)
        t1, e1, w1 = sampler.essFromAcov(acov, N)
        assert np.array_equal(w, w1) and np.allclose(t, t1, rtol=1e-13, atol=0) and np.allclose(e, e1, rtol=1e-13, atol=0)
        ts, es, ws = sampler.essFromAcov(acov[:, 3], N)
        assert (ts, es, ws) == (t1[3], e1[3], w1[3])
    merged = sampler.mergeAcov([_ess_stats(x, K) for x in chains])
    tau, ess, window, rho = R.multi_chain(chains, K)
    assert merged["count"] == 4 * N and merged["nchains"] == 4 and merged["maxlag"] == K
    assert np.allclose(merged["rho"], rho, rtol=0, atol=1e-12)
    tied = np.array([np.min(np.abs(rho[0:K:2, j] + rho[1:K + 1:2, j])) < 1e-9 for j in range(30)])
    assert not tied.any()
    assert np.array_equal(merged["window"], window) and np.allclose(merged["tau"], tau, rtol=0, atol=1e-10)
    assert np.allclose(merged["ess"], ess, rtol=1e-10, atol=0)
    assert np.all(merged["ess"] <= 4 * N * np.log10(4 * N) * (1 + 1e-15))
    one = sampler.mergeAcov([_ess_stats(chains[0], K)])                   # one chain: B = 0
    t0, e0, w0, _ = R.multi_chain(chains[:1], K)
    assert np.array_equal(one["window"], w0) and np.allclose(one["tau"], t0, rtol=0, atol=1e-10) and one["count"] == N
    for other in (_ess_stats(chains[1][:, :-1], K), _ess_stats(chains[1], K - 1), _ess_stats(chains[1], K, np.arange(30)[::-1])):
        with pytest.raises(ValueError):
            sampler.mergeAcov([_ess_stats(chains[0], K), other])
    with pytest.raises(ValueError):
        sampler.mergeAcov([])
    with pytest.raises(ValueError):
        sampler.acovOf(np.zeros((3, 0)), 4)
    with pytest.raises(ValueError):
        sampler.essFromAcov(np.zeros((3, 4)), 0)


def test_mcse_of_the_mean():
    rng = np.random.default_rng(12)
    x = R.ar1(rng, np.array([0.0, 0.6, 0.9, 0.3]), 2000)
    moments = (x.shape[1], x.mean(axis=1), ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(axis=1))
    st = _ess_stats(x[[2, 0]], 63, targets=np.array([2, 0]))
    se = sampler.mcseOfMean(st, moments)
    assert se.shape == (2,) and np.allclose(se, np.sqrt(x.var(axis=1)[[2, 0]] / st["ess"]), rtol=1e-14, atol=0)
    # the white-noise cell: sd / sqrt(N) within the estimator's scatter; the slow one is several times worse
    assert 0.7 < se[1] / (x[0].std() / np.sqrt(2000)) < 1.4 and se[0] > 2.5 * se[1]


def test_ess_model_round_trip(tmp_path):
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    rng = np.random.default_rng(13)
    st = _ess_stats(R.ar1(rng, rng.uniform(-0.3, 0.9, n), 120), 20)
    path = str(tmp_path / "essModel.model")
    ess = fileio.getESSModel(path, st, copy.deepcopy(mesh), inv)
    assert np.array_equal(ess, st["ess"]) and os.listdir(tmp_path) == ["essModel.model"]
    back = fileio.readEMModel2D(path)
    ref = inv.bgModel.copy(); ref[inv.activeIdx] += ess
    assert np.abs(back.sigma - ref)[inv.activeIdx].max() <= 6e-3 * ref[inv.activeIdx].max()         # the model file prints %4.2e
    with pytest.raises(ValueError, match="every active cell"):
        fileio.getESSModel(path, _ess_stats(R.ar1(rng, np.full(5, 0.5), 50), 20), mesh, inv, write=False)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "hmcmt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = {m.group(1): [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
              for m in re.finditer(r"^\s*(?:extern\s+)?int\s+(hmcmt_chain_[a-z_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)}
    so = ctypes.CDLL(L.build_library())
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    ctype = {"hmcmt_ctx*": "Ptr{Cvoid}", "int64_t": "Int64", "int32_t": "Int32", "const int64_t*": "Ptr{Int64}", "int64_t*": "Ref{Int64}",
             "double*": "Ptr{Float64}", "int32_t*": "Ptr{Int32}"}
    expect = {"hmcmt_chain_acov_begin": ["hmcmt_ctx*", "int64_t", "const int64_t*", "int32_t"],
              "hmcmt_chain_acov": ["hmcmt_ctx*", "int64_t*", "double*", "double*", "int32_t"],
              "hmcmt_chain_ess": ["hmcmt_ctx*", "double*", "double*", "int32_t*", "int32_t"]}
    for sym in NEW:
        assert sym in protos and sym in L.CHAIN_ACOV_SYMBOLS and sym in L.PRODUCT_SYMBOLS and hasattr(so, sym)
        types = [p.rsplit(" ", 1)[0].strip() for p in protos[sym]]
        assert types == expect[sym], (sym, types)
        fn = getattr(L.load_library(), sym)
        assert len(fn.argtypes) == len(types) and fn.restype is ctypes.c_int
        m = re.search(r"@ccall libhmcmt\.%s\((.*?)\)::Cint" % sym, jl, flags=re.S)
        assert m, f"{sym} is not bound in julia/HMCMTHip.jl"
        assert re.findall(r"::\s*([A-Za-z0-9{}]+)", m.group(1)) == [ctype[t] for t in types], sym
    assert L.ACOV_MAXLAG == E.maxlag() == 1023 and "maxlag <= 1023" in header
    exported = re.search(r"^export (.*?)\n\n", jl, flags=re.S | re.M).group(1)
    for name in ("chainAcovBegin!", "chainAcov", "chainEss", "chain_ess!"):
        assert name in exported and ("function " + name) in jl


def test_argument_validation_without_a_context():
    lib = L.load_library()
    t = np.zeros(1, dtype=np.int64)
    assert lib.hmcmt_chain_acov_begin(None, 1, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 8) == -1
    assert lib.hmcmt_chain_acov(None, None, None, None, 0) == -1
    assert lib.hmcmt_chain_ess(None, None, None, None, 0) == -1
    assert lib.hmcmt_debug_chain_acov_time(None, -1, None, None) == -1 and "hmcmt_debug_chain_acov_time" in L.DEBUG_SYMBOLS


# ---- the sampler on a stand-in context ---------------------------------------------------------------------------------------------
class OracleAcovContext(OracleChainContext):
    """OracleChainContext plus the autocovariance accumulator as the library runs it: a chain_begin ends it, a begin call counts the
    later commits behind the burn-in only; state and results are the item functions' (tests/emul/emul_acov.cpp) over those commits."""

    def chain_begin(self, *a, **kw):
        self.acov_from = None
        return super().chain_begin(*a, **kw)

    def chain_acov_begin(self, targets=None, maxlag=63):
        assert self.chain is not None and self.chain["p"] is None, "behind the begin, in front of the first momentum"
        self.acov_from, self.acov_args = len(self.chain["committed"]), (None if targets is None else np.asarray(targets).copy(), int(maxlag))
        self.acov_begins = getattr(self, "acov_begins", 0) + 1

    def chain_moments(self):
        if len(self.chain["committed"]) <= self.chain["burnin"]:            # (no sample yet: the library's zeroed moments)
            n = len(self.chain["m"])
            return 0, np.zeros(n), np.zeros(n)
        return super().chain_moments()

    def chain_acov_count(self):
        assert self.acov_from is not None, "no autocovariances"
        return len(self.chain["committed"][max(self.acov_from, self.chain["burnin"]):])

    def _acov(self):
        assert self.chain_acov_count() > 0, "the read-outs need a commit (HMCMT_EINVAL)"
        post = np.array(self.chain["committed"][max(self.acov_from, self.chain["burnin"]):]).T
        return post.shape[1], E.readout(E.accumulate(post, *self.acov_args), post.shape[1])

    def chain_acov(self):
        n, (mean, acov) = self._acov()
        return n, mean, acov

    def chain_ess(self):
        n, (_, acov) = self._acov()
        return E.ess(acov, n)


def test_device_chain_loop_with_ess():
    """The keyword changes neither draws nor records, the begin call comes behind the second chain_begin (which would end the
    accumulator) and in front of the first momentum, and the result is the estimator of the kept samples."""
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    prior = HMCPrior(totalsamples=7, burninsamples=2, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0])
    run = lambda ctx, **kw: sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), copy.deepcopy(prior),
                                                  np.random.default_rng(21), ctx=ctx, device_chain=True, **kw)
    hm0, st0, hd0 = run(OracleChainContext(mesh, data, inv))
    assert st0.ess is None and set(st0.acceptstats.tolist()) == {True, False}
    ctx = OracleAcovContext(mesh, data, inv)
    hm1, st1, hd1 = run(ctx, ess={"maxlag": 3}, keep_samples=False)
    assert hm1.shape == (n, 0) and np.array_equal(st1.hmstats, st0.hmstats) and np.array_equal(st1.acceptstats, st0.acceptstats)
    assert np.array_equal(st1.moments[1], st0.moments[1]) and ctx.acov_begins == 1
    e = st1.ess
    assert set(e) == {"count", "maxlag", "targets", "mean", "acov", "tau", "ess", "window", "misfit"}
    assert e["count"] == 5 and e["maxlag"] == 3 and np.array_equal(e["targets"], np.arange(n))
    kept = hm0[:, 2:]
    two = R.two_pass(kept, 3)
    assert e["acov"].shape == (4, n) and np.abs(e["acov"] - two).max() <= 1e-12 * two[0].max()
    assert np.abs(e["mean"] - kept.mean(axis=1)).max() <= 1e-14 * np.abs(kept).max()
    t, es, w, _ = R.geyer(e["acov"], 5)
    assert np.array_equal(e["window"], w) and np.allclose(e["tau"], t, rtol=1e-12) and np.allclose(e["ess"], es, rtol=1e-12)
    D = st0.hmstats[0, 3:]
    assert e["misfit"]["count"] == 5 and np.abs(e["misfit"]["acov"] - R.two_pass(D[None, :], 3)[:, 0]).max() <= 1e-12 * D.var()
    assert e["misfit"]["tau"] == sampler.essFromAcov(e["misfit"]["acov"], 5)[0]
    se = sampler.mcseOfMean(e, st1.moments)
    assert se.shape == (n,) and np.all(np.isfinite(se))
    # chosen targets, with the samples kept: the same draws
    t2 = np.array([3, 3, n - 1, 0])
    hm2, st2, hd2 = run(OracleAcovContext(mesh, data, inv), ess={"targets": t2, "maxlag": 70})
    assert np.array_equal(hm2, hm0) and np.array_equal(hd2, hd0) and np.array_equal(st2.hmstats, st0.hmstats)
    assert st2.ess["acov"].shape == (71, 4) and np.array_equal(st2.ess["targets"], t2) and np.all(st2.ess["acov"][5:] == 0.0)
    assert np.array_equal(st2.ess["acov"][:, 0], st2.ess["acov"][:, 1])
    assert np.abs(st2.ess["acov"][:4] - two[:, t2]).max() <= 1e-12 * two[0].max()
    with pytest.raises(ValueError, match="device_chain"):
        sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(1), ctx=OracleChainContext(mesh, data, inv), ess={})
    # an unknown key is refused before the context is touched and before the first draw
    ctx, rng = OracleAcovContext(mesh, data, inv), np.random.default_rng(4)
    state = copy.deepcopy(rng.bit_generator.state)
    with pytest.raises(ValueError, match="no key"):
        sampler.runHMCSampler(mesh, data, inv, prior, rng, ctx=ctx, device_chain=True, ess={"lags": 3})
    assert rng.bit_generator.state == state and getattr(ctx, "chain", None) is None and not hasattr(ctx, "acov_begins")
    with pytest.raises(ValueError, match="no key"):
        sampler.runHMCSampler(mesh, data, inv, prior, rng, ctx=ctx, device_chain=True, hist={"bins": 3})
    assert rng.bit_generator.state == state and getattr(ctx, "chain", None) is None


def test_a_chain_that_ends_inside_its_burn_in_keeps_its_other_results():
    """no commit is counted, the read-outs of the library would refuse: the sampler asks for the count first"""
    mesh, data, inv, _ = make_problem("tiny")
    prior = HMCPrior(totalsamples=3, burninsamples=3, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0])
    run = lambda ctx, **kw: sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), copy.deepcopy(prior),
                                                  np.random.default_rng(21), ctx=ctx, device_chain=True, **kw)
    _, st0, _ = run(OracleAcovContext(mesh, data, inv))
    _, st1, _ = run(OracleAcovContext(mesh, data, inv), ess={})
    assert np.array_equal(st1.hmstats, st0.hmstats) and np.array_equal(st1.acceptstats, st0.acceptstats)
    e = st1.ess
    assert e["count"] == 0 and e["maxlag"] == 63 and len(e["targets"]) == len(inv.strModel)
    assert all(e[k] is None for k in ("mean", "acov", "tau", "ess", "window", "misfit"))


def test_parallel_sampler_passes_ess_through_and_keeps_each_local_chains_result():
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    prior = HMCPrior(totalsamples=7, burninsamples=2, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0])
    hm, hs, hd = sampler.parallelHMCSampler(mesh, data, inv, prior, nchains=2, seed=5, device_chain=True, ess={"maxlag": 3},
                                            context_factory=lambda m, d, i, dev: OracleAcovContext(m, d, i))
    assert len(hs) == 2 and all(st.ess is not None and st.ess["count"] == 5 and st.ess["acov"].shape == (4, n) for st in hs)
    for c in range(2):
        two = R.two_pass(hm[c][:, 2:], 3)
        assert np.abs(hs[c].ess["acov"] - two).max() <= 1e-12 * two[0].max()
    assert not np.array_equal(hs[0].ess["acov"], hs[1].ess["acov"])       # (two chains, two streams)
    merged = sampler.mergeAcov([st.ess for st in hs])
    tau, ess, window, _ = R.multi_chain([hm[c][:, 2:] for c in range(2)], 3)
    assert merged["count"] == 10 and np.array_equal(merged["window"], window) and np.allclose(merged["ess"], ess, rtol=1e-9, atol=0)
