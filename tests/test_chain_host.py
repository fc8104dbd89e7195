"""The device-resident HMC chain without a GPU: the item functions of kernels_chain.h on the host (tests/emul/emul_chain.cpp)
against numpy, the moment algebra of sampler.py, the moments-based posterior files, the ABI of the six hmcmt_chain_* symbols,
and runHMCSampler(device_chain=True) on an oracle-backed stand-in context (which pins the order of the random draws)."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from hmcmt2d_amd import fileio, sampler
from hmcmt2d_amd import lib as L
from hmcmt2d_amd.structs import HMCParameter, HMCPrior
from tests.conftest import ROOT
from tests import chain_ref as R
from tests.emul import emul_chain_py as E
from tests.helpers import OracleContext, make_problem

EPS = np.finfo(float).eps
NB, NT = 64, 256
# either side of a 128- and a 256-thread workgroup, of one round of the NB workgroups, and a few rounds
SIZES = [1, 127, 128, 129, 255, 256, 257, 1000, NB * NT - 1, NB * NT + 1, 3 * NB * NT + 77]


def test_layout_is_the_leapfrog_kernels():
    assert E.layout() == (NB, NT)
    src = open(os.path.join(ROOT, "hmcmt2d_amd", "csrc", "kernels_path.h")).read()
    assert re.search(r"constexpr int LFNB = (\d+);", src).group(1) == str(NB)


@pytest.mark.parametrize("n", SIZES)
def test_momentum_item_against_numpy(n):
    """p = sqrtM * clip(z, +-2.5) with the diagonal mass of setMassMatrix(nparam, scaling) (invM = 1 / mass, sqrtM = sqrt(mass)), values
    beyond the clip present.  Bound: the item divides by sqrt(invM), numpy multiplies by sqrt(mass) -- 1 / mass, two square roots, a
    division and a product, each correctly rounded: 4 eps relative covers them."""
    rng = np.random.default_rng(n)
    z = 2.0 * rng.standard_normal(n)
    z[0] = 7.5                                            # (beyond the clip whatever the draw)
    if n > 1:
        z[-1] = -3.25
    mass = rng.uniform(0.5, 4.0, n)
    invM, sqrtM = 1.0 / mass, np.sqrt(mass)
    p, K = E.momentum(z, invM)
    ref = sqrtM * np.clip(z, -2.5, 2.5)
    assert np.abs(z).max() > 2.5 and np.abs(np.clip(z, -2.5, 2.5)).max() == 2.5
    assert np.abs(p - ref).max() <= 4 * EPS * np.abs(ref).max()
    assert np.array_equal(E.clip(z), np.clip(z, -2.5, 2.5))
    # the two-stage kinetic energy, fused with the momentum and on its own (diagonal, and with x = M^-1 p given)
    Kref = 0.5 * p @ (invM * p)
    for val in (K, E.kinetic(p, invM=invM), E.kinetic(p, x=invM * p)):
        assert abs(val - Kref) <= 1e-14 * Kref


def _ensemble(rng, nparam=37, nsamples=12):
    """12 'samples' as a chain leaves them: a rejection repeats the current model"""
    ens = np.empty((nparam, nsamples))
    cur = -4.0 + rng.standard_normal(nparam)
    for s in range(nsamples):
        if s in (0, 2, 3, 7) or rng.random() < 0.5:
            cur = cur + 0.3 * rng.standard_normal(nparam)
        ens[:, s] = cur
    assert any(np.array_equal(ens[:, s], ens[:, s - 1]) for s in range(1, nsamples))
    return ens


def test_welford_item_against_two_pass_numpy():
    ens = _ensemble(np.random.default_rng(3))
    count, mean, m2 = E.welford(ens, burnin=3)
    post = ens[:, 3:]
    assert count == 9 == post.shape[1]
    assert np.abs(mean - post.mean(axis=1)).max() <= 1e-14 * np.abs(post.mean(axis=1)).max()
    var = post.var(axis=1)
    assert np.all(np.abs(m2 / count - var) <= 1e-12 * var)
    # getPosteriorModel's E[x^2] - mean^2 cancels: it agrees to 64 eps max(mean^2 / var, 1) per cell, not to a fixed tolerance
    naive = (post ** 2).mean(axis=1) - post.mean(axis=1) ** 2
    bound = 64 * EPS * np.maximum(post.mean(axis=1) ** 2 / var, 1.0)
    assert np.all(np.abs(m2 / count - naive) <= bound * var)


def test_welford_cells_that_never_move_have_zero_m2():
    rng = np.random.default_rng(4)
    ens = _ensemble(rng)
    frozen = [0, 5, 36]
    ens[frozen, :] = np.array([-4.605170185988091, 0.1, -13.815510557964274])[:, None]
    count, mean, m2 = E.welford(ens, burnin=3)
    assert count == 9
    assert np.all(m2[frozen] == 0.0) and np.array_equal(mean[frozen], ens[frozen, 0])
    others = np.setdiff1d(np.arange(ens.shape[0]), frozen)
    assert np.all(m2[others] > 0)


def _moments(x):
    return x.shape[1], x.mean(axis=1), ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)


# ---- tests/chain_ref.py, the reference of tests/test_gpu_chain_kernels.py, against the item functions -------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_reference_against_the_item_functions(n):
    """chain_ref.momentum / kinetic / moments (longdouble sums) against the emulation, at the bounds of the tests above (the momentum
    per element); a non-unit mass, the clip's edge cases planted."""
    rng = np.random.default_rng(1000 + n)
    z = 2.0 * rng.standard_normal(n)
    z[0] = 7.5
    if n > 3:
        z[-1], z[1], z[2] = -3.25, 2.5, -0.0
    invM = rng.uniform(0.25, 4.0, n)
    p, K = E.momentum(z, invM)
    pr, Kr = R.momentum(z, invM)
    assert np.all(np.abs(p - pr) <= 4 * EPS * np.abs(pr))
    assert abs(K - Kr) <= 1e-14 * Kr
    x = invM * p
    assert abs(E.kinetic(p, invM=invM) - R.kinetic(p, invM=invM)) <= 1e-14 * Kr
    assert abs(E.kinetic(p, x=x) - R.kinetic(p, x=x)) <= 1e-14 * Kr
    assert abs(R.kinetic(p, invM=invM) - Kr) <= 4 * EPS * Kr        # (the rounded p: its own 1/2 ulp, twice)
    ens = _ensemble(rng, nparam=n)
    count, mean, m2 = E.welford(ens, burnin=3)
    cr, mr, m2r = R.moments(ens[:, 3:])
    bmean, bvar = R.moments_bounds(mr, m2r, cr)
    assert count == cr == 9
    assert np.abs(mean - mr).max() <= bmean
    assert np.all(np.abs(m2 / count - m2r / cr) <= bvar)


def test_reference_moments_of_a_chain_that_stands_still():
    ens = np.repeat(np.array([[-4.605170185988091], [0.1], [-13.815510557964274]]), 5, axis=1)
    count, mean, m2 = R.moments(ens)
    assert count == 5 and np.array_equal(mean, ens[:, 0]) and np.all(m2 == 0.0)


def test_reference_prior_term_and_misfit_against_numpy():
    mesh, data, inv, m = make_problem("tiny")
    n = len(m)
    rng = np.random.default_rng(8)
    mref = m + 0.1 * np.sin(np.arange(n) / 7.0)
    d = m - mref
    val, S = R.mnorm(m, mref, inv.Wm, 1.7)
    plain = 0.5 * float(d @ (inv.Wm @ d)) * 1.7
    nnz = int(np.diff(inv.Wm.tocsr().indptr).max())
    assert S >= abs(val) > 0 and abs(plain - val) <= (nnz + 8) * EPS * S
    assert R.mnorm(m, mref, inv.Wm.toarray(), 1.7) == (val, S)
    assert R.mnorm(mref, mref, inv.Wm, 1.7) == (0.0, 0.0)
    pred = inv.obsData * (1.0 + 0.05 * rng.standard_normal(len(inv.obsData))) + 1e-3j * rng.standard_normal(len(inv.obsData))
    ref = R.misfit(pred, inv)
    assert ref > 0 and abs(sampler.compDataMisfit(pred, inv) - ref) <= (np.log2(len(pred)) + 8) * EPS * ref   # (numpy sums pairwise)


def test_reference_decision_rule():
    # downhill: accepted whatever u; uphill: u against exp(hdif); the order of operations is hmcmt_chain_step's
    assert R.decision(10.0, 1.0, 2.0, 9.0, 2.0, 1.0, 0.999) == (1.0, True)
    h, acc = R.decision(10.0, 1.0, 2.0, 10.5, 2.0, 1.0, 0.5)
    assert h == -0.5 and acc and not R.decision(10.0, 1.0, 2.0, 10.5, 2.0, 1.0, 0.7)[1]
    assert R.decision(0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 0.5)[0] == (0.1 + 0.2 + 0.3) - 0.0
    assert R.decision(3.0 + 1e12, 1.0, 2.0, 5.0, 2.0, 1.0, 1.0)[1]                  # a forced acceptance
    assert R.decision(3.0 - 1e12, 1.0, 2.0, 5.0, 2.0, 1.0, 0.0) == ((3.0 - 1e12 + 1.0 + 2.0) - (5.0 + 2.0 + 1.0), False)   # and rejection


def test_merge_moments_of_unequal_splits():
    rng = np.random.default_rng(5)
    x = 3.0 + rng.standard_normal((23, 40)) * rng.uniform(0.1, 2.0, (23, 1))
    parts = [x[:, :7], x[:, 7:29], x[:, 29:]]
    n, mean, m2 = sampler.mergeMoments([_moments(p) for p in parts])
    n0, mean0, m20 = _moments(x)
    assert n == n0 == 40
    assert np.abs(mean - mean0).max() <= 1e-13 * np.abs(mean0).max()
    assert np.all(np.abs(m2 - m20) <= 1e-13 * m20)
    # an empty set is passed over; the Welford item's moments merge like numpy's
    n1, mean1, m21 = sampler.mergeMoments([(0, np.zeros(23), np.zeros(23)), E.welford(parts[0], 0), E.welford(x[:, 7:], 0)])
    assert n1 == 40 and np.abs(mean1 - mean0).max() <= 1e-13 * np.abs(mean0).max() and np.all(np.abs(m21 - m20) <= 1e-13 * m20)
    with pytest.raises(ValueError):
        sampler.mergeMoments([])


def test_gelman_rubin_against_the_textbook_formula():
    rng = np.random.default_rng(6)
    m, n, nparam = 4, 50, 11
    chains = [rng.standard_normal((nparam, n)) * (1 + 0.2 * j) + 0.5 * j * (np.arange(nparam)[:, None] % 3) for j in range(m)]
    rhat = sampler.gelmanRubin([_moments(c) for c in chains])
    means = np.stack([c.mean(axis=1) for c in chains])
    W = np.stack([c.var(axis=1, ddof=1) for c in chains]).mean(axis=0)
    B = n * means.var(axis=0, ddof=1)
    ref = np.sqrt(((n - 1) / n * W + B / n) / W)
    assert np.abs(rhat - ref).max() <= 1e-12 * ref.max()
    assert rhat[0] < 1.1 < rhat[1]                      # (cell 0: the chains share a mean; cell 1: they do not)
    with pytest.raises(ValueError):
        sampler.gelmanRubin([_moments(chains[0]), _moments(chains[1][:, :10])])


def _numbers(path):
    out = []
    for line in open(path):
        if line.startswith("#"):
            continue
        for tok in line.split():
            try:
                out.append(float(tok))
            except ValueError:
                pass
    return np.array(out)


def test_posterior_files_from_moments_equal_those_from_the_samples(tmp_path):
    mesh, data, inv, _ = make_problem("tiny")
    nparam = len(inv.strModel)
    ens = _ensemble(np.random.default_rng(7), nparam=nparam, nsamples=12)
    prior = HMCPrior(burninsamples=3, totalsamples=12)
    a, b = tmp_path / "samples", tmp_path / "moments"
    a.mkdir(); b.mkdir()
    mean0, std0 = fileio.getPosteriorModel(ens, copy.deepcopy(mesh), inv, prior, outdir=str(a))
    mean1, std1 = fileio.getPosteriorModelFromMoments(E.welford(ens, 3), copy.deepcopy(mesh), inv, outdir=str(b))
    assert np.abs(mean1 - mean0).max() <= 1e-14 * np.abs(mean0).max()
    for name in ("meanModel.model", "stdModel.model"):
        x, y = _numbers(a / name), _numbers(b / name)
        assert x.shape == y.shape and x.size > nparam
        text = open(a / name).read()
        digits = len(re.search(r"\d\.(\d+)[eE][-+]\d+", text).group(1))        # the files' printed precision
        assert np.all(np.abs(x - y) <= 10.0 ** -digits * np.abs(x) * 1.0001 + 0.0)
    with pytest.raises(ValueError):
        fileio.getPosteriorModelFromMoments((0, mean0, std0), mesh, inv, write=False)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
CHAIN = ["hmcmt_chain_begin", "hmcmt_chain_momentum", "hmcmt_chain_step", "hmcmt_chain_state", "hmcmt_chain_moments", "hmcmt_chain_end"]


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "hmcmt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
            for m in re.finditer(r"^\s*int\s+(hmcmt_chain_[a-z_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)}


def test_chain_symbols_are_declared_exported_and_bound():
    so = ctypes.CDLL(L.build_library())
    protos = _header_prototypes()
    EXTRA = ["hmcmt_chain_set_energy"]                  # (beside the six: the reference's start, a restored chain)
    assert sorted(protos) == sorted(CHAIN + EXTRA) == sorted(L.CHAIN_SYMBOLS)
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    for sym in CHAIN + EXTRA:
        assert sym in L.EXPORTED_SYMBOLS and hasattr(so, sym)
        nargs = len(protos[sym])
        assert len(getattr(L.load_library(), sym).argtypes) == nargs, sym
        m = re.search(r"ccall\(\(:%s, libhmcmt\), Cint,\s*\((.*?)\),\s*\n?\s*ctx" % sym, jl, flags=re.S)
        if m:
            types = [t for t in re.split(r",(?![^{]*\})", m.group(1)) if t.strip()]
        else:                                               # the @ccall form: value::Type pairs
            m = re.search(r"@ccall libhmcmt\.%s\((.*?)\)::Cint" % sym, jl, flags=re.S)
            assert m, f"{sym} is not bound in julia/HMCMTHip.jl"
            types = re.findall(r"::\s*([A-Za-z0-9{}]+)", m.group(1))
        assert len(types) == nargs, (sym, types, protos[sym])
    # hmcmt_chain_step's argument types, by hand: the record's pointer is the one type the other bindings do not have
    step = re.search(r"@ccall libhmcmt\.hmcmt_chain_step\((.*?)\)::Cint", jl, flags=re.S).group(1)
    assert re.findall(r"::\s*([A-Za-z0-9{}]+)", step) == ["Ptr{Cvoid}", "Int32", "Float64", "Ref{HmcmtChainRecord}", "Ptr{Float64}", "Ptr{ComplexF64}"]
    assert [p.split()[0] for p in protos["hmcmt_chain_step"]] == ["hmcmt_ctx*", "int32_t", "double", "hmcmt_chain_record*", "double*", "double*"]


def test_record_layout_in_c_python_and_julia(tmp_path):
    import subprocess
    fields = [f for f, _ in L.ChainRecord._fields_]
    src = tmp_path / "rec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmcmt.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(hmcmt_chain_record));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(hmcmt_chain_record, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "rec"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == ctypes.sizeof(L.ChainRecord) == 80
    assert out[1:] == [getattr(L.ChainRecord, f).offset for f in fields]
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    body = re.search(r"struct HmcmtChainRecord\b(.*?)\nend", jl, flags=re.S).group(1)
    jf = re.findall(r"^\s*([A-Za-z_0-9]+)::(\w+)", body, flags=re.M)
    ctype = {ctypes.c_int32: "Int32", ctypes.c_int64: "Int64", ctypes.c_double: "Float64"}
    assert jf == [(f, ctype[t]) for f, t in L.ChainRecord._fields_]


# ---- the sampler on a stand-in context ---------------------------------------------------------------------------------------------
class OracleChainContext(OracleContext):
    """OracleContext plus the chain_* methods of HipContext in numpy: the trajectory is sampler.proposeLeapfrog on the oracle's
    gradients, the Hamiltonian terms are getHamiltonian's expressions, the moments are numpy's over the committed samples."""

    def set_prior(self, mref, Wm, invM):
        self.mref, self.Wm, self.invM = np.asarray(mref, float).copy(), Wm, np.asarray(invM, float).copy()
        self.chain = None

    def _mnorm(self, m):
        d = m - self.mref
        return 0.5 * float(d @ (self.Wm @ d)) * self.prior.regParam

    def chain_begin(self, m_start, dt, regParam, lnSigMin, lnSigMax, burnin=0):
        self.prior = HMCPrior(dt=dt, regParam=regParam, sigBounds=[float(np.exp(lnSigMin)), float(np.exp(lnSigMax))])
        self.cinv = copy.deepcopy(self.inv)
        self.cinv.refModel = self.mref.copy()
        m = np.asarray(m_start, float).copy()
        pred, D = self.forward(m)
        self.chain = dict(m=m, pred=pred, D=D, M=self._mnorm(m), burnin=int(burnin), committed=[], p=None)
        return D, self.chain["M"]

    def chain_set_energy(self, D, M):
        self.chain.update(D=D, M=M)

    def chain_momentum(self, z):
        c = self.chain
        c["p"] = np.clip(z, -2.5, 2.5) / np.sqrt(self.invM)
        c["K0"] = 0.5 * float(np.dot(c["p"], self.invM * c["p"]))
        return c["K0"]

    def chain_step(self, L, u, outputs=True):
        c = self.chain
        assert c["p"] is not None, "no momentum since the last step"
        par = HMCParameter(len(c["m"]), c["m"].copy(), c["p"].copy(), self.invM, np.sqrt(1.0 / self.invM))
        n0 = self.ngrad
        m1, p1 = sampler.proposeLeapfrog(par, self.mesh, self.data, self.cinv, self.prior, None, int(L), self)
        _, pred1, D1 = self._cache
        K1 = 0.5 * float(np.dot(p1, self.invM * p1))
        M1 = self._mnorm(m1)
        hdif = (c["D"] + c["M"] + c["K0"]) - (D1 + K1 + M1)
        acc = hdif > 0 or u < np.exp(hdif)
        if acc:
            c.update(m=m1.copy(), pred=pred1, D=D1, M=M1)
        c["committed"].append(c["m"].copy())
        c["p"] = None
        rec = dict(accepted=int(acc), nfevals=self.ngrad - n0, K0=c["K0"], K1=K1, D1=D1, M1=M1, D=c["D"], M=c["M"], hdif=hdif,
                   nsamples=len(c["committed"]), nmoments=max(0, len(c["committed"]) - c["burnin"]))
        return rec, (c["m"].copy() if outputs else None), (c["pred"].copy() if outputs else None)

    def chain_state(self):
        return self.chain["m"].copy(), self.chain["p"], self.chain["pred"].copy()

    def chain_moments(self):
        post = np.array(self.chain["committed"][self.chain["burnin"]:]).T
        return _moments(post)


def test_device_chain_loop_draws_in_the_host_loops_order():
    """runHMCSampler(device_chain=True) on the stand-in gives the host loop's decisions, Hamiltonian terms and samples from the same
    seed: the draws are the first momentum, (rhoref,) then per sample L, u, the next momentum."""
    mesh, data, inv, _ = make_problem("tiny")
    prior = HMCPrior(totalsamples=5, burninsamples=2, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0])
    seen = set()
    for rhoref in (None, 80.0):
        p0, p1 = copy.deepcopy(prior), copy.deepcopy(prior)
        hm0, st0, hd0 = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), p0, np.random.default_rng(21), rhoref=rhoref,
                                              ctx=OracleContext(mesh, data, inv))
        ctx = OracleChainContext(mesh, data, inv)
        hm1, st1, hd1 = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), p1, np.random.default_rng(21), rhoref=rhoref,
                                              ctx=ctx, device_chain=True)
        assert st0.moments is None
        seen |= set(st0.acceptstats.tolist())
        assert np.array_equal(st1.acceptstats, st0.acceptstats) and (st1.nAccept, st1.nReject) == (st0.nAccept, st0.nReject)
        assert np.allclose(st1.hmstats, st0.hmstats, rtol=1e-13, atol=0)
        assert np.allclose(hm1, hm0, rtol=1e-13, atol=0) and np.allclose(hd1, hd0, rtol=1e-13, atol=0)
        count, mean, m2 = st1.moments
        assert count == 3 and np.allclose(mean, hm0[:, 2:].mean(axis=1), rtol=1e-13) and p1.nfevals == p0.nfevals
        # keep_samples=False: the same chain, nothing but the moments and the statistics come back
        p2 = copy.deepcopy(prior)
        hm2, st2, hd2 = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), p2, np.random.default_rng(21), rhoref=rhoref,
                                              ctx=OracleChainContext(mesh, data, inv), device_chain=True, keep_samples=False)
        assert hm2.shape == (hm0.shape[0], 0) and hd2.shape == (hd0.shape[0], 1) and np.array_equal(hd2[:, 0], hd1[:, 0])
        assert np.array_equal(st2.hmstats, st1.hmstats) and np.array_equal(st2.acceptstats, st1.acceptstats)
        assert st2.moments[0] == 3 and np.array_equal(st2.moments[1], mean) and np.array_equal(st2.moments[2], m2)
    assert seen == {True, False}                        # (both kinds of decision were compared)


def test_device_chain_refuses_checkpoints_and_keep_samples_needs_it(tmp_path):
    mesh, data, inv, _ = make_problem("tiny")
    prior = HMCPrior(totalsamples=2, burninsamples=0, dt=0.02, timestep=[1, 2], sigBounds=[1e-4, 1.0])
    with pytest.raises(ValueError, match="checkpoint"):
        sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(1), ctx=OracleChainContext(mesh, data, inv),
                              device_chain=True, checkpoint=str(tmp_path / "c.npz"), checkpoint_every=1)
    with pytest.raises(ValueError, match="keep_samples"):
        sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(1), ctx=OracleContext(mesh, data, inv), keep_samples=False)


# ---- the optional outputs together, and through parallelHMCSampler -----------------------------------------------------------------
HIST_KW = {"nbins": 17, "lo": -6.0, "hi": -3.5}          # (targets [3, 3, n - 1, 0]: a repeat, the last cell and the first)
OUT_PRIOR = dict(totalsamples=7, burninsamples=2, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0])


def _combined_context():
    """The stand-in with the histogram, data-moment and autocovariance accumulators at once: their chain_begin / chain_step overrides
    chain through super()."""
    from tests.test_acov_host import OracleAcovContext
    from tests.test_hist_host import OracleHistContext

    class OracleOutputsContext(OracleHistContext, OracleAcovContext):
        pass

    return OracleOutputsContext


def _same(a, b):
    """equality, array for array, of what fills an HMCStatus field: tuples, dicts, arrays, numbers, None"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_outputs_together_are_the_outputs_alone():
    """hist, data_moments and ess in one run: the chain is the chain without them, and every output is what its keyword alone gives."""
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    Ctx = _combined_context()
    kws = {"hist": dict(HIST_KW, targets=[3, 3, n - 1, 0]), "data_moments": True, "ess": {"maxlag": 3}}
    run = lambda **kw: sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), HMCPrior(**OUT_PRIOR), np.random.default_rng(21),
                                             ctx=Ctx(mesh, data, inv), device_chain=True, **kw)
    hm0, st0, hd0 = run()
    hm1, st1, hd1 = run(**kws)
    assert set(st0.acceptstats.tolist()) == {True, False}
    assert (st0.hist, st0.dataMoments, st0.ess, st0.cov, st0.adapt) == (None,) * 5
    assert np.array_equal(hm1, hm0) and np.array_equal(hd1, hd0) and np.array_equal(st1.hmstats, st0.hmstats)
    assert np.array_equal(st1.acceptstats, st0.acceptstats) and _same(st1.moments, st0.moments) and st1.moments[0] == 5
    for key, field in (("hist", "hist"), ("data_moments", "dataMoments"), ("ess", "ess")):
        _, alone, _ = run(**{key: kws[key]})
        assert getattr(st1, field) is not None and _same(getattr(st1, field), getattr(alone, field)), key
        assert [f for f in ("hist", "dataMoments", "ess") if getattr(alone, f) is not None] == [field]
    assert st1.hist[0] == st1.dataMoments[0] == st1.ess["count"] == 5 and st1.ess["misfit"]["count"] == 5


class _Recorded:
    """Hands every method of a context on and logs its name."""

    def __init__(self, ctx):
        self._ctx, self.log = ctx, []

    def __getattr__(self, name):
        fn = getattr(self._ctx, name)
        if not callable(fn):
            return fn

        def logged(*a, **kw):
            self.log.append(name)
            return fn(*a, **kw)

        return logged


def test_order_of_the_library_calls_up_to_the_first_momentum():
    """set_prior (set_mass), chain_begin at the homogeneous model, chain_state, chain_begin at the file's model and chain_set_energy,
    the outputs' begins in the order hist, data_moments, ess, cov, adapt, chain_adapt_info, chain_momentum -- and no begin behind it.
    The stand-in has no covariance and no warm-up: the second run gives it call-compatible stubs that compute nothing (count 0, a
    warm-up that leaves dt alone), which is all the order needs."""
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    kws = {"hist": dict(HIST_KW, targets=[3, 3, n - 1, 0]), "data_moments": True, "ess": {"maxlag": 3}}
    begins = ["chain_hist_begin", "chain_data_moments_begin", "chain_acov_begin"]

    def logged(ctx, prior, **kw):
        rec = _Recorded(ctx)
        sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), prior, np.random.default_rng(21), ctx=rec, device_chain=True, **kw)
        first = rec.log.index("chain_momentum")
        assert not [c for c in rec.log[first:] if c.endswith("begin")]
        tail = rec.log[first:]
        assert tail.index("chain_moments") < min(i for i, c in enumerate(tail) if c in READS)     # (chain_moments: the first read-out)
        assert tail.index("chain_moments") > max(i for i, c in enumerate(tail) if c in ("chain_step", "chain_momentum"))
        return rec.log[:first + 1]

    READS = ("chain_hist", "chain_data_moments", "chain_acov_count", "chain_acov", "chain_ess", "chain_cov_count", "chain_mass_diag")
    Ctx = _combined_context()
    assert logged(Ctx(mesh, data, inv), HMCPrior(**OUT_PRIOR), **kws) == \
        ["set_prior", "chain_begin", "chain_state", "chain_begin", "chain_set_energy"] + begins + ["chain_momentum"]

    class Stubbed(Ctx):
        def set_mass(self, kind):
            pass

        def chain_cov_begin(self, rows, batch):
            assert self.chain["p"] is None

        def chain_cov_count(self):
            return 0

        def chain_adapt_begin(self, nwarmup, **opts):
            assert self.chain["p"] is None

        def chain_adapt_info(self):
            return {"dt": self.prior.dt, "active": 0, "next_window_end": -1, "step": len(self.chain["committed"]), "window_count": 0}

    prior = HMCPrior(massType="nondiagonal", **OUT_PRIOR)
    assert logged(Stubbed(mesh, data, inv), prior, cov={"rows": [0, 3]}, adapt={"nwarmup": 2}, **kws) == \
        ["set_prior", "set_mass", "chain_begin", "chain_state", "chain_begin", "chain_set_energy"] + begins + \
        ["chain_cov_begin", "chain_adapt_begin", "chain_adapt_info", "chain_momentum"]


def test_parallel_sampler_keeps_every_output_of_a_local_chain():
    """hist and dataMoments stay with a chain that ran on this rank, as ess, cov and adapt do: the pooled histogram of two chains is
    the histogram of their kept samples pooled."""
    from tests import hist_ref
    Ctx = _combined_context()
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    t = np.array([3, 3, n - 1, 0])
    hm, hs, hd = sampler.parallelHMCSampler(mesh, data, inv, HMCPrior(**OUT_PRIOR), nchains=2, seed=5, device_chain=True,
                                            hist=dict(HIST_KW, targets=t), data_moments=True, ess={"maxlag": 3},
                                            context_factory=lambda m, d, i, dev: Ctx(m, d, i))
    assert len(hs) == 2 and all(st.hist is not None and st.dataMoments is not None and st.ess is not None for st in hs)
    assert all(st.cov is None and st.adapt is None for st in hs)
    for c in range(2):
        assert hs[c].hist[0] == 5 and hs[c].hist[2] == (17, -6.0, -3.5) and np.array_equal(hs[c].hist[3], t)
        assert np.array_equal(hs[c].hist[1], hist_ref.counts_of(list(hm[c][:, 2:].T), t, 17, -6.0, -3.5))
        post = hd[c][:, 3:]                                  # (column 0 is the start's)
        assert hs[c].dataMoments[0] == 5 and np.allclose(hs[c].dataMoments[1], post.mean(axis=1), rtol=1e-13, atol=0)
    assert not np.array_equal(hm[0], hm[1])              # (two chains, two streams)
    total, counts, bins, targets = sampler.mergeHistograms([st.hist for st in hs])
    pooled = list(hm[0][:, 2:].T) + list(hm[1][:, 2:].T)
    assert total == 10 and bins == (17, -6.0, -3.5) and np.array_equal(counts, hist_ref.counts_of(pooled, t, 17, -6.0, -3.5))


def test_gather_block_layout_sums_to_the_documented_size():
    """the fields of a chain's block add up to the formula of parallelHMCSampler's docstring"""
    nparam, ns, ndata = 37, 6, 10
    for ncols, with_moments in ((ns, True), (0, True), (ns, False)):
        fields = sampler.gatherBlockFields(nparam, ncols, ns, ndata, with_moments)
        assert [name for name, _ in fields][:5] == ["model", "hmstats", "acceptstats", "data", "secs_and_flag"]
        doc = nparam * ncols + 4 * (ns + 1) + ns + 2 * ndata * (ncols + 1) + 2 + ((1 + 2 * nparam) if with_moments else 0)
        assert sum(size for _, size in fields) == doc and all(size >= 0 for _, size in fields)
        if ncols == 0 and with_moments:
            assert doc == 2 * nparam + 5 * ns + 2 * ndata + 7
