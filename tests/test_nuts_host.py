"""The No-U-turn sampler without a GPU: the draws of hmcmt_rng_nuts against tests/rng_ref.py's Philox, the checkpoint rule against a
brute-force enumeration of the aligned spans, the host instantiation of the item functions (tests/emul/emul_nuts.cpp: the scalar state
machine and k_nuts_leaf's sums) against tests/nuts_ref.py and a longdouble evaluation, and nuts_ref's stationarity on a correlated
Gaussian -- with a deliberately wrong sampler that the same bound refuses."""
import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd import sampler as S
from tests import nuts_ref as N
from tests.emul import emul_nuts_py as E

LD = np.longdouble
SEED = 0x5EED0123456789AB
T_HIGH = (1 << 32) + 5


# ---- 1. the draws --------------------------------------------------------------------------------------------------------------------
def test_rng_nuts_is_the_reference_bit_for_bit():
    """hmcmt_rng_nuts (and the item function on the host) = rng_ref's Philox at c0 = 0xC0000000 + j / 0x80000000 + l: u bit for bit,
    forward exactly, for t = 0 and t = 2^32 + 5 and two streams"""
    fwd = []
    for stream in (0, 3):
        for t in (0, T_HIGH):
            for kind, idx in [(0, j) for j in range(10)] + [(1, l) for l in (0, 1, 2, 7, 511, 1022, (1 << 30) - 1)]:
                ref = N.rng_nuts(SEED, stream, t, kind, idx)
                assert L.rng_nuts(SEED, stream, t, kind, idx) == ref
                assert E.rng(SEED, stream, t, kind, idx) == ref
                assert 0.0 < ref[1] < 1.0
                if kind == 0:
                    fwd.append(ref[0])
    assert 0 in fwd and 1 in fwd
    assert N.rng_nuts(SEED, 0, 0, 0, 0)[1] != N.rng_nuts(SEED, 0, 0, 1, 0)[1]
    for bad in ((2, 0), (-1, 0), (0, 32), (1, 1 << 30)):
        with pytest.raises(L.HmcmtError):
            L.rng_nuts(SEED, 0, 0, *bad)


# ---- 2. the checkpoint rule ------------------------------------------------------------------------------------------------------------
def test_checkpoints_are_the_aligned_spans():
    """For every odd i < 1024 the slots visited hold the first leaves of exactly the aligned spans [i + 1 - 2^s, i], s = 1 .. trailing
    ones of i, each once: the slots are filled by the even leaves in order and looked up as the rule says."""
    owner = {}
    for i in range(1024):
        slot, ndue = E.checkpoints(i)
        assert slot == bin(i >> 1).count("1") and (i >= 512 or slot < E.constants()["ck_max"])
        if i % 2 == 0:
            owner[slot] = i
            continue
        starts = [owner[slot - c] for c in range(ndue)]
        assert [slot - c for c in range(ndue)] == N.due_checkpoints(i)
        brute = [a for a in range(i) if (i + 1 - a) & (i - a) == 0 and i + 1 - a >= 2 and a % (i + 1 - a) == 0]
        assert sorted(starts) == brute and len(set(starts)) == len(starts) == ndue >= 1
        assert [i + 1 - (1 << s) for s in range(1, ndue + 1)] == starts
    assert max(E.checkpoints(i)[0] for i in range(0, 512, 2)) == E.constants()["ck_max"] - 1       # (depth 10: every slot is used)


# ---- 3. the host instantiation ---------------------------------------------------------------------------------------------------------
def gaussian(dim=6, seed=11, lo=0.05, hi=9.0):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    var = np.geomspace(lo, hi, dim)
    cov = (Q * var) @ Q.T
    return cov, np.linalg.inv(cov)


def test_host_instantiation_takes_the_reference_decisions():
    """200 samples on a 6-dimensional correlated Gaussian with a non-unit diagonal mass: the item functions' state machine, fed by the
    emulated kernels' sums, takes nuts_ref's decisions; energies agree to 1e-12 relative"""
    cov, A = gaussian()
    inv_m = np.array([0.7, 1.3, 1.0, 0.5, 2.0, 1.1])
    G = N.Gaussian(A, inv_m, 0.25)
    rng = np.random.default_rng(5)
    m = rng.standard_normal(6)
    stops, depths, worst = set(), set(), 0.0
    for t in range(200):
        p0 = rng.standard_normal(6) / np.sqrt(inv_m)
        ref = N.sample(G.state(m, p0), G.leaf, 6, *N.philox_draws(SEED, 2, t))
        rec, m_sel, energies = E.sample(A, inv_m, 0.25, 6, SEED, 2, t, m, p0)
        for key in ("depth", "nleaves", "stop", "dirs", "selected"):
            assert rec[key] == ref[key], (t, key, rec, ref)
        assert abs(rec["alpha"] - ref["alpha"]) <= 1e-12
        e_ref = np.array(ref["energies"])
        worst = max(worst, float(np.max(np.abs(energies - e_ref) / np.abs(e_ref))), abs(rec["Hsel"] - ref["state"].H) / abs(ref["state"].H))
        assert np.allclose(m_sel, ref["state"].m, rtol=0, atol=1e-12)
        stops.add(ref["stop"]); depths.add(ref["depth"])
        m = ref["state"].m
    print(f"\n[host instantiation] stops {sorted(stops)}, depths {sorted(depths)}, worst relative energy difference {worst:.3g}")
    assert worst <= 1e-12 and {1, 2} <= stops and len(depths) >= 3


def leaf_cases(n, seed=3):
    """The leaf passes the kernel tests share (tests/test_gpu_chain_nuts.py runs the same on the device): name -> keyword arguments of
    emul_nuts_py.leaf / HipContext.debug_nuts_leaf as host arrays.  0, 1, 4 and 9 due checkpoints (9: three passes), the merged-tree
    pair, both signs, an even leaf that writes its checkpoint, the diagonal mass and a given x."""
    rng = np.random.default_rng(seed + n)
    v = lambda: rng.standard_normal(n)
    inv_m = rng.uniform(0.5, 2.0, n)
    trips = [(v(), v(), v()) for _ in range(9)]
    merged = lambda ob: dict(rho=v(), rho_next=np.zeros(n), p_other=v(), other_backward=ob)
    return {
        "even first": dict(p=v(), rho_s=v(), inv_m=inv_m, first=True, ck_write=(np.zeros(n), np.zeros(n), np.zeros(n))),
        "even backward": dict(p=v(), rho_s=v(), inv_m=inv_m, backward=True, ck_write=(np.zeros(n), np.zeros(n), np.zeros(n))),
        "single leaf": dict(p=v(), rho_s=v(), inv_m=inv_m, first=True, ck_write=(np.zeros(n), np.zeros(n), np.zeros(n)), merged=merged(True)),
        "odd 1": dict(p=v(), rho_s=v(), inv_m=inv_m, ck_due=trips[:1]),
        "odd 1 backward x": dict(p=v(), rho_s=v(), x=v(), backward=True, ck_due=trips[1:2]),
        "odd 4 merged": dict(p=v(), rho_s=v(), inv_m=inv_m, ck_due=trips[:4], merged=merged(True)),
        "odd 4 merged backward x": dict(p=v(), rho_s=v(), x=v(), inv_m=inv_m, backward=True, ck_due=trips[2:6],
                                        merged=dict(merged(False), x_other=v())),
        "odd 9 merged": dict(p=v(), rho_s=v(), inv_m=inv_m, ck_due=trips, merged=merged(True)),
    }


def copy_case(kw):
    out = dict(kw)
    out["rho_s"] = kw["rho_s"].copy()
    if "ck_write" in kw:
        out["ck_write"] = tuple(a.copy() for a in kw["ck_write"])
    if "merged" in kw:
        out["merged"] = dict(kw["merged"], rho_next=kw["merged"]["rho_next"].copy())
    return out


def leaf_longdouble(kw):
    """the sums of one pass in longdouble with the bound n 2^-53 sum |terms| per sum, and the vectors the pass writes"""
    n = len(kw["p"])
    sg = -1.0 if kw.get("backward") else 1.0
    p = sg * kw["p"]
    x = sg * (kw["x"] if kw.get("x") is not None else kw["inv_m"] * kw["p"])
    rs = p.copy() if kw.get("first") else kw["rho_s"] + p
    sums, bound = np.zeros(21, dtype=LD), np.zeros(21, dtype=LD)

    def dot(q, a, b):
        terms = a.astype(LD) * b.astype(LD)
        sums[q], bound[q] = terms.sum(), LD(n) * LD(2.0) ** -53 * np.abs(terms).sum()

    dot(0, p, x)
    out = {"rho_s": rs}
    if kw.get("merged"):
        M = kw["merged"]
        so = -1.0 if M.get("other_backward") else 1.0
        xo = so * (M["x_other"] if M.get("x_other") is not None else kw["inv_m"] * M["p_other"])
        rn = M["rho"] + rs
        dot(1, x, rn); dot(2, xo, rn)
        out["rho_next"] = rn
    for c, (pk, xk, rk) in enumerate(kw.get("ck_due", ())):
        span = (rs - rk) + pk
        dot(3 + 2 * c, xk, span); dot(4 + 2 * c, x, span)
    if kw.get("ck_write") is not None:
        out["ck_write"] = (p, x, rs)
    return sums, bound, out


@pytest.mark.parametrize("n", [96, 390, 20000])
def test_emulated_leaf_sums_against_longdouble(n):
    """k_nuts_leaf's arithmetic and order on the host: every sum within n 2^-53 sum |terms| of the longdouble evaluation, the vectors
    written (rho_s, the checkpoint, rho_next) exactly the elementwise fp64 results, rows that are not due 0"""
    worst = 0.0
    for name, kw in leaf_cases(n).items():
        run = copy_case(kw)
        sums = E.leaf(**run)
        ref, bound, out = leaf_longdouble(kw)
        nq = 3 + 2 * len(kw.get("ck_due", ()))
        assert np.all(sums[nq:] == 0.0) and np.all(np.abs(sums[:nq].astype(LD) - ref[:nq]) <= bound[:nq]), name
        worst = max(worst, float(np.max(np.abs(sums[:nq].astype(LD) - ref[:nq]) / np.maximum(bound[:nq], LD(1e-300)))))
        assert np.array_equal(run["rho_s"], out["rho_s"]), name
        if "ck_write" in kw:
            assert all(np.array_equal(a, b) for a, b in zip(run["ck_write"], out["ck_write"])), name
        if "merged" in kw:
            assert np.array_equal(run["merged"]["rho_next"], out["rho_next"]), name
            assert sums[1] != 0.0 and sums[2] != 0.0
        else:
            assert sums[1] == 0.0 and sums[2] == 0.0
    print(f"\n[emulated leaf sums, n {n}] worst |sum - longdouble| / bound {worst:.3g}")


# ---- 4. stationarity ---------------------------------------------------------------------------------------------------------------------
def acov_of(y, maxlag):
    y = y - y.mean(axis=0)
    n = len(y)
    return np.array([(y[:n - k] * y[k:]).sum(axis=0) / n for k in range(maxlag + 1)])


def gaussian_run(dt, nsamples, seed, use_weights=True, max_depth=8):
    cov, A = gaussian()
    G = N.Gaussian(A, np.ones(6), dt)
    rng = np.random.default_rng(seed)
    m = np.linalg.cholesky(cov) @ rng.standard_normal(6)
    xs = np.empty((nsamples, 6))
    leaves = 0
    for t in range(nsamples):
        r = N.sample(G.state(m, rng.standard_normal(6)), G.leaf, max_depth, *N.philox_draws(seed, 0, t), use_weights=use_weights)
        m = r["state"].m
        xs[t] = m
        leaves += r["nleaves"]
    return cov, xs, leaves


def deviations(cov, xs):
    """per coordinate (in the eigenbasis of nothing: the coordinates themselves): |mean| and |variance - true| in standard errors
    computed from the run's own autocovariances (sampler.essFromAcov)"""
    n = len(xs)
    true_var = np.diag(cov)
    _, ess_x, _ = S.essFromAcov(acov_of(xs, 200), n)
    y = (xs - xs.mean(axis=0)) ** 2
    _, ess_y, _ = S.essFromAcov(acov_of(y, 200), n)
    se_mean = np.sqrt(xs.var(axis=0) / ess_x)
    se_var = np.sqrt(y.var(axis=0) / ess_y)
    return np.abs(xs.mean(axis=0)) / se_mean, np.abs(xs.var(axis=0) - true_var) / se_var, xs.var(axis=0) / true_var


STATIONARITY_SEED = 2017


def test_reference_is_stationary_on_a_correlated_gaussian():
    """nuts_ref on a 6-dimensional correlated Gaussian with variances 0.05 to 9, dt = 0.25, max_depth = 8, 4000 samples: per-coordinate
    mean and variance within 5 standard errors.  The bound has teeth: the same run with leaves selected uniformly (weights ignored)
    at dt = 0.6 fails it."""
    cov, xs, leaves = gaussian_run(0.25, 4000, STATIONARITY_SEED)
    dm, dv, ratio = deviations(cov, xs)
    print(f"\n[stationarity] {leaves / 4000:.1f} leaves per sample; |mean| / se {np.round(dm, 2)}; |var - true| / se {np.round(dv, 2)}; "
          f"variance ratios {np.round(ratio, 3)}")
    assert np.all(dm <= 5.0) and np.all(dv <= 5.0)
    cov, xs, leaves = gaussian_run(0.6, 4000, STATIONARITY_SEED, use_weights=False)
    dm, dv, ratio = deviations(cov, xs)
    print(f"[uniform selection, dt 0.6] |mean| / se {np.round(dm, 2)}; |var - true| / se {np.round(dv, 2)}; variance ratios {np.round(ratio, 3)}")
    assert np.any(dm > 5.0) or np.any(dv > 5.0)


# ---- 5. the records' layout ----------------------------------------------------------------------------------------------------------------
def test_record_layouts_match_the_header(tmp_path):
    """hmcmt_nuts_record and hmcmt_debug_nuts_args through a C compiler against the ctypes mirrors of hmcmt2d_amd/lib.py, and the field
    order of julia/HMCMTHip.jl's HmcmtNutsRecord"""
    import ctypes
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = [f for f, _ in L.NutsRecord._fields_]
    args = [f for f, _ in L.DebugNutsArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hmcmt_debug.h"', 'int main(void) {',
             'printf("sizeof rec %zu\\nsizeof args %zu\\n", sizeof(hmcmt_nuts_record), sizeof(hmcmt_debug_nuts_args));',
             'printf("const depth %d\\nconst ck %d\\nconst sums %d\\n", HMCMT_NUTS_DEPTH_MAX, HMCMT_NUTS_CK_MAX, HMCMT_NUTS_SUMS);']
    lines += [f'printf("rec.{f} %zu\\n", offsetof(hmcmt_nuts_record, {f}));' for f in rec]
    lines += [f'printf("args.{f} %zu\\n", offsetof(hmcmt_debug_nuts_args, {f}));' for f in args]
    src = tmp_path / "nuts_abi.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = str(tmp_path / "nuts_abi")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got["sizeof rec"]) == ctypes.sizeof(L.NutsRecord) and int(got["sizeof args"]) == ctypes.sizeof(L.DebugNutsArgs)
    for f in rec:
        assert int(got[f"rec.{f}"]) == getattr(L.NutsRecord, f).offset, f
    for f in args:
        assert int(got[f"args.{f}"]) == getattr(L.DebugNutsArgs, f).offset, f
    assert (int(got["const depth"]), int(got["const ck"]), int(got["const sums"])) == (L.NUTS_DEPTH_MAX, L.NUTS_CK_MAX, L.NUTS_SUMS)
    c = E.constants()
    assert (c["depth_max"], c["ck_max"], c["nq"]) == (L.NUTS_DEPTH_MAX, L.NUTS_CK_MAX, L.NUTS_SUMS)
    julia = open(os.path.join(root, "julia", "HMCMTHip.jl")).read()
    body = re.search(r"struct HmcmtNutsRecord\n(.*?)\nend", julia, flags=re.S).group(1)
    assert [ln.split("::")[0].strip() for ln in body.splitlines()] == rec
    # run_chain!(...; nuts=d): its loop holds an HmcmtNutsRecord there, whose chain record is the field `rec`.  No field of the chain
    # record may be read from the loop's `rec` before it is unwrapped, in either branch that can hold a tree's record
    fn = julia[julia.index("function run_chain!("):]
    loop = fn[fn.index("for it = 1:nsamples"):fn.index("adaptStats =")]
    unwrap = loop.index("rec = rec.rec")
    assert "push!(nutsRecs, rec)" in loop[:unwrap] and "rec.alpha" in loop[:unwrap]
    chain_fields = [f for f, _ in L.ChainRecord._fields_]
    before = loop[:unwrap]
    guard = before.rindex("if nuts !== nothing")
    assert not re.search(r"\brec\.(%s)\b" % "|".join(chain_fields), before[:guard]), "a chain-record field is read before the unwrap"
    after_else = loop[unwrap:loop.index("end", unwrap) + 3]
    assert re.search(r"else\s+alphaOf = rec\.hdif", after_else)              # (the hdif-based alpha only where rec is a chain record)
    for sym in ("hmcmt_chain_nuts_sample", "hmcmt_chain_nuts_run"):
        assert re.search(r"@ccall libhmcmt\.%s\(" % sym, julia), sym
    export = re.search(r"^export (.*?)\n\n", julia, flags=re.S | re.M).group(1)
    assert all(name in export for name in ("chain_nuts_sample!", "chain_nuts_run!", "HmcmtNutsRecord"))
