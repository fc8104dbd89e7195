"""The chain's own random numbers without a GPU: Philox4x32-10, the uniforms, the scalars and the normals -- the item functions on the
host (tests/emul/emul_rng.cpp) and the product's own hmcmt_rng_draw / hmcmt_rng_normals through libhmcmt_hip.so against the
reference tests/rng_ref.py (Python integers, longdouble Box-Muller), Random123's known answers, the sanity of one draw, and the
bindings' symbol list."""
import os
import re

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from tests import rng_ref as R
from tests.conftest import ROOT
from tests.emul import emul_rng_py as E

F = 0xFFFFFFFF
LD = np.longdouble
# (seed, stream, t) of the draws the tests share: small numbers, every counter word in use, the high halves in use
DRAWS = [(1, 0, 0), (1, 1, 0), (1, 0, 1), (2, 0, 0), (0x0123456789ABCDEF, 0xDEADBEEF, (1 << 32) + 5), ((1 << 64) - 1, F, (1 << 64) - 1)]


@pytest.fixture(scope="module", autouse=True)
def so():
    L.build_library()
    return L.load_library()


def key_of(k):
    """the (seed, ...) that build a known answer's key"""
    return k[0] | (k[1] << 32)


@pytest.mark.parametrize("c,k,out", R.KAT)
def test_known_answers_of_the_reference_and_of_the_item_function(c, k, out):
    assert R.philox4x32(c, k) == out
    assert E.philox(c, k) == out


def test_known_answers_through_the_library():
    """The library's generator has no entry point of its own; its counter is (c0, stream, t lo, t hi) and its key the seed's halves, so
    a seed, stream, t and cell are built that make each known answer's block the block of a draw.  c0 = 0xFFFFFFFF is the scalars'
    block: the all-ones vector comes out of hmcmt_rng_draw, u bit for bit and L exactly.  The other two have c0 < 2^31, a cell's
    block: their normals come out of hmcmt_rng_normals and are held to the normal of the PUBLISHED words."""
    c, k, out = R.KAT[1]
    assert c[0] == R.C0_SCALARS
    Lv, u = L.rng_draw(key_of(k), c[1], c[2] | (c[3] << 32), 6, 10)
    assert u == R.u52(out[0], out[1]) and Lv == 6 + ((out[2] * 5) >> 32)
    for c, k, out in (R.KAT[0], R.KAT[2]):
        assert c[0] < 2 ** 31
        z = L.rng_normals(key_of(k), c[1], c[2] | (c[3] << 32), 1, a0=c[0])
        assert abs(float(LD(z[0]) - R.normal_of_block(out))) <= R.NORMAL_TOL
        assert R.block(key_of(k), c[1], c[2] | (c[3] << 32), c[0]) == out


def test_uniforms_bit_for_bit():
    rng = np.random.default_rng(11)
    words = [(0, 0), (F, F), (0, F), (F, 0), (63, 63), (64, 64), (1 << 31, 1 << 31)] + [tuple(int(x) for x in rng.integers(0, 1 << 32, 2)) for _ in range(2000)]
    for hi, lo in words:
        u = E.u52(hi, lo)
        assert u == R.u52(hi, lo) and 0.0 < u < 1.0
        k = R.u52_k(hi, lo)
        assert 0 <= k < 1 << 52 and u * 2.0 ** 53 == 2 * k + 1       # (exact: an odd integer below 2^53)
    assert E.u52(0, 0) == 2.0 ** -53 and E.u52(F, F) == 1.0 - 2.0 ** -53
    assert E.u52(63, 63) == 2.0 ** -53                                # (the low six bits of either word are not used)


@pytest.mark.parametrize("seed,stream,t", DRAWS)
def test_scalars_through_the_library_and_of_the_item_function(seed, stream, t):
    for Lmin, Lmax in ((6, 10), (1, 1), (1, 2 ** 31 - 1), (7, 7)):
        ref = R.scalars(seed, stream, t, Lmin, Lmax)
        assert L.rng_draw(seed, stream, t, Lmin, Lmax) == ref
        assert E.scalars(seed, stream, t, Lmin, Lmax) == ref
        assert Lmin <= ref[0] <= Lmax and 0.0 < ref[1] < 1.0


def test_trajectory_lengths_over_4096_draws():
    got = [L.rng_draw(3, 2, t, 6, 10) for t in range(4096)]
    assert got == [R.scalars(3, 2, t, 6, 10) for t in range(4096)]
    Ls = np.array([g[0] for g in got])
    assert set(Ls.tolist()) == {6, 7, 8, 9, 10}
    counts = np.bincount(Ls)[6:]
    # five equally likely values (the multiply-shift's bias is 5 / 2^32): each count within 5 sigma of 4096 / 5
    assert np.all(np.abs(counts - 4096 / 5) < 5 * np.sqrt(4096 * 0.2 * 0.8)), counts
    us = np.array([g[1] for g in got])
    assert abs(us.mean() - 0.5) < 4 / np.sqrt(12 * 4096) and len(set(us.tolist())) == 4096
    assert [L.rng_draw(3, 2, t, 4, 4)[0] for t in range(64)] == [4] * 64


def test_bad_arguments_of_the_host_calls():
    for Lmin, Lmax in ((0, 3), (-1, 3), (4, 3)):
        with pytest.raises(L.HmcmtError) as e:
            L.rng_draw(1, 0, 0, Lmin, Lmax)
        assert e.value.code == -1
    for a0, n in ((-1, 4), (0, -1), (2 ** 31 - 1, 2), (2 ** 31, 0)):
        with pytest.raises(L.HmcmtError) as e:
            L.rng_normals(1, 0, 0, n, a0=a0)
        assert e.value.code == -1
    assert len(L.rng_normals(1, 0, 0, 0)) == 0
    assert len(L.rng_normals(1, 0, 0, 1, a0=2 ** 31 - 1)) == 1
    with pytest.raises(ValueError):
        L.rng_draw(1 << 64, 0, 0, 1, 2)
    with pytest.raises(ValueError):
        L.rng_draw(1, 1 << 32, 0, 1, 2)


@pytest.fixture(scope="module")
def reference_normals():
    """the longdouble normals of 2000 cells per shared draw (computed once, left unchanged)"""
    return {d: R.normals(*d, 2000) for d in DRAWS}


@pytest.mark.parametrize("seed,stream,t", DRAWS)
def test_normals_against_the_longdouble_reference(seed, stream, t, reference_normals):
    """hmcmt_rng_normals (the library's host code: hipcc's host compiler, glibc) and the emulated item (g++ -O2, glibc) within
    rng_ref.NORMAL_TOL = 4e-14 absolute of the longdouble Box-Muller of the exact uniforms.  Measured over these 12000 normals: both
    1.74e-15 at the most -- one ulp of a value in [4, 8) is 8.9e-16."""
    ref = reference_normals[(seed, stream, t)]
    worst = {}
    for name, z in (("library", L.rng_normals(seed, stream, t, 2000)), ("item", E.normals(seed, stream, t, 2000))):
        worst[name] = float(np.abs(z.astype(LD) - ref).max())
        assert np.all(np.isfinite(z)) and np.abs(z).max() <= 8.58
    print(f"\n[normals, seed {seed:#x} stream {stream:#x} t {t:#x}] largest |z - ref|: {worst} (bound {R.NORMAL_TOL})")
    assert max(worst.values()) <= R.NORMAL_TOL


def test_sanity_of_one_draw_of_20000_cells():
    """seed 1, stream 0, t = 0: mean, variance and the share beyond the clip of a standard normal within four standard errors; other
    streams, draws and seeds give other vectors; a cell's value depends neither on n nor on a0.  Catches a wrong word order, which
    the block function's known answers cannot."""
    n = 20000
    z = L.rng_normals(1, 0, 0, n)
    assert abs(z.mean()) < 4 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 4 * np.sqrt(2.0 / n)
    share = float((np.abs(z) > 2.5).mean())
    assert abs(share - 0.0124) < 4 * np.sqrt(0.0124 / n), share
    assert len(set(z.tolist())) == n
    for other in ((1, 1, 0), (1, 0, 1), (2, 0, 0), (1 << 32 | 1, 0, 0), (1, 0, 1 << 32)):
        zo = L.rng_normals(*other, n)
        assert not np.any(zo == z)
        assert abs(float(np.corrcoef(z, zo)[0, 1])) < 4 / np.sqrt(n)       # (uncorrelated: four standard errors of r)
    assert np.array_equal(L.rng_normals(1, 0, 0, 100), z[:100])
    assert np.array_equal(L.rng_normals(1, 0, 0, 300, a0=16000), z[16000:16300])
    assert np.abs(E.normals(1, 0, 0, 50, a0=19950) - z[19950:]).max() <= 2 * R.NORMAL_TOL      # (each within the bound of the reference)
    # the first cells against the reference's words, so that the draw above is the header's counter layout and not merely a good one
    assert np.abs(z[:64].astype(LD) - R.normals(1, 0, 0, 64)).max() <= R.NORMAL_TOL


def test_seeded_momentum_items_equal_the_fed_ones():
    """item_chain_draw_momentum (k_chain_draw_momentum's body) against item_chain_momentum fed with item_chain_draw_clip's output
    (k_chain_draw_clip, then k_chain_momentum): the same p and the same term of p' M^-1 p bit for bit, on the host instantiation;
    the clipped normals are the reference's, clipped."""
    n = 1500
    invM = np.random.default_rng(5).uniform(0.25, 4.0, n)
    zc, p_draw, p_fed, term_draw, term_fed = E.momentum(9, 3, 17, invM)
    assert np.array_equal(p_draw, p_fed) and np.array_equal(term_draw, term_fed)
    ref = R.clipped(R.normals(9, 3, 17, n))
    assert np.abs(zc.astype(LD) - ref).max() <= R.NORMAL_TOL
    assert (np.abs(zc) == 2.5).sum() >= 5 and np.abs(zc).max() == 2.5
    assert np.array_equal(p_draw, zc / np.sqrt(invM))


def test_the_header_the_bindings_and_julia_name_the_calls():
    hdr = open(os.path.join(ROOT, "include", "hmcmt.h")).read()
    for sym in L.CHAIN_RNG_SYMBOLS:
        assert re.search(r"extern int %s\(" % sym, hdr), sym
        assert sym in L.PRODUCT_SYMBOLS
    assert len(L.CHAIN_RNG_SYMBOLS) == 8
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    for sym in ("hmcmt_chain_seed", "hmcmt_chain_sample", "hmcmt_chain_run", "hmcmt_chain_rng_state"):
        assert f"libhmcmt.{sym}(" in jl, sym
    for fn in ("chain_seed!", "chain_sample!", "chain_run!"):
        assert f"function {fn}(" in jl or f"\n{fn}(" in jl, fn
    assert re.search(r"function run_chain!\(.*?seed::", jl, flags=re.S)
