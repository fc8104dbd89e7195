"""The row sketch of the device chain without a GPU: the numpy reference (tests/sketch_ref.py), sampler.sketchOf / pcaFromSketch /
mergeSketches / lowRankMassFromSketch, and the host instantiation of the library's item functions (tests/emul/emul_sketch.cpp)
under the guarantee the header states."""
import numpy as np
import pytest

from hmcmt2d_amd import sampler as S
from tests import sketch_ref as R
from tests.emul import emul_sketch_py as E

# (cells, commits, ell): one partly filled workgroup and a full one with a partial one; ell 12 at 22 commits never shrinks
SHAPES = [(96, 22, 4), (390, 22, 4), (390, 22, 12), (390, 200, 8)]
RANK = 4            # the chains have three strong modes: the fourth component is noise, 2e-5 of the first
# The Gram-route PCA of the REFERENCE against numpy.linalg.eigh of the exact centred covariance, measured on the CPU over the shapes
# of NO_SHRINK below (rank 4): the largest relative eigenvalue error was 3.4e-12, the largest residual |C u - lam u| / lam_1 2.1e-13
# (the Gram route squares the condition: the fourth eigenvalue is 2e-5 of the first).  The bounds are 100 x that, since the library's
# fma order and its Jacobi differ from numpy's; its host instantiation measured 2.2e-11 and 6.0e-13.
PCA_REL, PCA_RES = 100 * 3.4e-12, 100 * 2.1e-13
NO_SHRINK = [(96, 22, 12), (390, 22, 12)]


def chain_of(n, N, ell):
    return R.synthetic_chain(n, N, modes=3, seed=1000 * ell + n + N)


_cache = {}


def case(shape):
    """the chain of a shape and its three sketches, computed once and left unchanged"""
    if shape not in _cache:
        n, N, ell = shape
        X = chain_of(*shape)
        _cache[shape] = {"X": X, "ref": R.sketch(X, ell), "np": S.sketchOf(X.T, ell), "emul": E.as_sketch(E.commit(E.begin(n, ell), X))}
    return _cache[shape]


def check_guarantee(sk, A, what):
    """0 <= A'A - B'B <= Delta I and Delta <= min_k |A - A_k|_F^2 / (ell - k), with the rounding slack s = 1e-12 |A|_F^2"""
    g = R.guarantee(sk, A)
    s = 1e-12 * g["frob2"]
    print(f"{what}: lmin/|A|^2 {g['lmin'] / g['frob2']:.2e} lmax-Delta {g['lmax'] - sk['Delta']:.2e} Delta {sk['Delta']:.6e} bound {g['bound']:.6e}")
    assert g["lmin"] >= -s and g["lmax"] <= sk["Delta"] + s
    assert sk["Delta"] <= g["bound"] + s
    return s


def check_eigenvalues(lam, err, A, s, what):
    exact = np.linalg.eigvalsh(R.centred_cov(A))[::-1]
    shift = np.abs(lam - exact[:len(lam)])
    print(f"{what}: shift {shift} err {err:.6e}")
    assert np.all(np.diff(lam) <= 0) and np.all(shift <= err + s / A.shape[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_three_sketches_meet_the_guarantee_and_agree(shape):
    n, N, ell = shape
    c = case(shape)
    A = c["ref"]["A"]
    shrinks = 0 if N < 2 * ell else (N - ell) // ell
    for name in ("ref", "np", "emul"):
        sk = c[name]
        assert (sk["count"], sk["ell"], sk["shrinks"]) == (N, ell, shrinks) and sk["fill"] == N - shrinks * ell == sk["rows"].shape[0]
        s = check_guarantee(sk, A, f"{shape} {name}")
        lam, U, err = (R.pca(sk, RANK) if name == "ref" else S.pcaFromSketch(sk, RANK))
        assert err == sk["Delta"] / N
        check_eigenvalues(lam, err, A, s, f"{shape} {name}")
        if shrinks == 0:
            assert sk["Delta"] == 0.0 and np.abs(A.T @ A - sk["rows"].T @ sk["rows"]).max() <= s
    # the same algorithm three times: the Gram matrices of the rows agree far inside the guarantee's slack
    G = c["ref"]["rows"].T @ c["ref"]["rows"]
    for name in ("np", "emul"):
        assert np.abs(c[name]["rows"].T @ c[name]["rows"] - G).max() <= 1e-12 * np.trace(A.T @ A)
        assert abs(c[name]["Delta"] - c["ref"]["Delta"]) <= 1e-10 * max(c["ref"]["Delta"], 1e-300) or shrinks == 0
        for k in ("x0", "tot", "q"):
            assert np.allclose(c[name][k], c["ref"][k], rtol=1e-13, atol=0)
    # the commit's sums are the library's bits in numpy too: serial adds and one subtraction
    assert np.array_equal(c["emul"]["x0"], c["np"]["x0"]) and np.array_equal(c["emul"]["tot"], c["np"]["tot"])


def test_the_emulation_pca_meets_the_bound_behind_shrinks():
    for shape in SHAPES:
        n, N, ell = shape
        X = chain_of(*shape)
        st = E.commit(E.begin(n, ell), X)
        lam, U, err, G, coef = E.pca(st, RANK)
        A = X - X[0][None, :]
        check_eigenvalues(lam, err, A, 1e-12 * float((A * A).sum()), f"{shape} emul pca")
        assert np.abs(U @ U.T - np.eye(len(lam))).max() <= 1e-8
        for k in range(len(lam)):
            assert U[k, np.argmax(np.abs(U[k]))] > 0
        rows = st["B"][:st["fill"]].copy()
        lam2, U2 = E.pca(st, RANK)[:2]                       # a read-out changes nothing but the staging row
        assert np.array_equal(lam, lam2) and np.array_equal(U, U2) and np.array_equal(rows, st["B"][:st["fill"]])


@pytest.mark.parametrize("shape", NO_SHRINK)
def test_gram_route_pca_against_eigh_where_nothing_was_shrunk(shape):
    """Measured (see PCA_REL, PCA_RES above): reference 3.4e-12 / 2.1e-13, the library's host instantiation 2.2e-11 / 6.0e-13."""
    n, N, ell = shape
    X = chain_of(*shape)
    A = X - X[0][None, :]
    C = R.centred_cov(A)
    exact = np.linalg.eigvalsh(C)[::-1]
    for name, (lam, U) in (("ref", R.pca(R.sketch(X, ell), RANK)[:2]), ("np", S.pcaFromSketch(S.sketchOf(X.T, ell), RANK)[:2]),
                           ("emul", E.pca(E.commit(E.begin(n, ell), X), RANK)[:2])):
        assert len(lam) == RANK
        rel = np.max(np.abs(lam - exact[:RANK]) / exact[:RANK])
        res = max(np.linalg.norm(C @ U[k] - lam[k] * U[k]) / lam[0] for k in range(RANK))
        print(f"{shape} {name}: rel {rel:.2e} residual {res:.2e}")
        assert rel <= PCA_REL and res <= PCA_RES


def test_merge_of_two_chains_under_a_common_pivot():
    n, ell = 390, 8
    X1, X2 = R.synthetic_chain(n, 60, seed=5), R.synthetic_chain(n, 75, seed=6)
    pivot = X1[0] + 0.01
    both = np.vstack([X1, X2])
    A = both - pivot[None, :]
    for name, sk_of, merge in (("ref", lambda X: R.sketch(X, ell, pivot), R.merge), ("np", lambda X: S.sketchOf(X.T, ell, pivot), S.mergeSketches)):
        merged, whole = merge([sk_of(X1), sk_of(X2)]), sk_of(both)
        assert merged["count"] == whole["count"] == 135 and merged["shrinks"] > sk_of(X1)["shrinks"] + sk_of(X2)["shrinks"]
        assert np.allclose(merged["tot"], whole["tot"], rtol=1e-12) and np.allclose(merged["q"], whole["q"], rtol=1e-12)
        for what, sk in (("merged", merged), ("whole", whole)):
            s = check_guarantee(sk, A, f"merge {name} {what}")
            lam, U, err = S.pcaFromSketch(sk, 3)
            check_eigenvalues(lam, err, A, s, f"merge {name} {what}")
    # the merge needs one given pivot, byte for byte
    a, b = S.sketchOf(X1.T, ell, pivot), S.sketchOf(X2.T, ell, pivot + 1e-9)
    with pytest.raises(ValueError, match="pivot"):
        S.mergeSketches([a, b])
    with pytest.raises(ValueError, match="pivot"):
        S.mergeSketches([S.sketchOf(X1.T, ell), S.sketchOf(X1.T, ell)])
    with pytest.raises(ValueError, match="ell"):
        S.mergeSketches([a, S.sketchOf(X2.T, ell + 1, pivot)])


@pytest.mark.parametrize("shape", NO_SHRINK)
def test_low_rank_mass_from_a_sketch_equals_the_one_from_the_samples_where_nothing_was_shrunk(shape):
    n, N, ell = shape
    X = chain_of(*shape)
    for invM in (None, np.linspace(0.5, 2.0, n)):
        s0, U0, l0 = S.lowRankMassFromSamples(X.T, rank=RANK, cutoff=2.0, invM=invM)
        s1, U1, l1 = S.lowRankMassFromSketch(S.sketchOf(X.T, ell), invM=invM, rank=RANK, cutoff=2.0)
        assert len(l0) == len(l1) == 3                      # the three modes; the noise stays below the cutoff
        assert np.allclose(s0, s1, rtol=1e-12, atol=0)
        assert np.max(np.abs(l1 - l0) / l0) <= PCA_REL and np.abs(U1 - U0).max() <= 100 * PCA_RES
        assert np.abs(U1 @ U1.T - np.eye(3)).max() <= 1e-10


def test_the_helpers_refuse_what_the_library_refuses():
    X = chain_of(96, 22, 4)
    for ell in (1, 65):
        with pytest.raises(ValueError):
            S.sketchOf(X.T, ell)
    with pytest.raises(ValueError):
        S.sketchOf(X.T, 4, pivot=np.full(96, np.nan))
    with pytest.raises(ValueError):
        S.pcaFromSketch(S.sketchOf(X[:1].T, 4), 2)
    c = E.constants()
    assert (c["ell_min"], c["ell_max"], c["ell_default"]) == (2, 64, 32)
    from hmcmt2d_amd import lib as L
    assert L.SKETCH_ELL_MAX == c["ell_max"] and set(L.CHAIN_SKETCH_SYMBOLS) <= set(L.PRODUCT_SYMBOLS)
    assert any(out.name == "sketch" and out.field == "sketch" for out in S.CHAIN_OUTPUTS)


def test_getPCAModels_round_trips_through_its_reader(tmp_path):
    from hmcmt2d_amd import fileio
    from tests.helpers import make_problem
    mesh, data, inv, m = make_problem("tiny")
    n = len(inv.activeIdx)
    sk = S.sketchOf(chain_of(n, 22, 12).T, 12)
    lam, U, err = S.pcaFromSketch(sk, 3)
    stats = dict(sk, lam=lam, U=U, err=err)
    path = str(tmp_path / "post")
    got = fileio.getPCAModels(path, stats, mesh, inv)
    assert np.array_equal(got[0], lam) and np.array_equal(got[1], U) and np.array_equal(got[2], lam / sk["var"].sum()) and got[3] == err
    blam, bU, bexp, berr = fileio.readPCAModels(path, inv)
    assert np.array_equal(blam, lam) and np.array_equal(bexp, got[2]) and berr == err
    assert bU.shape == (3, n) and np.all(np.abs(bU - U) <= 0.5e-2 * np.abs(U) + 1e-12)      # (%4.2e: three digits)
    with pytest.raises(ValueError):
        fileio.getPCAModels(path, dict(stats, U=U[:, :-1]), mesh, inv)


def test_abi_of_the_new_symbols():
    """declared, exported, in the Python mirror; NULL context -> HMCMT_EINVAL before anything else; the ctypes mirror of
    hmcmt_sketch_info has the header's layout (a C program prints it)"""
    import ctypes
    import os
    import re
    import subprocess
    import tempfile
    from hmcmt2d_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = ctypes.CDLL(L.build_library())
    header = open(os.path.join(root, "include", "hmcmt.h")).read()
    for sym in L.CHAIN_SKETCH_SYMBOLS:
        assert re.search(r"extern int %s\(" % sym, header) and sym in L.PRODUCT_SYMBOLS and hasattr(so, sym)
    for sym in ("hmcmt_debug_chain_sketch", "hmcmt_debug_chain_sketch_time"):
        assert sym in L.DEBUG_SYMBOLS and hasattr(so, sym)
    lib = L.load_library()
    assert lib.hmcmt_chain_sketch_begin(None, 4, None) == -1 and lib.hmcmt_chain_sketch(None, None, None, None, None, 0) == -1
    assert lib.hmcmt_chain_pca(None, 2, None, None, None, None, 0) == -1
    fields = [f for f, _ in L.SketchInfo._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"hmcmt.h\"\nint main(void) { printf(\"%zu\", sizeof(hmcmt_sketch_info));\n" + \
           "".join(f'printf(" %zu", offsetof(hmcmt_sketch_info, {f}));\n' for f in fields) + "return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "a.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(d, "a.c"), "-o", os.path.join(d, "a")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "a")], text=True).split()]
    assert out[0] == ctypes.sizeof(L.SketchInfo) and out[1:] == [getattr(L.SketchInfo, f).offset for f in fields]
    assert "SKCH" in header and L.SKETCH_ELL_MAX == int(re.search(r"#define HMCMT_SKETCH_ELL_MAX (\d+)", header).group(1))


def test_sampler_refuses_sketch_without_the_device_chain_and_bad_values():
    from hmcmt2d_amd.structs import HMCPrior
    prior = HMCPrior(totalsamples=2, burninsamples=0, dt=0.01, timestep=[1, 1], sigBounds=[1e-4, 1.0], regParam=1.0)
    with pytest.raises(ValueError, match="sketch needs device_chain"):
        S.runHMCSampler(None, None, None, prior, sketch={})
    with pytest.raises(ValueError, match="sketch has no key"):
        S.runHMCSampler(None, None, None, prior, device_chain=True, sketch={"l": 4})
    for bad in ({"ell": 1}, {"ell": 65}, {"rank": 0}, {"rank": 33}):
        with pytest.raises(ValueError, match="sketch needs 2 <= ell"):
            S.runHMCSampler(None, None, None, prior, device_chain=True, sketch=bad)


def test_julia_binding_names_the_sketch_calls():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jl = open(os.path.join(root, "julia", "HMCMTHip.jl")).read()
    for name in ("chain_sketch_begin!", "chain_sketch", "chain_pca"):
        assert re.search(r"^function %s\(" % re.escape(name), jl, flags=re.M) and name in jl.split("const libhmcmt")[0]
    for sym in ("hmcmt_chain_sketch_begin", "hmcmt_chain_sketch", "hmcmt_chain_pca"):
        assert f"libhmcmt.{sym}(" in jl
    body = re.search(r"struct HmcmtSketchInfo\b(.*?)\nend", jl, flags=re.S).group(1)
    from hmcmt2d_amd import lib as L
    assert re.findall(r"^\s*([A-Za-z_]+)::", body, flags=re.M) == [f for f, _ in L.SketchInfo._fields_]
    assert "sketch::Union{Nothing,NamedTuple}=nothing" in jl


def test_parallel_sampler_gives_one_pivot_gathers_the_sketches_and_pools_them(monkeypatch):
    """Two chains in one process through parallelHMCSampler with sketch={...}: every chain receives the start model as its pivot, the
    sketches come back through the gather block bit for bit, and the first chain's sketch carries the pooled one, which is
    mergeSketches of the two and meets the guarantee for the concatenated rows."""
    from hmcmt2d_amd.structs import HMCPrior, HMCStatus
    from tests.helpers import make_problem
    mesh, data, inv, m = make_problem("tiny")
    nparam, ndata = len(inv.strModel), len(inv.obsData)
    ns, burn, ell = 40, 3, 4
    seen, chains = [], {}

    def fake_sampler(mesh_c, data_c, inv_c, prior_c, rng, ctx=None, **kw):
        """what runHMCSampler(device_chain=True, keep_samples=False, sketch=...) returns, from a synthetic chain round the start model"""
        c = len(seen)
        seen.append(kw)
        X = R.synthetic_chain(nparam, ns, seed=20 + c) + 2.0 + inv_c.strModel[None, :]
        chains[c] = X[burn:]
        st = HMCStatus(ns // 2, ns - ns // 2, np.arange(ns) % 2 == 0, rng.standard_normal((4, ns + 1)))
        st.moments = (ns - burn, X[burn:].mean(axis=0), ((X[burn:] - X[burn:].mean(axis=0)) ** 2).sum(axis=0))
        sk = S.sketchOf(X[burn:].T, kw["sketch"]["ell"], kw["sketch"]["pivot"])
        lam, U, err = S.pcaFromSketch(sk, kw["sketch"]["rank"])
        st.sketch = dict(sk, lam=lam, U=U, err=err)
        return np.zeros((nparam, 0)), st, np.zeros((ndata, 1), dtype=np.complex128)

    monkeypatch.setattr(S, "runHMCSampler", fake_sampler)
    prior = HMCPrior(totalsamples=ns, burninsamples=burn)
    hm, hs, hd = S.parallelHMCSampler(mesh, data, inv, prior, nchains=2, seed=3, context_factory=lambda *a: None, device_chain=True,
                                      keep_samples=False, sketch={"ell": ell, "rank": 3})
    assert len(seen) == 2
    for kw in seen:                                          # one pivot, the start model's, byte for byte
        assert kw["sketch"]["pivot"].tobytes() == np.asarray(inv.strModel, dtype=np.float64).tobytes() and kw["sketch"]["ell"] == ell
    for c in range(2):
        sk = hs[c].sketch
        ref = S.sketchOf(chains[c].T, ell, inv.strModel)
        assert all(sk[k] == ref[k] for k in ("count", "ell", "fill", "shrinks", "Delta", "pivot_given"))
        assert all(np.array_equal(sk[k], ref[k]) for k in ("x0", "tot", "q", "rows")) and sk["lam"] is not None
    # the gather block carries what the docstring says, and a block without the sketch is what it was
    plain = S.gatherBlockFields(nparam, 0, ns, ndata, True)
    assert S.gatherBlockFields(nparam, 0, ns, ndata, True, ell)[:len(plain)] == plain
    assert sum(size for _, size in S.gatherBlockFields(nparam, 0, ns, ndata, True, ell)[len(plain):]) == (2 * ell + 3) * nparam + 6
    unpacked = S._sketch_unpack(S._sketch_pack(hs[1].sketch, ell, nparam), nparam)
    assert all(np.array_equal(unpacked[k], hs[1].sketch[k]) for k in ("x0", "tot", "q", "rows", "mean", "var")) and unpacked["Delta"] == hs[1].sketch["Delta"]
    assert S._sketch_unpack(S._sketch_pack(None, ell, nparam), nparam) is None
    # the pooled sketch on the first chain
    merged = hs[0].sketch["merged"]
    assert "merged" not in hs[1].sketch
    ref = S.mergeSketches([S.sketchOf(chains[c].T, ell, inv.strModel) for c in range(2)])
    assert merged["count"] == 2 * (ns - burn) == ref["count"] and merged["nchains"] == 2 and merged["Delta"] == ref["Delta"]
    assert np.array_equal(merged["rows"], ref["rows"]) and np.array_equal(merged["tot"], ref["tot"])
    A = np.vstack([chains[0], chains[1]]) - np.asarray(inv.strModel)[None, :]
    s = check_guarantee(merged, A, "parallel merged")
    check_eigenvalues(merged["lam"], merged["err"], A, s, "parallel merged")
    assert merged["U"].shape == (3, nparam) and np.allclose(merged["explained"], merged["lam"] / merged["var"].sum())
    # without the keyword nothing of this happens
    seen.clear()
    monkeypatch.setattr(S, "runHMCSampler", lambda *a, **kw: (seen.append(kw), fake_plain(a[4]))[1])

    def fake_plain(rng):
        st = HMCStatus(1, 1, np.array([True, False]), rng.standard_normal((4, 3)))
        return np.zeros((nparam, 2)), st, np.zeros((ndata, 3), dtype=np.complex128)

    hm, hs, hd = S.parallelHMCSampler(mesh, data, inv, HMCPrior(totalsamples=2, burninsamples=0), nchains=2, seed=3, context_factory=lambda *a: None)
    assert all("sketch" not in kw for kw in seen) and all(h.sketch is None for h in hs)


def test_sampler_records_a_refused_pca_once_and_does_not_retry():
    """_Sketch.read: HMCMT_EBREAKDOWN from chain_pca is recorded in pca_error, lam and U stay None, one call; any other error raises"""
    from hmcmt2d_amd.lib import HmcmtError
    sk = S.sketchOf(chain_of(96, 22, 4).T, 4)

    class Ctx:
        calls, code = 0, -11

        def chain_sketch_info(self):
            return {k: sk[k] for k in ("count", "ell", "fill", "shrinks", "Delta", "pivot_given")}

        def chain_sketch(self):
            return dict(sk)

        def chain_pca(self, rank):
            Ctx.calls += 1
            raise HmcmtError(Ctx.code, "hmcmt_chain_pca: the components are not orthonormal")

    out = next(o for o in S.CHAIN_OUTPUTS if o.name == "sketch")
    got = out.read(Ctx(), (4, 8, None), None, None)
    assert Ctx.calls == 1 and got["lam"] is None and got["U"] is None and "not orthonormal" in got["pca_error"] and got["count"] == 22
    assert np.array_equal(got["rows"], sk["rows"])
    Ctx.code = -3
    with pytest.raises(HmcmtError):
        out.read(Ctx(), (4, 8, None), None, None)
