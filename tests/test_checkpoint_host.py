"""Checkpoint and resume of the device chain without a GPU: the blob's container through hmcmt_chain_blob_info (which needs neither a
context nor a device) against tests/chain_blob_ref.py, which writes and reads it from the header's text alone; the bindings; and the
sampler's chain_checkpoint= keyword on the stand-in contexts of tests/test_chain_host.py, test_hist_host.py and test_acov_host.py,
subclassed here with chain_save / chain_restore over their Python state and a step-size warm-up."""
import copy
import ctypes
import os
import pickle
import re
import struct

import numpy as np
import pytest

from hmcmt2d_amd import lib as L
from hmcmt2d_amd import sampler
from hmcmt2d_amd.structs import HMCPrior
from tests import chain_blob_ref as B
from tests.conftest import ROOT
from tests.helpers import make_problem
from tests.test_acov_host import OracleAcovContext
from tests.test_chain_host import _same
from tests.test_hist_host import OracleHistContext

EINVAL = -1
NAC, NDATA = 5, 3


@pytest.fixture(scope="module", autouse=True)
def so():
    L.build_library()
    return L.load_library()


def info_code(blob):
    h = L.ChainBlobHeader()
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    return L.load_library().hmcmt_chain_blob_info(blob.ctypes.data, blob.size, ctypes.byref(h))


def sections(extra=()):
    rng = np.random.default_rng(1)
    chan = B.chan_payload(NAC, NDATA, nsamples=7, nmoments=4, seed=11, t=7, stream=2, seeded=1, m=rng.standard_normal(NAC),
                          pred=rng.standard_normal(2 * NDATA))
    return [("CHAN", chan), ("MASS", B.mass_payload(NAC))] + list(extra)


def good(extra=(), **kw):
    return B.write(sections(extra), NAC, NDATA, seeded=1, nsamples=7, nmoments=4, **kw)


# ---- 1. the container -----------------------------------------------------------------------------------------------------------------
def test_a_blob_written_from_the_headers_text_passes_with_every_field():
    dmom = struct.pack("<q", 4) + np.arange(4 * NDATA, dtype="<f8").tobytes()
    blob = good([("DMOM", dmom)])
    info = L.chain_blob_info(blob)
    assert info == {"version": 1, "total_bytes": blob.size, "nAC": NAC, "nData": NDATA, "mass_kind": 0, "seeded": 1, "nsamples": 7, "nmoments": 4,
                    "sections": [("CHAN", 96 + 8 * (3 * NAC + 2 * NDATA)), ("MASS", 32 + 8 * NAC), ("DMOM", len(dmom))]}
    assert L.chain_blob_info(blob.tobytes()) == info                      # (bytes are taken too)
    back = B.read(blob)
    assert back["order"] == ["CHAN", "MASS", "DMOM"] and back["sections"]["DMOM"] == dmom
    chan = B.read_chan(back["sections"]["CHAN"], NAC, NDATA)
    assert (chan["nsamples"], chan["nmoments"], chan["seed"], chan["t"], chan["stream"], chan["seeded"]) == (7, 4, 11, 7, 2, 1)
    # the checksum of the header's text on a known word sequence: two steps by hand
    h = ((0xcbf29ce484222325 ^ 1) * 0x100000001b3) % 2 ** 64
    assert B.checksum(struct.pack("<QQ", 1, 2)) == ((h ^ 2) * 0x100000001b3) % 2 ** 64


def test_every_damaged_container_is_refused():
    blob = good()
    assert info_code(blob) == 0
    n = len(sections())
    payload0 = 64 + 24 * n
    for at in (payload0 + 40, blob.size - 9, 30, 8, 64 + 3, 3):         # a payload byte (two places), header fields, the table, the magic
        bad = blob.copy(); bad[at] ^= 0x10
        assert info_code(bad) == EINVAL, at
    bad = blob.copy(); bad[-1] ^= 1                                       # the checksum itself
    assert info_code(bad) == EINVAL
    assert info_code(blob[:-8]) == EINVAL and info_code(blob[:64]) == EINVAL and info_code(blob[:8]) == EINVAL          # truncated
    assert info_code(np.concatenate([blob, np.zeros(8, dtype=np.uint8)])) == EINVAL                                       # trailing bytes
    assert info_code(good(version=2)) == EINVAL
    assert info_code(good(total=blob.size + 8)) == EINVAL
    s = sections()
    l0, l1 = len(s[0][1]), len(s[1][1])
    # (each of these carries a valid checksum: the table is what is wrong)
    assert info_code(good(table=[("CHAN", payload0 + 4, l0), ("MASS", payload0 + l0, l1)])) == EINVAL     # an offset that is no multiple of 8
    assert info_code(good(table=[("CHAN", payload0, l0), ("MASS", payload0 + l0 - 8, l1 + 8)])) == EINVAL  # overlapping sections
    assert info_code(good(table=[("CHAN", payload0, l0 - 8), ("MASS", payload0 + l0, l1)])) == EINVAL      # a gap
    assert info_code(good(table=[("CHAN", payload0, l0), ("MASS", payload0 + l0, l1 + 8)])) == EINVAL      # past the end
    assert info_code(good(table=[("MASS", payload0, l0), ("MASS", payload0 + l0, l1)])) == EINVAL          # no CHAN, a repeated tag
    assert info_code(B.write([("MASS", s[1][1]), ("DMOM", struct.pack("<q", 0) + bytes(32 * NDATA))], NAC, NDATA)) == EINVAL   # no CHAN
    assert info_code(B.write([s[1], s[0]], NAC, NDATA, seeded=1, nsamples=7, nmoments=4)) == EINVAL        # MASS in front of CHAN
    assert info_code(good([("XXXX", bytes(8))])) == EINVAL                                                 # an unknown tag
    assert info_code(good([("ADLR", bytes(168))])) == EINVAL                                               # ADLR without ADPT
    assert info_code(B.write(sections(), NAC, NDATA, seeded=1, nsamples=8, nmoments=4)) == EINVAL          # the header against CHAN
    assert info_code(B.write(sections(), NAC + 1, NDATA, seeded=1, nsamples=7, nmoments=4)) == EINVAL      # CHAN's length against nAC
    lib = L.load_library()
    h = L.ChainBlobHeader()
    assert lib.hmcmt_chain_blob_info(None, 0, ctypes.byref(h)) == EINVAL and lib.hmcmt_chain_blob_info(blob.ctypes.data, blob.size, None) == EINVAL
    with pytest.raises(L.HmcmtError):
        L.chain_blob_info(blob[:-8])


def test_calls_without_a_context_are_refused_and_the_symbols_are_bound(tmp_path):
    lib = L.load_library()
    n = ctypes.c_uint64()
    buf = np.zeros(64, dtype=np.uint8)
    assert lib.hmcmt_chain_save_size(None, ctypes.byref(n)) == EINVAL and lib.hmcmt_chain_save(None, buf.ctypes.data, 64, ctypes.byref(n)) == EINVAL
    assert lib.hmcmt_chain_restore(None, buf.ctypes.data, 64) == EINVAL
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hmcmt.h")).read(), flags=re.S)
    protos = {m.group(1): [p.strip().rsplit(" ", 1)[0].strip() for p in m.group(2).replace("\n", " ").split(",")]
              for m in re.finditer(r"^\s*extern\s+int\s+(hmcmt_chain_[a-z_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)}
    expect = {"hmcmt_chain_save_size": ["hmcmt_ctx*", "uint64_t*"], "hmcmt_chain_save": ["hmcmt_ctx*", "void*", "uint64_t", "uint64_t*"],
              "hmcmt_chain_restore": ["hmcmt_ctx*", "const void*", "uint64_t"],
              "hmcmt_chain_blob_info": ["const void*", "uint64_t", "hmcmt_chain_blob_header*"]}
    ctype = {"hmcmt_ctx*": "Ptr{Cvoid}", "uint64_t*": "Ref{UInt64}", "void*": "Ptr{UInt8}", "const void*": "Ptr{UInt8}", "uint64_t": "UInt64",
             "hmcmt_chain_blob_header*": "Ref{HmcmtChainBlobHeader}"}
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    for sym in L.CHAIN_SAVE_SYMBOLS:
        assert protos[sym] == expect[sym] and sym in L.PRODUCT_SYMBOLS and hasattr(lib, sym)
        fn = getattr(lib, sym)
        assert len(fn.argtypes) == len(expect[sym]) and fn.restype is ctypes.c_int
        m = re.search(r"@ccall libhmcmt\.%s\((.*?)\)::Cint" % sym, jl, flags=re.S)
        assert m, f"{sym} is not bound in julia/HMCMTHip.jl"
        assert re.findall(r"::\s*([A-Za-z0-9{}]+)", m.group(1)) == [ctype[t] for t in expect[sym]], sym
    exported = re.search(r"^export (.*?)\n\n", jl, flags=re.S | re.M).group(1)
    for name in ("chain_save", "chain_restore!", "chain_blob_info"):
        assert name in exported and ("function " + name) in jl
    # the header struct in C, Python and Julia
    import subprocess
    fields = [f for f, _ in L.ChainBlobHeader._fields_]
    src = tmp_path / "hdr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmcmt.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(hmcmt_chain_blob_header));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(hmcmt_chain_blob_header, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "hdr"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == ctypes.sizeof(L.ChainBlobHeader) and out[1:] == [getattr(L.ChainBlobHeader, f).offset for f in fields]
    body = re.search(r"struct HmcmtChainBlobHeader\b(.*?)\nend", jl, flags=re.S).group(1)
    assert re.findall(r"^\s*([A-Za-z_0-9]+)::", body, flags=re.M) == fields


# ---- 2. the sampler's keyword on a stand-in -----------------------------------------------------------------------------------------
class Crash(Exception):
    pass


class CheckpointContext(OracleHistContext, OracleAcovContext):
    """The stand-in with the histogram, data-moment and autocovariance accumulators, a step-size warm-up (dual averaging in Stan's
    form, no mass) and chain_save / chain_restore over all of that Python state.  die_at: the chain_step that raises (1-based)."""
    SAVED = ("chain", "prior", "hist_from", "hist_args", "dmom_from", "preds", "acov_from", "acov_args", "adapt")
    die_at = None

    def chain_begin(self, *a, **kw):
        self.adapt = None
        self.steps = 0
        return super().chain_begin(*a, **kw)

    def chain_adapt_begin(self, nwarmup, adapt_mass=0, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, **_):
        assert not adapt_mass
        self.adapt = dict(nwarmup=int(nwarmup), c=0, t=0, mu=float(np.log(10 * self.prior.dt)), s_bar=0.0, x_bar=0.0, alpha_last=0.0, alpha_sum=0.0,
                          active=True, delta=delta, gamma=gamma, t0=t0, kappa=kappa)

    def chain_adapt_info(self):
        a = self.adapt
        return dict(step=a["c"], nwarmup=a["nwarmup"], window_count=0, next_window_end=-1, active=int(a["active"]), windows_done=0,
                    dt=self.prior.dt, dt_bar=float(np.exp(a["x_bar"])) if a["t"] else self.prior.dt, mu=a["mu"], s_bar=a["s_bar"],
                    alpha_last=a["alpha_last"], alpha_sum=a["alpha_sum"])

    def chain_step(self, L, u, outputs=True):
        self.steps = getattr(self, "steps", 0) + 1
        if self.die_at is not None and self.steps >= self.die_at:
            raise Crash()
        out = super().chain_step(L, u, outputs)
        a = self.adapt
        if a is not None and a["active"]:
            alpha = 1.0 if out[0]["hdif"] > 0 else float(np.exp(out[0]["hdif"]))
            a["alpha_last"] = alpha; a["alpha_sum"] += alpha
            a["t"] += 1
            eta = 1.0 / (a["t"] + a["t0"])
            a["s_bar"] = (1 - eta) * a["s_bar"] + eta * (a["delta"] - alpha)
            x = a["mu"] - a["s_bar"] * np.sqrt(a["t"]) / a["gamma"]
            w = a["t"] ** -a["kappa"]
            a["x_bar"] = (1 - w) * a["x_bar"] + w * x
            self.prior.dt = float(np.exp(x))
            a["c"] += 1
            if a["c"] == a["nwarmup"]:
                self.prior.dt = float(np.exp(a["x_bar"]))
                a["active"] = False
        return out

    def chain_save(self):
        return np.frombuffer(pickle.dumps({k: getattr(self, k) for k in self.SAVED if hasattr(self, k)}), dtype=np.uint8).copy()

    def chain_restore(self, blob):
        assert self.chain is None, "behind set_prior, in place of chain_begin"
        self.saves_restored = getattr(self, "saves_restored", 0) + 1
        for k, v in pickle.loads(np.asarray(blob, dtype=np.uint8).tobytes()).items():
            setattr(self, k, v)
        self.cinv = copy.deepcopy(self.inv)
        self.cinv.refModel = self.mref.copy()
        self.chain["p"] = None                                            # (a momentum is not restored)


PRIOR = dict(totalsamples=9, burninsamples=3, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0])


def run(ctx, path=None, every=2, prior=None, seed=21, inv=None, mesh_data=None, **kw):
    mesh, data, inv0, _ = mesh_data
    kws = dict(hist={"targets": [3, 3, len(inv0.strModel) - 1, 0], "nbins": 17, "lo": -6.0, "hi": -3.5}, data_moments=True, ess={"maxlag": 3},
               adapt={"mass": False})
    kws.update(kw)
    p = HMCPrior(**PRIOR) if prior is None else prior
    out = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv0 if inv is None else inv), p, np.random.default_rng(seed), ctx=ctx,
                                device_chain=True, keep_samples=False, chain_checkpoint=path, chain_checkpoint_every=every, **kws)
    return out[1], p


def same_run(a, b):
    (sa, pa), (sb, pb) = a, b
    assert np.array_equal(sa.hmstats, sb.hmstats) and np.array_equal(sa.acceptstats, sb.acceptstats)
    assert (sa.nAccept, sa.nReject, pa.nfevals) == (sb.nAccept, sb.nReject, pb.nfevals)
    for f in ("moments", "hist", "dataMoments", "ess", "adapt"):
        assert getattr(sa, f) is not None and _same(getattr(sa, f), getattr(sb, f)), f


@pytest.fixture(scope="module")
def tiny():
    return make_problem("tiny")


@pytest.fixture(scope="module")
def full(tiny):
    mesh, data, inv, _ = tiny
    out = run(CheckpointContext(mesh, data, inv), mesh_data=tiny)
    assert set(out[0].acceptstats.tolist()) == {True, False} and out[0].adapt["dt_final"] != PRIOR["dt"]
    return out


@pytest.mark.parametrize("die_at", [4, 5, 9])
def test_a_killed_run_resumes_to_the_uninterrupted_one(tmp_path, tiny, full, die_at):
    """killed inside sample die_at (behind sample die_at - 1): the file is the flush behind the last even sample; the second run goes on
    from it -- inside the warm-up (3 samples) for die_at = 4 only behind it -- and ends as the uninterrupted run does, array for array"""
    mesh, data, inv, _ = tiny
    ck = str(tmp_path / "chain.ckpt")
    dying = CheckpointContext(mesh, data, inv)
    dying.die_at = die_at
    with pytest.raises(Crash):
        run(dying, ck, mesh_data=tiny)
    at = 2 * ((die_at - 1) // 2)
    assert int(np.load(ck)["it"]) == at and not os.path.exists(ck + ".tmp")
    ctx = CheckpointContext(mesh, data, inv)
    res = run(ctx, ck, mesh_data=tiny)
    same_run(res, full)
    assert ctx.saves_restored == 1 and ctx.steps == PRIOR["totalsamples"] - at and not hasattr(ctx, "hist_begins")
    assert int(np.load(ck)["it"]) == PRIOR["totalsamples"]                # (behind the last sample too: 9 is no multiple of 2)
    # a finished run's file resumes to the same result without a step
    ctx = CheckpointContext(mesh, data, inv)
    same_run(run(ctx, ck, mesh_data=tiny), full)
    assert getattr(ctx, "steps", 0) == 0


def test_a_warm_up_cut_in_its_middle(tmp_path, tiny, full):
    mesh, data, inv, _ = tiny
    ck = str(tmp_path / "chain.ckpt")
    dying = CheckpointContext(mesh, data, inv)
    dying.die_at = 3
    with pytest.raises(Crash):
        run(dying, ck, every=1, mesh_data=tiny)
    g = np.load(ck)
    assert int(g["it"]) == 2 and np.isnan(g["out_adapt_dt"][2:]).all() and not np.isnan(g["out_adapt_dt"][:2]).any()
    same_run(run(CheckpointContext(mesh, data, inv), ck, every=1, mesh_data=tiny), full)


def test_a_file_of_another_run_and_keep_samples_are_refused(tmp_path, tiny, full):
    mesh, data, inv, _ = tiny
    ck = str(tmp_path / "chain.ckpt")
    dying = CheckpointContext(mesh, data, inv)
    dying.die_at = 5
    with pytest.raises(Crash):
        run(dying, ck, mesh_data=tiny)
    fresh = lambda: CheckpointContext(mesh, data, inv)
    with pytest.raises(ValueError, match="different run"):
        run(fresh(), ck, prior=HMCPrior(**{**PRIOR, "dt": 0.021}), mesh_data=tiny)
    with pytest.raises(ValueError, match="different run"):
        run(fresh(), ck, seed=22, mesh_data=tiny)                          # another rhoref: another refModel
    inv2 = copy.deepcopy(inv)
    inv2.obsData = inv2.obsData * (1 + 1e-9)
    with pytest.raises(ValueError, match="different run"):
        run(fresh(), ck, inv=inv2, mesh_data=tiny)
    with pytest.raises(ValueError, match="different run"):
        run(fresh(), ck, hist={"targets": [3, 3, len(inv.strModel) - 1, 0], "nbins": 18, "lo": -6.0, "hi": -3.5}, mesh_data=tiny)
    with pytest.raises(ValueError, match="different run"):
        run(fresh(), ck, ess={"maxlag": 4}, mesh_data=tiny)
    with pytest.raises(ValueError, match="different run"):
        run(fresh(), ck, prior=HMCPrior(**{**PRIOR, "burninsamples": 4}), mesh_data=tiny)
    same_run(run(fresh(), ck, mesh_data=tiny), full)                       # (the refusals left the file alone)
    for kw in (dict(device_chain=True, keep_samples=True), dict(device_chain=False, keep_samples=True)):
        with pytest.raises(ValueError, match="chain_checkpoint"):
            sampler.runHMCSampler(mesh, data, copy.deepcopy(inv), HMCPrior(**PRIOR), np.random.default_rng(1), ctx=fresh(), chain_checkpoint=ck, **kw)
    with pytest.raises(ValueError, match="chain_checkpoint"):              # the host loop's keyword stays refused, and names the new one
        sampler.runHMCSampler(mesh, data, copy.deepcopy(inv), HMCPrior(**PRIOR), np.random.default_rng(1), ctx=fresh(), device_chain=True,
                              checkpoint=ck, checkpoint_every=1)


def test_a_crash_between_the_tmp_file_and_the_replace_leaves_the_older_file(tmp_path, tiny, full, monkeypatch):
    mesh, data, inv, _ = tiny
    ck = str(tmp_path / "chain.ckpt")
    real, calls = os.replace, []

    def replace(src, dst):
        calls.append(dst)
        if len(calls) == 2:
            raise Crash()
        return real(src, dst)

    monkeypatch.setattr(os, "replace", replace)
    with pytest.raises(Crash):
        run(CheckpointContext(mesh, data, inv), ck, mesh_data=tiny)
    monkeypatch.setattr(os, "replace", real)
    assert int(np.load(ck)["it"]) == 2 and os.path.exists(ck + ".tmp") and int(np.load(ck + ".tmp")["it"]) == 4
    same_run(run(CheckpointContext(mesh, data, inv), ck, mesh_data=tiny), full)
    assert not os.path.exists(ck + ".tmp")


def test_parallel_sampler_gives_each_chain_its_own_file(tmp_path, tiny):
    mesh, data, inv, _ = tiny
    ck = str(tmp_path / "run.ckpt")
    sampler.parallelHMCSampler(mesh, data, inv, HMCPrior(**{**PRIOR, "totalsamples": 3, "burninsamples": 1}), nchains=2, seed=3,
                               context_factory=lambda m, d, i, dev: CheckpointContext(m, d, i), device_chain=True, keep_samples=False,
                               chain_checkpoint=ck, chain_checkpoint_every=2)
    assert sorted(os.listdir(tmp_path)) == ["run.ckpt.chain1", "run.ckpt.chain2"]
    assert [int(np.load(f"{ck}.chain{c}")["it"]) for c in (1, 2)] == [3, 3]


def test_fingerprint_covers_the_chains_keywords_and_takes_arrays_of_any_shape():
    """the keywords' values in a canonical form: a list and an array of the same numbers are the same run, another value is another run;
    mass_lowrank = (invM[n], U[r, n], lam[r]) -- arrays of three shapes in one tuple -- is hashed array by array"""
    from types import SimpleNamespace
    inv = SimpleNamespace(obsData=np.ones(3), dataW=np.ones(3), refModel=np.zeros(5))
    prior = HMCPrior(totalsamples=4, burninsamples=1)
    base = dict(outputs={"hist": {"targets": [3, 3, 4, 0], "nbins": 17}, "adapt": {"lowrank": True}}, invM=None,
                mass_lowrank=(np.ones(5), np.zeros((2, 5)), np.ones(2)), library_rng=(1, 0), nuts=3)
    f = lambda **kw: sampler._chain_fingerprint(inv, prior, 5, **{**base, **kw})
    assert f() == f() == f(outputs={"hist": {"targets": np.array([3, 3, 4, 0], dtype=np.int32), "nbins": np.int64(17)}, "adapt": {"lowrank": True}})
    others = [f(outputs={"hist": {"targets": [3, 3, 4, 1], "nbins": 17}, "adapt": {"lowrank": True}}), f(outputs={"hist": base["outputs"]["hist"]}),
              f(mass_lowrank=(np.ones(5), np.zeros((2, 5)), 2 * np.ones(2))), f(mass_lowrank=None), f(invM=np.ones(5)), f(library_rng=(1, 1)),
              f(library_rng=None), f(nuts=4), f(nuts=None)]
    assert len(set(others + [f()])) == len(others) + 1
