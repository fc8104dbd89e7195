"""Host-side logic: file formats, inverse set-up, and the sampler mirror driven by an oracle-backed
stand-in for the HIP context (so the O(nparam) host code is checked against the oracle on CPU)."""
import copy
import os
import numpy as np
import pytest

import hmcmt2d_amd as H
from hmcmt2d_amd import synthetic as S, sampler
from hmcmt2d_amd.structs import HMCPrior
from tests.helpers import make_problem, relmax, OracleContext


def test_model_and_data_file_round_trip(tmp_path):
    mesh, data, sig = S.make_config("tiny")
    mesh.sigma = sig
    H.writeEMModel2D(str(tmp_path / "m.mod"), mesh)
    back = H.readEMModel2D(str(tmp_path / "m.mod"))
    assert back.gridSize == mesh.gridSize
    assert np.allclose(back.yLen, mesh.yLen) and np.allclose(back.zLen, mesh.zLen)
    assert np.allclose(back.origin, mesh.origin)
    assert np.allclose(back.sigma, mesh.sigma, rtol=5e-3)          # %4.2e in the writer
    assert np.all(back.sigma[:mesh.gridSize[0] * len(mesh.airLayer)] == 1e-8)
    pred = (np.arange(len(data.rxID)) + 1) * (1e-3 - 2e-3j)
    H.writeMT2DData(str(tmp_path / "d.dat"), data, pred)
    d2, obs, err = H.readMT2DData(str(tmp_path / "d.dat"))
    assert d2.dataType == "Impedance" and d2.dataComp == ["ZXY", "ZYX"] and d2.compTE and d2.compTM
    assert np.array_equal(d2.freqID, data.freqID) and np.array_equal(d2.rxID, data.rxID)
    assert np.array_equal(d2.dtID, data.dtID) and d2.dataID.all()
    assert np.allclose(obs, pred, rtol=1e-6) and np.allclose(err, 0.03 * np.abs(pred), rtol=1e-6)
    assert np.allclose(d2.freqs, data.freqs, rtol=1e-4)


def test_startup_file_and_blank_lines(tmp_path):
    mesh, data, sig = S.make_config("tiny")
    mesh.sigma = np.where(sig > 1e-7, 0.01, sig)
    H.writeEMModel2D(str(tmp_path / "start.mod"), mesh)
    H.writeMT2DData(str(tmp_path / "obs.dat"), data, np.full(len(data.rxID), 0.1 + 0.1j))
    (tmp_path / "startupfile").write_text(
        "datafile:        obs.dat\n\nmodelfile:       start.mod\n# comment\nburninsamples:   5\ntotalsamples:    20\n"
        "resistivity:    1.0 1e4 0.05\ntimeinterval:   0.03\ntimestep:       6 10\nsmoothparameter: 2.0\n"
        "linearsolver: hip\n")
    m, d, inv, prior = H.readstartupFile(str(tmp_path / "startupfile"))
    assert prior.burninsamples == 5 and prior.totalsamples == 20 and prior.dt == 0.03
    assert prior.timestep == [6, 10] and prior.regParam == 2.0 and prior.linearSolver == "hip"
    assert np.allclose(prior.sigBounds, [1e-4, 1.0])
    ny, nzt = m.gridSize
    nair = len(m.airLayer)
    assert len(inv.strModel) == ny * (nzt - nair) and np.allclose(inv.strModel, np.log(0.01))
    assert np.all(inv.bgModel[:ny * nair] == 1e-8) and np.all(inv.bgModel[ny * nair:] == 0)


def test_inverse_setup_matches_oracle():
    from oracle import hmcmt_oracle as O
    mesh, data, inv, m = make_problem("tiny")
    ref = O.setupInverseDataModel(mesh, [S.SIG_AIR], 0, 0, inv.obsData, 1.0 / inv.dataW)
    assert np.array_equal(ref.activeIdx, inv.activeIdx) and np.array_equal(ref.bgModel, inv.bgModel)
    assert abs(ref.Wm - inv.Wm).max() == 0
    # top earth row keeps the extra diagonal term of its removed air neighbour
    ny = mesh.gridSize[0]
    d = inv.Wm.diagonal()
    assert d[ny + 3] == 4.0 and d[3] == 4.0 and d[0] == 3.0


def test_sampler_mirror_equals_oracle_chain():
    """runHMCSampler of the package (host logic) with an oracle-backed context reproduces the
    oracle's own restatement of the chain, sample for sample, under the same Generator."""
    from oracle import hmcmt_oracle as O
    mesh, data, inv, m = make_problem("tiny")
    prior = HMCPrior(totalsamples=3, burninsamples=1, dt=0.02, timestep=[2, 3], sigBounds=[1e-4, 1.0], regParam=1.0)
    # oracle chain
    mesh_o, inv_o, prior_o = copy.deepcopy(mesh), copy.deepcopy(inv), copy.deepcopy(prior)
    O.setupTensorMesh2D(mesh_o)
    mo, so, do = O.runHMCSampler(mesh_o, data, inv_o, prior_o, np.random.default_rng(5), dense_dbc=False)
    # package chain on the test double
    inv_p, prior_p = copy.deepcopy(inv), copy.deepcopy(prior)
    ctx = OracleContext(mesh, data, inv)
    mp, sp_, dp = sampler.runHMCSampler(copy.deepcopy(mesh), data, inv_p, prior_p, np.random.default_rng(5), ctx=ctx)
    assert relmax(mp, mo) < 1e-12 and relmax(dp, do) < 1e-12
    assert np.array_equal(sp_.acceptstats, so["acceptstats"]) and relmax(sp_.hmstats, so["hmstats"]) < 1e-12
    assert prior_p.nfevals == prior_o.nfevals
    # forward reuse: one forward at the start, none per sample (the oracle path does 1 + nsamples)
    assert ctx.nfwd == 1 and ctx.ngrad == prior_p.nfevals


def test_checkpointed_chain_resumes_bit_for_bit(tmp_path):
    """checkpoint / resume (not in the reference, which loses the run on a crash: SURVEY section 5): a chain killed in
    the middle of a sample and restarted with the same seed continues behind its last flushed sample and ends with
    exactly the samples, statistics and evaluation count of an uninterrupted run."""
    mesh, data, inv, m = make_problem("tiny")
    prior = HMCPrior(totalsamples=5, burninsamples=1, dt=0.02, timestep=[2, 3], sigBounds=[1e-4, 1.0], regParam=1.0)
    full = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), copy.deepcopy(prior), np.random.default_rng(5),
                                 ctx=OracleContext(mesh, data, inv))

    class Crash(Exception):
        pass

    class Dying(OracleContext):
        def grad(self, m):
            if self.ngrad >= 9:                    # somewhere inside the fourth trajectory
                raise Crash()
            return super().grad(m)

    ck = str(tmp_path / "chain.ckpt")
    with pytest.raises(Crash):
        sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), copy.deepcopy(prior), np.random.default_rng(5),
                              ctx=Dying(mesh, data, inv), checkpoint=ck, checkpoint_every=2)
    assert os.path.exists(ck) and int(np.load(ck)["it"]) == 2
    prior2 = copy.deepcopy(prior)
    ctx2 = OracleContext(mesh, data, inv)
    res = sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), prior2, np.random.default_rng(5), ctx=ctx2,
                                checkpoint=ck, checkpoint_every=2)
    assert np.array_equal(res[0], full[0]) and np.array_equal(res[2], full[2])
    assert np.array_equal(res[1].hmstats, full[1].hmstats) and np.array_equal(res[1].acceptstats, full[1].acceptstats)
    assert (res[1].nAccept, res[1].nReject) == (full[1].nAccept, full[1].nReject)
    assert ctx2.ngrad < prior2.nfevals                     # (the resumed process did only the remaining trajectories)
    assert int(np.load(ck)["it"]) == 5
    # the samples live in an append-only file of one record per sample (a flush writes the new samples only)
    nparam, ndata = full[0].shape[0], full[2].shape[0]
    assert os.path.getsize(ck + ".samples") == 5 * (nparam + 2 * ndata) * 8
    # a checkpoint of another run is refused: another reference model (seed), other sampler settings, other data
    with pytest.raises(ValueError):
        sampler.runHMCSampler(copy.deepcopy(mesh), data, copy.deepcopy(inv), copy.deepcopy(prior), np.random.default_rng(6),
                              ctx=OracleContext(mesh, data, inv), checkpoint=ck, checkpoint_every=2)
    for change in ("dt", "obs"):
        prior3, inv3 = copy.deepcopy(prior), copy.deepcopy(inv)
        if change == "dt":
            prior3.dt = 0.021
        else:
            inv3.obsData = inv3.obsData * (1 + 1e-9)
        with pytest.raises(ValueError):
            sampler.runHMCSampler(copy.deepcopy(mesh), data, inv3, prior3, np.random.default_rng(5),
                                  ctx=OracleContext(mesh, data, inv), checkpoint=ck, checkpoint_every=2)


def test_get_hamiltonian_without_reuse_repeats_forward():
    mesh, data, inv, m = make_problem("tiny")
    ctx = OracleContext(mesh, data, inv)
    prior = HMCPrior()
    inv.strModel = m.copy()
    sampler.compDataGradient(mesh, data, inv, prior, ctx)
    hp = H.initHMCParameter(len(m)); hp.invM[:] = 1; hp.momentum[:] = 0.5
    a = sampler.getHamiltonian(data, mesh, inv, prior, hp, ctx, reuse_forward=True)
    b = sampler.getHamiltonian(data, mesh, inv, prior, hp, ctx, reuse_forward=False)
    assert ctx.nfwd == 1 and abs(a[2] - b[2]) / abs(b[2]) < 1e-12
    assert abs(a[1] - 0.125 * len(m)) < 1e-9


def test_check_parameter_bound_matches_reference_loop():
    from oracle import hmcmt_oracle as O
    prior = HMCPrior(sigBounds=[0.01, 0.5])
    rng = np.random.default_rng(0)
    m = np.log(0.05) + 4.0 * rng.standard_normal(200)
    p = rng.standard_normal(200)
    a = sampler.checkParameterBound(m.copy(), p.copy(), prior)
    b = O.checkParameterBound(m.copy(), p.copy(), prior)
    assert np.allclose(a[0], b[0], atol=1e-14) and np.array_equal(a[1], b[1])
    with pytest.raises(FloatingPointError):
        sampler.checkParameterBound(np.array([np.nan]), np.array([1.0]), prior)


def test_posterior_and_outputs(tmp_path):
    mesh, data, inv, m = make_problem("tiny")
    prior = HMCPrior(burninsamples=2, totalsamples=6)
    rng = np.random.default_rng(1)
    hm = np.log(0.01) + 0.1 * rng.standard_normal((len(m), 6))
    mean, std = H.getPosteriorModel(hm, mesh, inv, prior, outdir=str(tmp_path))
    assert np.allclose(mean, hm[:, 2:].mean(axis=1)) and np.allclose(std, hm[:, 2:].std(axis=1))
    back = H.readEMModel2D(str(tmp_path / "meanModel.model"))
    assert back.gridSize == mesh.gridSize
    st = H.initHMCStatus(6); st.nAccept = 4; st.nReject = 2; st.acceptstats[:4] = True
    H.outputHMCSamples(hm, st, np.zeros((len(inv.obsData), 7), complex), ichain=3, cputime=1.5, outdir=str(tmp_path))
    lines = (tmp_path / "hmcsamples_id3.model").read_text().splitlines()
    assert len(lines) == 6 and len(lines[0].split()) == len(m)
    assert "nAccept:      4" in (tmp_path / "hmcstatistics_id3.log").read_text()


def test_only_hip_solver_is_accepted():
    mesh, data, inv, m = make_problem("tiny")
    with pytest.raises(ValueError):
        sampler.compDataGradient(mesh, data, inv, HMCPrior(linearSolver="mumps"))


def test_bench_gpus_n_spawns_one_rank_process_per_gpu():
    """`python bench.py --gpus 2` as a plain command (no torch.distributed.run, no WORLD_SIZE): the parent touches no GPU, starts
    two rank processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, hands rank 0's stdout through and exits non-zero when a
    rank fails -- in this GPU-less container both ranks get as far as "needs a GPU" (the reference's parallel entry is one call
    too: parallelHMC.jl:10-49).  With WORLD_SIZE set and a different --gpus the mismatch is an error, not a silent single rank."""
    import subprocess
    import sys
    from tests.conftest import HAVE_GPU
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if HAVE_GPU:
        pytest.skip("the spawn path is exercised for real on the GPU box by bench.py itself")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--no-cpu-baseline"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=root)
    assert r.returncode != 0
    assert r.stderr.count("bench.py needs a GPU") == 2, r.stderr[-1500:]
    assert "exited with" in r.stderr and r.stdout.strip() == ""
    env["WORLD_SIZE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--no-cpu-baseline"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=root)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_cu_shares_follow_the_chains_that_actually_run():
    """parallelHMCSampler(chains_per_gpu=c) with n local chains: shares = the largest of 4, 2, 1 that exceeds neither (ADVICE r5:
    chains_per_gpu = 4 with two local chains confined each chain to a quarter of every XCD and left half the GPU idle)."""
    from hmcmt2d_amd.sampler import cu_shares_for
    assert [cu_shares_for(4, n) for n in (1, 2, 3, 4, 7)] == [1, 2, 2, 4, 4]
    assert [cu_shares_for(2, n) for n in (1, 2, 3)] == [1, 2, 2]
    assert cu_shares_for(1, 8) == 1 and cu_shares_for(3, 8) == 2


@pytest.mark.parametrize("chains_per_gpu,nchains", [(3, 3), (3, 8), (5, 3), (5, 8), (8, 3), (8, 8)])
def test_chains_per_gpu_outside_1_2_4_runs_every_chain_on_its_shares(monkeypatch, chains_per_gpu, nchains):
    """chains_per_gpu = 3, 5, 8 (a warning, not an error): as many worker threads as CU shares, every chain on a share of its own
    while it runs -- more workers than shares popped an empty share list (IndexError) -- and every chain's result returned."""
    import threading
    import time
    import warnings
    mesh, data, inv, m = make_problem("tiny")
    prior = HMCPrior(totalsamples=2)
    nparam, ndata = len(inv.strModel), len(inv.obsData)
    shares = sampler.cu_shares_for(chains_per_gpu, nchains)
    lock, running, seen = threading.Lock(), [0, 0], []

    def factory(mesh_c, data_c, inv_c, dev):
        return object()

    def fake_run(mesh_c, data_c, inv_c, prior_c, rng, ctx=None, **kw):
        with lock:
            running[0] += 1
            running[1] = max(running[1], running[0])
        time.sleep(0.02)                                   # (long enough for the pool's other workers to be inside as well)
        with lock:
            running[0] -= 1
            seen.append(float(rng.standard_normal()))
        st = H.HMCStatus(1, 1, np.array([True, False]), np.zeros((4, 3)))
        return np.full((nparam, 2), float(len(seen))), st, np.zeros((ndata, 3), complex)

    monkeypatch.setattr(sampler, "runHMCSampler", fake_run)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hm, hs, hd = sampler.parallelHMCSampler(mesh, data, inv, prior, nchains=nchains, seed=3, context_factory=factory,
                                                chains_per_gpu=chains_per_gpu)
    assert len(hm) == len(hs) == len(hd) == nchains and len(seen) == nchains
    assert all(h is not None and h.shape == (nparam, 2) for h in hm)
    assert sorted(float(h[0, 0]) for h in hm) == list(range(1, nchains + 1))      # every chain's own result
    assert 1 <= running[1] <= shares


def test_bench_dump_writes_float64_npy_files_under_the_size_limit(tmp_path):
    """bench.py --dump-outputs DIR: one DIR/<name>.npy per output, float64, and a dump beyond the limit is refused."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_dump", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    arrays = {"model": np.arange(5, dtype=np.float32), "scal": np.array([1.5, 2.5])}
    bench.write_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["model.npy", "scal.npy"]
    back = np.load(tmp_path / "d" / "model.npy")
    assert back.dtype == np.float64 and np.array_equal(back, np.arange(5))
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "e"), {"big": np.zeros(9)}, limit=64)
    assert not (tmp_path / "e").exists()
