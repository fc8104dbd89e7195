"""What a checkpoint of the device chain costs, on one MI355X -> profiles/chain_checkpoint.log (DESIGN 4.9.10 quotes it).  Every
measurement is a process of its own (this file with --worker), REPS repetitions, reported as median [min - max]; the chain is the
seeded one of scripts/gpu_chain_seeded_time.py (bench.py's settings near the true model, L = 8, dt = 0.03).

  save      blob size, hmcmt_chain_save and hmcmt_chain_restore (into the context whose chain was ended) for three chains behind
            two samples: `bare`; `outputs` = histograms of every cell (300 bins), autocovariances at maxlag 63, data moments and a
            low-rank adaptation of 64 pairs; `outputs_cov` = that plus 64 rows of cross moments
  flush     runHMCSampler(device_chain=True, keep_samples=False, library_rng=..., chain_checkpoint=...) with the `outputs` keywords:
            the wall time of one flush (blob, host part, file write, fsync, replace) beside the run's median sample
  step      hmcmt_chain_run's time per sample on this build and on a build of the parent commit (--parent ROOT: a checkout of it with
            its library built), interleaved; no save is called on either side.  Expected: this build's median inside the range the
            parent's runs span

    python scripts/gpu_chain_checkpoint.py [cfg3 cfg5] [--reps 5] [--legs save flush step] [--parent build_ab/parent]

One JSON line per configuration and leg is appended to the log; every line carries its command line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, DT, RHOREF = 8, 0.03, 100.0
CHAINS = ("bare", "outputs", "outputs_cov")


def setup(root, name):
    import numpy as np
    from hmcmt2d_amd import synthetic as S
    from hmcmt2d_amd.lib import HipContext
    from tests.helpers import make_problem
    mesh, data, inv, _ = make_problem(name)
    inv.strModel = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])
    return mesh, data, inv, HipContext(mesh, data, inv, device_id=0)


def worker_save(root, name, chain, seed):
    import numpy as np
    from hmcmt2d_amd.sampler import setMassMatrix
    mesh, data, inv, ctx = setup(root, name)
    try:
        n = len(inv.strModel)
        start = np.log(np.ones(n) / RHOREF)
        ctx.set_prior(start, inv.Wm, setMassMatrix(n, 1.0)[0])
        ctx.chain_begin(np.asarray(inv.strModel, dtype=np.float64), DT, 1.0, float(np.log(1e-4)), 0.0)
        ctx.chain_seed(seed, 0)
        if chain != "bare":
            ctx.chain_hist_begin(np.arange(n), 300, float(np.log(1e-4)), 0.0)
            ctx.chain_acov_begin(None, 63)
            ctx.chain_data_moments_begin()
            ctx.chain_adapt_begin(200, init_buffer=0, term_buffer=50, base_window=100)
            ctx.chain_adapt_lowrank(rank=8, max_samples=64)
        if chain == "outputs_cov":
            ctx.chain_cov_begin(np.linspace(0, n - 1, 64).astype(np.int64), 0)
        ctx.chain_run(2, L, L, outputs=False)
        t0 = time.perf_counter()
        blob = ctx.chain_save()
        t1 = time.perf_counter()
        ctx.chain_end()
        t2 = time.perf_counter()
        ctx.chain_restore(blob)
        t3 = time.perf_counter()
        assert (ctx.chain_save() == blob).all()
        rec = ctx.chain_run(1, L, L, outputs=False)[0][0]
    finally:
        ctx.close()
    print(json.dumps({"bytes": int(blob.size), "save_ms": 1e3 * (t1 - t0), "restore_ms": 1e3 * (t3 - t2), "nfevals_behind_restore": rec["nfevals"]}))


def worker_flush(root, name, seed, ns):
    import copy
    import numpy as np
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd.structs import HMCPrior
    mesh, data, inv, ctx = setup(root, name)
    flushes, real = [], sampler._ChainCheckpoint.save

    def timed(self, *a, **k):
        t0 = time.perf_counter()
        real(self, *a, **k)
        flushes.append(1e3 * (time.perf_counter() - t0))

    sampler._ChainCheckpoint.save = timed
    prior = HMCPrior(totalsamples=ns, burninsamples=ns, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "chain.ckpt")
        try:
            t0 = time.perf_counter()
            sampler.runHMCSampler(mesh, data, copy.deepcopy(inv), prior, np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, device_chain=True,
                                  keep_samples=False, library_rng=(seed, 0), hist={}, ess={"maxlag": 63}, data_moments=True,
                                  adapt={"lowrank": {"rank": 8, "max_samples": 64}, "init_buffer": 0, "term_buffer": 2, "base_window": ns - 2},
                                  chain_checkpoint=path, chain_checkpoint_every=ns // 2)
            total = 1e3 * (time.perf_counter() - t0)
        finally:
            ctx.close()
        size = os.path.getsize(path)
    print(json.dumps({"flush_ms": statistics.median(flushes), "flushes": len(flushes), "file_bytes": size,
                      "ms_per_sample_without_flushes": (total - sum(flushes)) / ns}))


def worker_step(root, name, seed, ns):
    import numpy as np
    from hmcmt2d_amd.sampler import setMassMatrix
    mesh, data, inv, ctx = setup(root, name)
    try:
        n = len(inv.strModel)
        ctx.set_prior(np.log(np.ones(n) / RHOREF), inv.Wm, setMassMatrix(n, 1.0)[0])
        ctx.chain_begin(np.asarray(inv.strModel, dtype=np.float64), DT, 1.0, float(np.log(1e-4)), 0.0)
        ctx.chain_seed(seed, 0)
        ctx.chain_run(1, L, L, outputs=False)               # untimed
        t0 = time.perf_counter()
        recs = ctx.chain_run(ns, L, L, outputs=False)[0]
        dt = time.perf_counter() - t0
    finally:
        ctx.close()
    print(json.dumps({"ms_per_sample": 1e3 * dt / ns, "accepted": sum(r["accepted"] for r in recs)}))


def measure(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root] + [str(a) for a in args]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root)
    if out.returncode != 0:
        raise RuntimeError(f"{args} of {root} failed ({out.returncode}): {out.stderr[-800:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["cfg3", "cfg5"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=6)
    ap.add_argument("--legs", nargs="*", default=["save", "flush", "step"])
    ap.add_argument("--parent", default=None, help="root of a checkout of the parent commit with its library built")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--config", default=None)
    ap.add_argument("--chain", default="bare")
    ap.add_argument("--seed", type=int, default=100)
    a = ap.parse_args()
    if a.worker:
        root = os.path.abspath(a.root)
        sys.path.insert(0, root)                            # (the package and the tests' problems of the build that is measured)
        if a.leg == "save":
            return worker_save(root, a.config, a.chain, a.seed)
        if a.leg == "flush":
            return worker_flush(root, a.config, a.seed, max(a.samples, 4))
        return worker_step(root, a.config, a.seed, a.samples)
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    log = open(os.path.join(HERE, "profiles", "chain_checkpoint.log"), "a")

    def emit(line):
        line = {"script": "gpu_chain_checkpoint.py", "argv": sys.argv[1:], "reps": a.reps, **line}
        print(json.dumps(line)); log.write(json.dumps(line) + "\n"); log.flush()

    for name in a.configs:
        if "save" in a.legs:
            for chain in CHAINS:
                rs = [measure(HERE, ["--leg", "save", "--config", name, "--chain", chain, "--seed", 100 + rep]) for rep in range(a.reps)]
                emit({"leg": "save", "config": name, "chain": chain, "bytes": rs[0]["bytes"], "save_ms": spread([r["save_ms"] for r in rs]),
                      "restore_ms": spread([r["restore_ms"] for r in rs]), "nfevals_behind_restore": rs[0]["nfevals_behind_restore"], "L": L})
        if "flush" in a.legs and name == "cfg3":
            rs = [measure(HERE, ["--leg", "flush", "--config", name, "--seed", 100 + rep, "--samples", a.samples]) for rep in range(a.reps)]
            emit({"leg": "flush", "config": name, "file_bytes": rs[0]["file_bytes"], "flush_ms": spread([r["flush_ms"] for r in rs]),
                  "ms_per_sample_without_flushes": spread([r["ms_per_sample_without_flushes"] for r in rs])})
        if "step" in a.legs:
            roots = [("this_build", HERE)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
            ms = {k: [] for k, _ in roots}
            for rep in range(a.reps):                       # interleaved: this build, parent, this build, ...
                for key, root in roots:
                    ms[key].append(measure(root, ["--leg", "step", "--config", name, "--seed", 100 + rep, "--samples", a.samples])["ms_per_sample"])
                    print(f"{name} rep {rep} {key}: {ms[key][-1]:.3f} ms per sample", file=sys.stderr, flush=True)
            line = {"leg": "step", "config": name, "L": L, "dt": DT, "samples_per_run": a.samples, "ms_per_sample": {k: spread(v) for k, v in ms.items()}}
            if a.parent:
                med = statistics.median(ms["this_build"])
                line["median_inside_the_parents_range"] = bool(min(ms["parent"]) <= med <= max(ms["parent"]))
            emit(line)


if __name__ == "__main__":
    main()
