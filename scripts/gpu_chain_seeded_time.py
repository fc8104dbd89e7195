"""Wall time per sample of the device chain with the host's random numbers and with the library's, interleaved in one session on one
MI355X -> profiles/chain_time.log.  The protocol is scripts/gpu_chain_time.py's: cfg3 then cfg5 with bench.py's settings near the true
model (L = 8, dt = 0.03), REPS interleaved repetitions, NS timed samples behind one untimed, median [min - max] per leg.

  (c)        runHMCSampler(device_chain=True, keep_samples=False): per sample nAC normals drawn by numpy and uploaded, two waits
  (g)        the same with library_rng=(seed, 0): the momenta drawn on the GPU, the run one hmcmt_chain_run, one wait per sample
  (c_parent) leg (c) on a build of the parent commit (--parent ROOT: a checkout of it with its library built), so that the comparison
             is against the parent and not against the code under test

Every measurement is a process of its own (this file with --worker, importing the package from the root it is given), so that the two
builds never share a process; the order is c, g, c_parent, c, g, ...  A gain of (g) is claimed only where (c) - (g) exceeds the
session's spread, the largest max - min of a leg.

    python scripts/gpu_chain_seeded_time.py [cfg3 cfg5] [--reps 5] [--samples 6] [--parent build_ab/parent]

One JSON line per configuration is appended to the log; every line names the build of each leg and carries its command line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, DT, RHOREF = 8, 0.03, 100.0
LEGS = {"c_device_chain_no_samples": dict(device_chain=True, keep_samples=False),
        "g_device_chain_no_samples_library_rng": dict(device_chain=True, keep_samples=False, library_rng=True)}


def worker(root, leg, name, ns, seed):
    """one measurement with the package of `root`: ms per sample of NS samples behind one untimed"""
    sys.path.insert(0, root)
    import copy
    import numpy as np
    from hmcmt2d_amd import sampler, synthetic as S
    from hmcmt2d_amd.lib import HipContext
    from hmcmt2d_amd.structs import HMCPrior
    from tests.helpers import make_problem
    kw = dict(LEGS[leg])
    if kw.get("library_rng"):
        kw["library_rng"] = (seed, 0)
    mesh, data, inv, _ = make_problem(name)
    inv.strModel = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])

    def prior(n):
        return HMCPrior(totalsamples=n, burninsamples=0, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)

    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        sampler.runHMCSampler(mesh, data, copy.deepcopy(inv), prior(1), np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, **kw)   # untimed
        t0 = time.perf_counter()
        _, st, _ = sampler.runHMCSampler(mesh, data, inv, prior(ns), np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, **kw)
        dt = time.perf_counter() - t0
    finally:
        ctx.close()
    print(json.dumps({"ms_per_sample": 1e3 * dt / ns, "accepted": int(st.nAccept)}))


def measure(root, leg, name, ns, seed):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--leg", leg, "--config", name, "--samples", str(ns),
           "--seed", str(seed)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    if out.returncode != 0:
        raise RuntimeError(f"{leg} of {root} failed ({out.returncode}): {out.stderr[-600:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["cfg3", "cfg5"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=6)
    ap.add_argument("--parent", default=None, help="root of a checkout of the parent commit with its library built")
    ap.add_argument("--this-build", default="this build", help="what the log calls the build under test")
    ap.add_argument("--parent-build", default="parent commit", help="what the log calls the parent's build")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--config", default=None)
    ap.add_argument("--seed", type=int, default=100)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.root), a.leg, a.config, a.samples, a.seed)
    plan = [(k, HERE, a.this_build) for k in LEGS]
    if a.parent:
        plan.append(("c_device_chain_no_samples", os.path.abspath(a.parent), a.parent_build))
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    log = open(os.path.join(HERE, "profiles", "chain_time.log"), "a")
    for name in a.configs:
        ms, acc = {}, {}
        for rep in range(a.reps):                           # interleaved: c, g, c_parent, c, g, ...
            for leg, root, build in plan:
                key = leg if root == HERE else leg + "_parent"
                r = measure(root, leg, name, a.samples, 100 + rep)
                ms.setdefault(key, []).append(r["ms_per_sample"]); acc[key] = r["accepted"]
                print(f"{name} rep {rep} {key} [{build}]: {r['ms_per_sample']:.3f} ms per sample", file=sys.stderr, flush=True)
        line = {"script": "gpu_chain_seeded_time.py", "config": name, "argv": sys.argv[1:], "L": L, "dt": DT, "samples_per_run": a.samples,
                "reps": a.reps, "ms_per_sample": {}}
        for (leg, root, build) in plan:
            key = leg if root == HERE else leg + "_parent"
            v = ms[key]
            line["ms_per_sample"][key] = {"build": build, "median": statistics.median(v), "min": min(v), "max": max(v), "accepted_last_run": acc[key]}
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        line["spread_ms"] = spread
        line["c_minus_g_ms"] = med["c_device_chain_no_samples"] - med["g_device_chain_no_samples_library_rng"]
        line["g_gain_resolved"] = bool(line["c_minus_g_ms"] > spread)
        if a.parent:
            p = med["c_device_chain_no_samples_parent"]
            line["c_parent_minus_g_ms"] = p - med["g_device_chain_no_samples_library_rng"]
            line["g_gain_over_parent_resolved"] = bool(line["c_parent_minus_g_ms"] > spread)
            line["c_minus_c_parent_ms"] = med["c_device_chain_no_samples"] - p
            line["c_within_spread_of_parent"] = bool(abs(line["c_minus_c_parent_ms"]) <= spread)
        print(json.dumps(line)); log.write(json.dumps(line) + "\n"); log.flush()


if __name__ == "__main__":
    main()
