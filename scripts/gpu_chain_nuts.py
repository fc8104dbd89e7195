"""What a leaf of the device chain's No-U-turn sampler costs and what the sampler buys, on one MI355X -> profiles/chain_nuts.log
(DESIGN.md 4.9.8).

  cost    cfg3, bench.py's sampler settings near the true model (dt = 0.03), the seeded device chain without samples kept:
            fixed        hmcmt_chain_run at L = 8: ms per leapfrog step = ms per sample / 8
            nuts         hmcmt_chain_nuts_run at max_depth = 3: ms per leaf = wall time / leaves taken
            fixed_parent leg `fixed` on a build of the parent commit (--parent ROOT: a checkout of it with its library built)
          --reps interleaved repetitions, every measurement a process of its own, median [min - max].  One untimed sample through
          runHMCSampler sets the chain up (prior, begin, seed, the start gradient on the device); the timed window is the one library
          call for --samples samples behind it (0.5 s and more), so no begin, start evaluation or Python set-up is inside.  The
          nuts leg also reports the solver's iterations per solve of the leaves that follow a change of direction against the others
          (hmcmt_debug_nuts_iters): the extrapolated guess of such a leaf comes from the other end's path.
  effect  DESIGN 4.9.4's protocol: cfg2 from the golden chain's start, 200 warm-up and 200 counted samples, adapt={} -- the fixed-length
          chain (L drawn from the golden prior's range) against nuts={"max_depth": 8}, both with the library's generator.  Median and
          minimum ESS per gradient evaluation of the counted samples, cells whose lags ran out.  One seed's outcome.

    python scripts/gpu_chain_nuts.py [--reps 5] [--samples 50] [--parent build_ab/parent] [--skip-cost] [--skip-effect]

One JSON line is appended to the log.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, DT, RHOREF, DEPTH_COST, DEPTH_EFFECT = 8, 0.03, 100.0, 3, 8


def cost_worker(root, leg, ns, seed):
    sys.path.insert(0, root)
    import numpy as np
    from hmcmt2d_amd import sampler, synthetic as S
    from hmcmt2d_amd.lib import HipContext
    from hmcmt2d_amd.structs import HMCPrior
    from tests.helpers import make_problem
    kw = dict(device_chain=True, keep_samples=False, library_rng=(seed, 0))
    if leg == "nuts":
        kw["nuts"] = {"max_depth": DEPTH_COST}
    mesh, data, inv, _ = make_problem("cfg3")
    inv.strModel = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])

    def prior(n):
        return HMCPrior(totalsamples=n, burninsamples=0, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)

    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        sampler.runHMCSampler(mesh, data, inv, prior(1), np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, **kw)   # untimed; the chain stays
        if leg == "nuts":
            ctx.debug_nuts_iters(reset=True)
            t0 = time.perf_counter()
            recs, _, _ = ctx.chain_nuts_run(ns, DEPTH_COST, outputs=False)
            secs = time.perf_counter() - t0
            steps = sum(r["nleaves"] for r in recs)
        else:
            t0 = time.perf_counter()
            recs, _, _ = ctx.chain_run(ns, L, L, outputs=False)
            secs = time.perf_counter() - t0
            steps = ns * L
        out = {"seconds": secs, "samples": ns, "moved": sum(r["accepted"] for r in recs), "nfevals": sum(r["nfevals"] for r in recs),
               "steps": steps, "ms_per_step": 1e3 * secs / steps}
        assert out["nfevals"] == steps                      # (every timed sample starts from a gradient kept on the device)
        if leg == "nuts":
            out["leaves"] = steps
            out["stops"] = [r["stop"] for r in recs]
            out["iters"] = ctx.debug_nuts_iters()
    finally:
        ctx.close()
    print(json.dumps(out))


def effect_worker(root, leg):
    sys.path.insert(0, root)
    import numpy as np
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd import lib as Lib
    from hmcmt2d_amd.lib import HipContext
    from tests.helpers import make_problem
    from tests.golden.make_chain import chain_prior_of, start_model_of, SEED, RHOREF as GOLDEN_RHOREF
    mesh, data, inv, _ = make_problem("cfg2")
    prior = chain_prior_of("cfg2")
    prior.burninsamples, prior.totalsamples = 200, 400
    inv.strModel = start_model_of("cfg2", mesh, inv)
    kw = dict(device_chain=True, keep_samples=False, ess={}, adapt={}, library_rng=(SEED, 0))
    if leg == "nuts":
        kw["nuts"] = {"max_depth": DEPTH_EFFECT}
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        t0 = time.perf_counter()
        _, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(SEED), rhoref=GOLDEN_RHOREF, ctx=ctx, **kw)
        secs = time.perf_counter() - t0
    finally:
        ctx.close()
    if leg == "nuts":
        counted = int(st.nuts["nleaves"][200:].sum())        # (every counted sample starts from a gradient kept on the device)
    else:
        counted = sum(Lib.rng_draw(SEED, 0, t, int(prior.timestep[0]), int(prior.timestep[1]))[0] for t in range(200, 400))
    ess = np.asarray(st.ess["ess"], dtype=float)
    out = {"seconds": secs, "nfevals_total": int(prior.nfevals), "nfevals_counted": counted, "counted": int(st.ess["count"]),
           "moved_of_counted": int(st.acceptstats[200:].sum()), "median_ess": float(np.median(ess)), "min_ess": float(ess.min()),
           "median_ess_per_sample": float(np.median(ess) / st.ess["count"]), "median_ess_per_eval": float(np.median(ess) / counted),
           "min_ess_per_eval": float(ess.min() / counted), "lags_ran_out_cells": int((np.asarray(st.ess["window"]) < 0).sum()),
           "cells": int(ess.size), "dt_final": float(st.adapt["dt_final"]), "mean_alpha_counted": float(st.adapt["alpha"][200:].mean())}
    if leg == "nuts":
        n = st.nuts
        out.update(mean_leaves_counted=float(n["nleaves"][200:].mean()), max_depth=DEPTH_EFFECT,
                   stops_counted={str(k): int((n["stop"][200:] == k).sum()) for k in range(4)},
                   depth_counted={str(k): int((n["depth"][200:] == k).sum()) for k in range(DEPTH_EFFECT + 1)})
    else:
        out["timestep"] = [int(prior.timestep[0]), int(prior.timestep[1])]
    print(json.dumps(out))


def measure(root, args, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=root)
    if out.returncode != 0:
        raise RuntimeError(f"{args} of {root} failed ({out.returncode}): {out.stderr[-800:]}")
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--parent", default=None, help="root of a checkout of the parent commit with its library built")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-effect", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--what", default="cost")
    ap.add_argument("--seed", type=int, default=100)
    a = ap.parse_args()
    if a.worker:
        return effect_worker(os.path.abspath(a.root), a.leg) if a.what == "effect" else cost_worker(os.path.abspath(a.root), a.leg, a.samples, a.seed)
    line = {"script": "gpu_chain_nuts.py", "argv": sys.argv[1:]}
    if not a.skip_cost:
        plan = [("fixed", HERE, "fixed"), ("nuts", HERE, "nuts")] + ([("fixed", os.path.abspath(a.parent), "fixed_parent")] if a.parent else [])
        runs = {}
        for rep in range(a.reps):                           # interleaved: fixed, nuts, fixed_parent, fixed, ...
            for leg, root, key in plan:
                r = measure(root, ["--leg", leg, "--samples", str(a.samples), "--seed", str(100 + rep)], 900)
                runs.setdefault(key, []).append(r)
                print(f"cfg3 rep {rep} {key}: {r['ms_per_step']:.3f} ms per step, {r['seconds']:.2f} s timed", file=sys.stderr, flush=True)
        cost = {"config": "cfg3", "dt": DT, "L": L, "max_depth": DEPTH_COST, "samples_per_run": a.samples, "reps": a.reps, "ms_per_step": {}}
        for key, rs in runs.items():
            v = [r["ms_per_step"] for r in rs]
            cost["ms_per_step"][key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        cost["spread_ms"] = max(max(r["ms_per_step"] for r in rs) - min(r["ms_per_step"] for r in rs) for rs in runs.values())
        its = [r["iters"] for r in runs["nuts"]]
        tot = {k: (sum(i[k][0] for i in its), sum(i[k][1] for i in its)) for k in ("after_change", "other")}
        cost["leaves_per_run"] = [r["leaves"] for r in runs["nuts"]]
        cost["timed_seconds"] = {key: [round(r["seconds"], 3) for r in rs] for key, rs in runs.items()}
        cost["iterations_per_solve"] = {k: {"iterations": v[0], "solves": v[1], "mean": (v[0] / v[1] if v[1] else None)} for k, v in tot.items()}
        line["cost_cfg3"] = cost
    if not a.skip_effect:
        line["effect_cfg2"] = {leg: measure(HERE, ["--what", "effect", "--leg", leg], 1150) for leg in ("fixed", "nuts")}
    print(json.dumps(line))
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "chain_nuts.log"), "a") as log:
        log.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
