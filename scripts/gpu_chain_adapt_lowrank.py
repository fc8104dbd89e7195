"""What the low-rank mass adaptation costs per step and per window end, and what it does, on one MI355X ->
profiles/chain_adapt_lowrank.log.  Every measurement is a process of its own (gpu_chain_nuts.py's pattern).

  cost    cfg3, bench.py's sampler settings near the true model (L = 8, dt = 0.03, the step size clipped to its start value so that the
          trajectories do not depend on the adaptation's step size): wall time per step of 30 steps of the device chain
          (keep_samples=False) inside ONE window (buffers 0 / 0, base 30), which closes behind the last step -- the diagonal adaptation
          on a build of the parent commit (--parent ROOT: a checkout of it with its library built) and on this build, and the low-rank
          upgrade at max_samples 64 (stride 1: a store launch in every step).  The low-rank row includes its one window end.  Median
          and min-max of --reps interleaved runs, each behind an untimed one-sample run on the same context.
  end     a window's end at cfg3 and cfg5 with n = 64 and n = 128 stored pairs: a seeded chain near the true model (L = 2, dt = 0.01: most
          steps move, so the pairs are distinct), ONE window of 128 steps, max_samples = n (n = 64: stride 2), every step timed on
          the host.  From hmcmt_debug_adapt_lowrank_time: ms of k_adapt_lr_mean + k_adapt_lr_gram and of k_adapt_lr_lift + k_adapt_lr_sign
          (HIP events), the host's wait for K; from the info: host_ms, dims, rank; and the closing step's wall time against the
          median step's.
  effect  DESIGN 4.9.4's protocol: cfg2 from the golden chain's start, 200 warm-up and 200 counted NUTS samples (max_depth 8), the
          library's generator, adapt={} against adapt={"lowrank": True}: accepted, final dt, rank and theta per window, median and
          minimum ESS per gradient evaluation of the counted samples, cells whose lags ran out.  One seed's outcome.

    python scripts/gpu_chain_adapt_lowrank.py [--reps 5] [--parent build_ab/parent] [--skip-cost] [--skip-end] [--skip-cfg5] [--skip-effect]

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
L, DT, RHOREF, NS = 8, 0.03, 100.0, 30
BASE = dict(mass=True, init_buffer=0, term_buffer=0, base_window=NS, dt_min=DT, dt_max=DT)
COST = {"diagonal": BASE, "lowrank_64": dict(BASE, lowrank={"max_samples": 64})}
END_STEPS, END_L, END_DT = 128, 2, 0.01


def cost_worker(root, leg, seed):
    sys.path.insert(0, root)
    import copy
    import numpy as np
    from hmcmt2d_amd import sampler, synthetic as S
    from hmcmt2d_amd.lib import HipContext
    from hmcmt2d_amd.structs import HMCPrior
    from tests.helpers import make_problem
    mesh, data, inv, _ = make_problem("cfg3")
    inv.strModel = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])
    prior = HMCPrior(totalsamples=NS, burninsamples=NS, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)
    warm = HMCPrior(totalsamples=1, burninsamples=1, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        sampler.runHMCSampler(mesh, data, copy.deepcopy(inv), warm, np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, device_chain=True,
                              keep_samples=False)                # untimed
        t0 = time.perf_counter()
        _, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, device_chain=True,
                                         keep_samples=False, adapt=COST[leg])
        secs = time.perf_counter() - t0
    finally:
        ctx.close()
    rows = (st.adapt.get("lowrank") or {}).get("windows") or []
    print(json.dumps({"ms_per_step": 1e3 * secs / NS, "accepted": int(st.nAccept), "window_end": rows[-1] if rows else None}))


def end_worker(root, cfg, n):
    sys.path.insert(0, root)
    import numpy as np
    from hmcmt2d_amd import synthetic as S
    from hmcmt2d_amd.lib import HipContext
    from tests.helpers import make_problem
    mesh, data, inv, _ = make_problem(cfg)
    start = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])
    nAC = len(start)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        ctx.set_prior(np.full(nAC, np.log(1.0 / RHOREF)), inv.Wm, np.ones(nAC))
        ctx.chain_begin(start, END_DT, 1.0, float(np.log(1e-4)), 0.0)
        ctx.chain_seed(7, 0)
        ctx.chain_adapt_begin(END_STEPS, init_buffer=0, term_buffer=0, base_window=END_STEPS, dt_min=END_DT, dt_max=END_DT)
        ctx.chain_adapt_lowrank(max_samples=n)
        walls, moved = [], 0
        for _ in range(END_STEPS):
            t0 = time.perf_counter()
            rec, _, _ = ctx.chain_sample(END_L, END_L, outputs=False)
            walls.append(1e3 * (time.perf_counter() - t0))
            moved += rec["accepted"]
        info, times = ctx.chain_adapt_lowrank_info(), ctx.debug_adapt_lowrank_time()
    finally:
        ctx.close()
    med = statistics.median(walls[:-1])
    print(json.dumps({"cfg": cfg, "cells": nAC, "n": n, "moved": moved, "info": info, "gram_us": 1e3 * times["gram_ms"], "lift_us": 1e3 * times["lift_ms"],
                      "wait_ms": times["wait_ms"], "check_ms": times["check_ms"], "median_step_ms": med, "closing_step_ms": walls[-1],
                      "window_end_wall_ms": walls[-1] - med}))


def effect_worker(root, leg):
    sys.path.insert(0, root)
    import numpy as np
    from hmcmt2d_amd import sampler
    from hmcmt2d_amd.lib import HipContext
    from tests.helpers import make_problem
    from tests.golden.make_chain import chain_prior_of, start_model_of, SEED, RHOREF as GOLDEN_RHOREF
    mesh, data, inv, _ = make_problem("cfg2")
    prior = chain_prior_of("cfg2")
    prior.burninsamples, prior.totalsamples = 200, 400
    inv.strModel = start_model_of("cfg2", mesh, inv)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        t0 = time.perf_counter()
        _, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(SEED), rhoref=GOLDEN_RHOREF, ctx=ctx, device_chain=True,
                                         keep_samples=False, ess={}, library_rng=(SEED, 0), nuts={"max_depth": 8},
                                         adapt={"lowrank": True} if leg == "lowrank" else {})
        secs = time.perf_counter() - t0
    finally:
        ctx.close()
    counted = int(st.nuts["nleaves"][200:].sum())
    ess = np.asarray(st.ess["ess"], dtype=float)
    out = {"seconds": secs, "nfevals_total": int(prior.nfevals), "nfevals_counted": counted, "counted": int(st.ess["count"]),
           "moved_of_counted": int(st.acceptstats[200:].sum()), "dt_final": float(st.adapt["dt_final"]),
           "mean_alpha_counted": float(st.adapt["alpha"][200:].mean()), "mean_leaves_counted": float(st.nuts["nleaves"][200:].mean()),
           "median_ess": float(np.median(ess)), "min_ess": float(ess.min()), "median_ess_per_eval": float(np.median(ess) / counted),
           "min_ess_per_eval": float(ess.min() / counted), "lags_ran_out_cells": int((np.asarray(st.ess["window"]) < 0).sum()), "cells": int(ess.size),
           "windows": st.adapt["windows"]}
    if leg == "lowrank":
        lr = st.adapt["lowrank"]
        out["lowrank_windows"] = [{k: w[k] for k in ("stored", "stride", "dims", "rank", "fallback", "theta_min", "theta_max", "host_ms")} for w in lr["windows"]]
        out["final_rank"], out["final_lam"] = int(len(lr["lam"])), [float(v) for v in lr["lam"]]
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
    ap.add_argument("--parent", default=None, help="root of a checkout of the parent commit with its library built")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-end", action="store_true")
    ap.add_argument("--skip-cfg5", action="store_true")
    ap.add_argument("--skip-effect", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--what", default="cost")
    ap.add_argument("--leg", default=None)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    if a.worker:
        root = os.path.abspath(a.root)
        return {"cost": lambda: cost_worker(root, a.leg, a.seed), "end": lambda: end_worker(root, a.leg, a.n),
                "effect": lambda: effect_worker(root, a.leg)}[a.what]()
    line = {"script": "gpu_chain_adapt_lowrank.py", "argv": sys.argv[1:]}
    if not a.skip_cost:
        plan = ([("diagonal", os.path.abspath(a.parent), "diagonal_parent")] if a.parent else []) + [("diagonal", HERE, "diagonal"), ("lowrank_64", HERE, "lowrank_64")]
        runs = {}
        for rep in range(a.reps):                           # interleaved
            for leg, root, key in plan:
                r = measure(root, ["--what", "cost", "--leg", leg], 600)
                runs.setdefault(key, []).append(r)
                print(f"cfg3 rep {rep} {key}: {r['ms_per_step']:.3f} ms per step, {r['accepted']} accepted", file=sys.stderr, flush=True)
        line["cost_cfg3"] = {"L": L, "dt": DT, "steps": NS, "reps": a.reps,
                             "ms_per_step": {k: {"median": statistics.median([r["ms_per_step"] for r in rs]), "min": min(r["ms_per_step"] for r in rs),
                                                 "max": max(r["ms_per_step"] for r in rs), "accepted": rs[-1]["accepted"], "window_end": rs[-1]["window_end"]}
                                             for k, rs in runs.items()}}
    if not a.skip_end:
        line["window_end"] = []
        for cfg in ["cfg3"] + ([] if a.skip_cfg5 else ["cfg5"]):
            for n in (64, 128):
                r = measure(HERE, ["--what", "end", "--leg", cfg, "--n", str(n)], 900)
                line["window_end"].append(r)
                print(f"{cfg} n {n}: gram {r['gram_us']:.0f} us, lift {r['lift_us']:.0f} us, host {r['info']['host_ms']:.1f} ms, wait {r['wait_ms']:.2f} ms, "
                      f"closing step {r['closing_step_ms']:.1f} ms against {r['median_step_ms']:.2f}, dims {r['info']['dims']}, rank {r['info']['rank']}", file=sys.stderr, flush=True)
    if not a.skip_effect:
        line["effect_cfg2"] = {leg: measure(HERE, ["--what", "effect", "--leg", leg], 1500) for leg in ("diagonal", "lowrank")}
        for leg, r in line["effect_cfg2"].items():
            print(f"cfg2 {leg}: {json.dumps(r)}", file=sys.stderr, flush=True)
    print(json.dumps(line))
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "chain_adapt_lowrank.log"), "a") as log:
        log.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
