"""What the MAP optimiser costs beside its evaluations on one MI355X -> profiles/map_time.log.

  map     --iters iterations of hmcmt_map_step from the rough state at history 8 (m_ref = ln 0.01, lambda = 1, bounds [ln 1e-4, 0]):
          host clock round hmcmt_map_begin and the steps (every call is complete on return); ms per iteration and per evaluation.
  floor   the same number of evaluations through hmcmt_grad_device_async + hmcmt_wait in the same session: the model every step
          returned, evaluated as often as that step evaluated (the rejected trials' models are not kept; theirs lie on the segment
          to it).  What the L-BFGS launches, the record's copy and the host's decisions add is the difference.
  The two are interleaved --reps times; median [min - max].  Also Phi and D per iteration and the solver's iterations (forward /
  adjoint maximum over the systems) of each step's last evaluation: how soon the run leaves the rough state's 25-30-iteration regime.

    python scripts/gpu_map_time.py [cfg3] [--iters 20] [--reps 5]

One JSON line is appended to the log.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmcmt2d_amd.lib import HipContext, MAP_RUNNING, MAP_STATUS       # noqa: E402
from tests.helpers import make_problem                               # noqa: E402

LO, HI, LAMBDA, HISTORY = float(np.log(1e-4)), 0.0, 1.0, 8


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def map_run(ctx, m0, iters):
    t0 = time.perf_counter()
    recs = [ctx.map_begin(m0, LAMBDA, LO, HI, history=HISTORY)]
    models, its = [], []
    ms = (time.perf_counter() - t0) * 1e3
    while recs[-1]["status"] == MAP_RUNNING and len(recs) <= iters:
        t0 = time.perf_counter()
        recs.append(ctx.map_step())
        ms += (time.perf_counter() - t0) * 1e3
        st = ctx.stats()                                     # (outside the clock, like the read-out of the model)
        its.append((st["iters_fwd_max"], st["iters_adj_max"]))
        models.append(ctx.map_state()[0])
    return ms, recs, models, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="cfg3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    mesh, data, inv, m0 = make_problem(args.config)
    n = len(m0)
    ctx = HipContext(mesh, data, inv, device_id=0)
    ctx.set_prior(np.full(n, np.log(0.01)), inv.Wm, np.ones(n))
    _, recs, models, its = map_run(ctx, m0, args.iters)     # untimed: the models of the floor, the figures of the run
    evals = [r["nfevals"] for r in recs]
    d_models = [torch.tensor(m, device="cuda:0") for m in [np.clip(m0, LO, HI)] + models]
    d_g = torch.empty(n, dtype=torch.float64, device="cuda:0")
    t_map, t_floor = [], []
    for _ in range(args.reps):
        t_map.append(map_run(ctx, m0, args.iters)[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d_m, k in zip(d_models, evals):
            for _ in range(k):
                ctx.grad_device_async(d_m.data_ptr(), None, None, d_g.data_ptr())
                ctx.wait()
        t_floor.append((time.perf_counter() - t0) * 1e3)
    ctx.map_end()
    ctx.close()
    nev, nit = sum(evals), len(recs) - 1
    out = {"script": "gpu_map_time.py", "config": args.config, "nAC": n, "history": HISTORY, "iterations": nit, "evaluations": nev,
           "status": MAP_STATUS[recs[-1]["status"]], "reps": args.reps,
           "ms_per_iteration": summary([t / max(nit, 1) for t in t_map]), "ms_per_evaluation": summary([t / nev for t in t_map]),
           "floor_ms_per_evaluation": summary([t / nev for t in t_floor]),
           "overhead_ms_per_evaluation": summary([(a - b) / nev for a, b in zip(t_map, t_floor)]),
           "phi": [r["phi"] for r in recs], "D": [r["D"] for r in recs], "backtracks": [r["backtracks"] for r in recs[1:]],
           "nbound": [r["nbound"] for r in recs], "solver_iters_fwd_adj": its}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "map_time.log"), "a") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
