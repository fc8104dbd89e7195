"""What the chain's warm-up adaptation costs and what it does, on one MI355X -> profiles/chain_adapt.log.

  cost    cfg3, bench.py's sampler settings near the true model (L = 8, dt = 0.03): wall time per step of 30 steps of the device chain
          (keep_samples=False) without adaptation, with the step size adapted but clipped to the start value (dt_min = dt_max = dt:
          the trajectories are those of the first run, bit for bit) and with the mass windows on as well (buffers 3 / 3, base 5: a
          window Welford launch in 24 of the 30 steps, two mass updates).  Median of --reps runs, interleaved, each behind an untimed
          one-sample run on the same context.
  effect  cfg2 from the golden chain's start (tests/golden/make_chain.py), 200 warm-up steps plus 200 counted samples, with and
          without adapt={}: acceptance rate of the counted samples, final dt, range of the adapted invM, median ESS per counted
          sample over the cells (hmcmt_chain_ess, maxlag 63).  One seed's outcome.

    python scripts/gpu_chain_adapt.py [--reps 5] [--skip-effect]

One JSON line is appended to the log.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmcmt2d_amd import sampler, synthetic as S                      # noqa: E402
from hmcmt2d_amd.lib import HipContext                               # noqa: E402
from hmcmt2d_amd.structs import HMCPrior                             # noqa: E402
from tests.helpers import make_problem                               # noqa: E402
from tests.golden.make_chain import chain_prior_of, start_model_of, SEED, RHOREF as GOLDEN_RHOREF      # noqa: E402

L, DT, RHOREF, NS = 8, 0.03, 100.0, 30
COST = {"off": None,
        "dt_clipped": dict(mass=False, dt_min=DT, dt_max=DT),
        "dt_clipped_mass_windows": dict(mass=True, init_buffer=3, term_buffer=3, base_window=5, dt_min=DT, dt_max=DT)}


def cost_run(kw, seed):
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
                                         keep_samples=False, adapt=kw)
        dt = time.perf_counter() - t0
    finally:
        ctx.close()
    return 1e3 * dt / NS, st.nAccept, (st.adapt or {}).get("windows"), float(st.hmstats[3, -1])


def effect_run(adapt):
    mesh, data, inv, _ = make_problem("cfg2")
    prior = chain_prior_of("cfg2")
    prior.burninsamples, prior.totalsamples = 200, 400
    inv.strModel = start_model_of("cfg2", mesh, inv)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        t0 = time.perf_counter()
        _, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(SEED), rhoref=GOLDEN_RHOREF, ctx=ctx, device_chain=True,
                                         keep_samples=False, ess={}, adapt=adapt)
        secs = time.perf_counter() - t0
    finally:
        ctx.close()
    out = {"accepted_of_counted": int(st.acceptstats[200:].sum()), "counted": 200, "accepted_of_warmup": int(st.acceptstats[:200].sum()),
           "median_ess_per_sample": float(np.median(st.ess["ess"]) / st.ess["count"]), "lags_ran_out_cells": int((st.ess["window"] < 0).sum()),
           "seconds": secs, "nfevals": int(prior.nfevals), "dt_start": prior.dt}
    if adapt is not None:
        out.update(dt_final=float(st.adapt["dt_final"]), invM_min=float(st.adapt["invM"].min()), invM_median=float(np.median(st.adapt["invM"])),
                   invM_max=float(st.adapt["invM"].max()), windows=st.adapt["windows"], mean_alpha_warmup=float(st.adapt["alpha"][:200].mean()),
                   mean_alpha_counted=float(st.adapt["alpha"][200:].mean()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-effect", action="store_true")
    a = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = {"argv": sys.argv[1:], "cost_cfg3": {"L": L, "dt": DT, "steps": NS, "reps": a.reps, "ms_per_step": {}}}
    ms, last = {k: [] for k in COST}, {}
    for rep in range(a.reps):                              # interleaved: off, clipped, windows, off, ...
        for k, kw in COST.items():
            t, nacc, windows, h = cost_run(kw, 100 + rep)
            ms[k].append(t); last[k] = (nacc, windows, h)
            print(f"cfg3 rep {rep} {k}: {t:.3f} ms per step, accepted {nacc}", file=sys.stderr, flush=True)
    for k, v in ms.items():
        line["cost_cfg3"]["ms_per_step"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "accepted_last_run": last[k][0],
                                               "windows_last_run": last[k][1]}
    line["cost_cfg3"]["clipped_chain_is_the_plain_chain"] = bool(last["off"][2] == last["dt_clipped"][2])
    if not a.skip_effect:
        line["effect_cfg2"] = {"off": effect_run(None), "adapt": effect_run({})}
    print(json.dumps(line))
    with open(os.path.join(ROOT, "profiles", "chain_adapt.log"), "a") as log:
        log.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
