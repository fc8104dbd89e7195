"""Does a low-rank-plus-diagonal mass estimated from a pilot chain buy effective samples?  One seed's outcome on `tiny`, on one GPU
-> profiles/mass_lowrank_ess.log.  Not a test: nothing is asserted, the figures are reported as found.

  pilot   runHMCSampler(device_chain=True, keep_samples=True, ess={}) with the all-ones diagonal mass
  mass    sampler.lowRankMassFromSamples of the pilot's samples behind its burn-in
  second  the same sampler call, same seed, under mass_lowrank=(invM, U, lam)

Per chain: accepted, gradient evaluations, minimum and median over the cells of hmcstats.ess["ess"] per gradient evaluation.
--adapt: both chains warm up over their burn-in (adapt={"nwarmup": burnin}) -- the pilot its step size and its diagonal mass, the
second chain its step size alone beside the low-rank mass -- so that each mass runs at a step size of its own.

    python tests/tools/mass_lowrank_ess.py [--samples 400] [--burnin 100] [--rank 8] [--adapt]

One JSON line is appended to the log.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from hmcmt2d_amd import sampler                                      # noqa: E402
from hmcmt2d_amd.lib import HipContext                               # noqa: E402
from hmcmt2d_amd.structs import HMCPrior                             # noqa: E402
from tests.helpers import make_problem                               # noqa: E402

RHOREF, SEED = 122.0, 21


def chain(args, **kw):
    mesh, data, inv, _ = make_problem("tiny")
    prior = HMCPrior(totalsamples=args.samples, burninsamples=args.burnin, dt=0.02, timestep=[1, 3], sigBounds=[1e-4, 1.0], regParam=1.0)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        hm, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(SEED), rhoref=RHOREF, ctx=ctx, device_chain=True,
                                          keep_samples=True, ess={}, **kw)
    finally:
        ctx.close()
    ess = np.asarray(st.ess["ess"], dtype=np.float64)
    out = {"accepted": int(st.nAccept), "samples": args.samples, "counted": int(st.ess["count"]), "nfevals": int(prior.nfevals),
           "ess_min": float(ess.min()), "ess_median": float(np.median(ess)),
           "ess_min_per_eval": float(ess.min() / prior.nfevals), "ess_median_per_eval": float(np.median(ess) / prior.nfevals),
           "lags_ran_out_cells": int((np.asarray(st.ess["window"]) < 0).sum())}
    if st.adapt is not None:
        out["dt_final"] = float(st.adapt["dt_final"])
    return hm, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=400)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--adapt", action="store_true")
    args = ap.parse_args()
    kw = {"adapt": {"nwarmup": args.burnin}} if args.adapt else {}
    hm, pilot = chain(args, **kw)
    invM, U, lam = sampler.lowRankMassFromSamples(hm[:, args.burnin:], rank=args.rank)
    _, second = chain(args, mass_lowrank=(invM, U, lam), **kw)
    out = {"config": "tiny", "seed": SEED, "adapt": bool(args.adapt), "rank_kept": int(U.shape[0]), "lam": [float(v) for v in lam],
           "invM_min": float(invM.min()), "invM_median": float(np.median(invM)), "invM_max": float(invM.max()),
           "pilot_diagonal": pilot, "second_lowrank": second}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mass_lowrank_ess.log"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
