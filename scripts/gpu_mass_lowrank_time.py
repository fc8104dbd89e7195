"""What the low-rank-plus-diagonal mass costs on one MI355X -> profiles/mass_lowrank_time.log.

  apply       cfg3 (20000 cells): hmcmt_mass_apply(HMCMT_MASS_OP_INV) on device pointers under the diagonal mass, M = Wm and the
              low-rank mass at rank 8 and 32.  The call is complete on return, so the host clock around --calls calls holds the launches,
              the kernels and one stream synchronisation per call; microseconds per call, median [min - max] of --reps interleaved windows.
  trajectory  cfg3 near the true model, bench.py's sampler settings (L = 8, dt = 0.03): hmcmt_leapfrog_device + hmcmt_wait from
              p0 = sqrtM z under the same four masses; milliseconds per trajectory, median [min - max] of --reps interleaved runs, each
              kind behind one untimed trajectory on its context.  The trajectories differ with the mass (other moves, other solves), so
              this row is the price of a trajectory under the mass, not of the mass kernels alone.

    python scripts/gpu_mass_lowrank_time.py [--reps 5] [--calls 3000]

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

from hmcmt2d_amd import synthetic as S                                # noqa: E402
from hmcmt2d_amd.lib import HipContext, HMCMT_MASS_DIAGONAL, HMCMT_MASS_WM, HMCMT_MASS_OP_INV, HMCMT_MASS_OP_SQRT      # noqa: E402
from tests.helpers import make_problem                               # noqa: E402
from tests.mass_lowrank_ref import problem as lowrank_problem        # noqa: E402

L, DT = 8, 0.03
LO, HI = float(np.log(1e-4)), 0.0
KINDS = ["diagonal", "wm", "lowrank_r8", "lowrank_r32"]


def set_kind(ctx, kind, n):
    if kind == "diagonal":
        ctx.set_mass(HMCMT_MASS_DIAGONAL)
    elif kind == "wm":
        ctx.set_mass(HMCMT_MASS_WM)
    else:
        invM, U, lam, _ = lowrank_problem(n, int(kind.split("_r")[1]))
        ctx.set_mass_lowrank(invM, U, lam)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3000)
    args = ap.parse_args()
    import torch
    mesh, data, inv, _ = make_problem("cfg3")
    n = len(inv.strModel)
    m0 = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])
    mref = np.full(n, np.log(0.01))
    ctxs = {}
    out = {"config": "cfg3", "nAC": n, "L": L, "dt": DT, "reps": args.reps, "calls": args.calls, "apply_us": {}, "trajectory_ms": {}}
    try:
        for kind in KINDS:
            ctx = ctxs[kind] = HipContext(mesh, data, inv, device_id=0)
            ctx.set_prior(mref, inv.Wm, np.ones(n))
            set_kind(ctx, kind, n)
        # ---- apply ----
        x = torch.from_numpy(np.random.default_rng(1).standard_normal(n)).cuda()
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        times = {k: [] for k in KINDS}
        for rep in range(args.reps + 1):                             # (the first window of every kind warms up and is dropped)
            for kind in KINDS:
                ctx = ctxs[kind]
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    ctx.mass_apply_device(HMCMT_MASS_OP_INV, x.data_ptr(), y.data_ptr())
                if rep:
                    times[kind].append(1e6 * (time.perf_counter() - t0) / args.calls)
        out["apply_us"] = {k: summary(v) for k, v in times.items()}
        # ---- trajectory ----
        z = np.clip(np.random.default_rng(2).standard_normal(n), -2.5, 2.5)
        p0 = {k: ctxs[k].mass_apply(HMCMT_MASS_OP_SQRT, z) for k in KINDS}
        times = {k: [] for k in KINDS}
        for rep in range(args.reps + 1):
            for kind in KINDS:
                ctx = ctxs[kind]
                dm, dp = torch.from_numpy(m0.copy()).cuda(), torch.from_numpy(p0[kind].copy()).cuda()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nf = ctx.leapfrog_device(dm.data_ptr(), dp.data_ptr(), DT, L, 1.0, LO, HI)
                ctx.wait()
                if rep:
                    times[kind].append(1e3 * (time.perf_counter() - t0))
                assert nf == L + 1 and np.isfinite(dm.cpu().numpy()).all()
        out["trajectory_ms"] = {k: summary(v) for k, v in times.items()}
    finally:
        for ctx in ctxs.values():
            ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mass_lowrank_time.log"), "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
