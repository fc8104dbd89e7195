"""Times of the block Jacobian products:
python -m scripts.gpu_jvp_block_time [dprism3d cfg3 cfg5 ...] [--singles-only] [--parent=FILE]
-> one JSON line (kept in profiles/jvp_block_time.log).

Per mesh and nvec in {1, 2, 4, 8, 16}: milliseconds of jvp_block, jtvp_block and gn_hessvec_block through the _device entry points
with their iteration sums, beside -- same run, same directions -- nvec sequential single-direction _device calls, the yardstick.
Every figure is the median of 5 repetitions after a warm-up (wall clock around the synchronous calls), with the spread max - min
of the repetitions.  --singles-only times the yardstick alone: it also runs on a build without the block entry points (the parent's
figures: --parent=FILE puts that run's JSON line under "parent" in this one's).  dprism3d: the reference's example directory
(tests/golden/examples/dprism3d, 96 x 49 cells below the air, 11 frequencies) at the perturbed start model of tests/golden/example_dprism3d.npz."""
import json
import os
import sys
import time

import numpy as np
import torch

from hmcmt2d_amd.lib import HipContext
from hmcmt2d_amd.fileio import readstartupFile
from tests.helpers import make_problem

NVEC = (1, 2, 4, 8, 16)
REPS = 5


def timed(fn):
    fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(ts)), "spread": float(max(ts) - min(ts))}


def problem(name):
    if name == "dprism3d":
        golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
        mesh, data, inv, _ = readstartupFile(os.path.join(golden, "examples", "dprism3d", "startupfile"))
        return mesh, data, inv, np.load(os.path.join(golden, "example_dprism3d.npz"))["m1"]
    return make_problem(name)


def run(name, singles_only):
    mesh, data, inv, m = problem(name)
    ctx = HipContext(mesh, data, inv, warm_start="cold")
    dev = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(0)
    dm = torch.tensor(m, **dev)
    dV = torch.tensor(rng.standard_normal((max(NVEC), ctx.nAC)), **dev)
    dU = torch.tensor(rng.standard_normal((max(NVEC), 2 * ctx.nData)), **dev)
    dJV = torch.zeros((max(NVEC), 2 * ctx.nData), **dev)
    dG = torch.zeros((max(NVEC), ctx.nAC), **dev)
    ctx.linearize_device(dm.data_ptr())
    out = {"nAC": ctx.nAC, "nData": ctx.nData, "systems": ctx.S}
    for k in NVEC:
        e = {}

        def singles(fn, X, Y):
            for j in range(k):
                fn(X[j].data_ptr(), Y[j].data_ptr())
        e["jvp_singles"] = timed(lambda: singles(ctx.jvp_device, dV, dJV))
        e["jtvp_singles"] = timed(lambda: singles(ctx.jtvp_device, dU, dG))
        e["gn_singles"] = timed(lambda: singles(ctx.gn_hessvec_device, dV, dG))
        e["gn_single_iters"] = [ctx.jvp_stats["iters_fwd_sum"], ctx.jvp_stats["iters_adj_sum"]]
        if not singles_only:
            e["jvp_block"] = timed(lambda: ctx.jvp_block_device(dV.data_ptr(), k, dJV.data_ptr()))
            e["jvp_block_iters"] = ctx.block_stats["iters_fwd_sum"]
            e["jtvp_block"] = timed(lambda: ctx.jtvp_block_device(dU.data_ptr(), k, dG.data_ptr()))
            e["jtvp_block_iters"] = ctx.block_stats["iters_adj_sum"]
            e["gn_block"] = timed(lambda: ctx.gn_hessvec_block_device(dV.data_ptr(), k, dG.data_ptr()))
            e["gn_block_iters"] = [ctx.block_stats["iters_fwd_sum"], ctx.block_stats["iters_adj_sum"]]
            e["jvp_speedup"] = e["jvp_singles"]["ms"] / e["jvp_block"]["ms"]
            e["gn_speedup"] = e["gn_singles"]["ms"] / e["gn_block"]["ms"]
        out[str(k)] = e
    out["persist"] = ctx.persist_info()
    ctx.close()
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    singles_only = "--singles-only" in sys.argv
    parent = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--parent=")]
    names = args or ["dprism3d", "cfg3", "cfg5"]
    res = {"singles_only": singles_only, **{n: run(n, singles_only) for n in names}}
    if parent:
        res["parent"] = json.loads(open(parent[0]).read().strip().splitlines()[-1])
    print(json.dumps(res))
