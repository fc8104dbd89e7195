"""Times of the matrix-free Jacobian products: python -m scripts.gpu_jvp_time [cfg3 cfg5 ...] -> one JSON line.

Per call of linearize, jvp, jtvp and gn_hessvec through the _device entry points on the tests' golden models (best of 3 after a
warm-up, wall clock around the synchronous calls, with the products' iteration sums), beside -- same run, same build -- the
explicit route to J v (hmcmt_jacobian_device in row blocks + a device mat-vec) and a cold hmcmt_grad_device."""
import json
import sys
import time

import numpy as np
import torch

from hmcmt2d_amd.lib import HipContext
from tests.helpers import make_problem


def best(fn, n=3):
    fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def run(name):
    mesh, data, inv, m = make_problem(name)
    ctx = HipContext(mesh, data, inv, warm_start="cold")
    dev = dict(dtype=torch.float64, device="cuda")
    dm = torch.tensor(m, **dev)
    dv = torch.tensor(np.random.default_rng(0).standard_normal(ctx.nAC), **dev)
    du = torch.randn(2 * ctx.nData, **dev)
    djv, dg = torch.zeros(2 * ctx.nData, **dev), torch.zeros(ctx.nAC, **dev)
    dpred, dmis = torch.zeros(2 * ctx.nData, **dev), torch.zeros(1, **dev)
    out = {}
    out["grad_cold_ms"] = best(lambda: ctx.grad_device(dm.data_ptr(), dpred.data_ptr(), dmis.data_ptr(), dg.data_ptr()))
    st = ctx.stats()
    out["grad_iters"] = [st["iters_fwd_sum"], st["iters_adj_sum"]]
    out["linearize_ms"] = best(lambda: ctx.linearize_device(dm.data_ptr()))
    out["jvp_ms"] = best(lambda: ctx.jvp_device(dv.data_ptr(), djv.data_ptr()))
    out["jvp_iters"] = ctx.jvp_stats["iters_fwd_sum"]
    out["jtvp_ms"] = best(lambda: ctx.jtvp_device(du.data_ptr(), dg.data_ptr()))
    out["jtvp_iters"] = ctx.jvp_stats["iters_adj_sum"]
    out["gn_hessvec_ms"] = best(lambda: ctx.gn_hessvec_device(dv.data_ptr(), dg.data_ptr()))
    out["gn_iters"] = [ctx.jvp_stats["iters_fwd_sum"], ctx.jvp_stats["iters_adj_sum"]]
    blk = min(ctx.nData, 648)
    buf = torch.empty((blk, ctx.nAC), dtype=torch.complex128, device="cuda")
    ref = torch.zeros(ctx.nData, dtype=torch.complex128, device="cuda")
    cv = dv.to(torch.complex128)

    def explicit():
        for r0 in range(0, ctx.nData, blk):
            n = min(blk, ctx.nData - r0)
            ctx.jacobian_device(dm.data_ptr(), r0, n, buf.data_ptr())
            ref[r0:r0 + n] = buf[:n] @ cv
    out["explicit_Jv_ms"] = best(explicit, n=1 if name == "cfg5" else 3)
    out["explicit_over_jvp"] = out["explicit_Jv_ms"] / out["jvp_ms"]
    ctx.close()
    return out


if __name__ == "__main__":
    names = sys.argv[1:] or ["cfg3", "cfg5"]
    print(json.dumps({n: run(n) for n in names}))
