"""Cost of the explicit Jacobian at the headline (cfg3) and stress (cfg5) sizes, at the golden models of the tests:
python -m scripts.gpu_jacobian_time [reps]
Prints one JSON line: per config the milliseconds of one full J into device memory (hmcmt_jacobian_device), of one full J into
host memory (hmcmt_jacobian, cfg3; cfg5: the device J plus its copy to the host), of one hmcmt_sensitivity, the number of
batches (receivers) and the adjoint iterations per batch (mean over the batches of the summed iterations of the batch's systems,
and the largest single-system count)."""
import json
import sys
import time
import numpy as np
import torch
from hmcmt2d_amd.lib import HipContext
from tests.helpers import make_problem

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out = {}
for name in ("cfg3", "cfg5"):
    mesh, data, inv, m = make_problem(name)
    ctx = HipContext(mesh, data, inv)
    ctx.grad(m)
    dm = torch.tensor(m, dtype=torch.float64, device="cuda")
    dJ = torch.empty((ctx.nData, ctx.nAC), dtype=torch.complex128, device="cuda")

    def best(f):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return min(ts)

    dev_ms = best(lambda: ctx.jacobian_device(dm.data_ptr(), 0, ctx.nData, dJ.data_ptr()))
    st = dict(ctx.jac_stats)
    if name == "cfg3":
        host_ms = best(lambda: ctx.jacobian(m))
    else:
        host_ms = best(lambda: (ctx.jacobian_device(dm.data_ptr(), 0, ctx.nData, dJ.data_ptr()), dJ.cpu()))
    sens_ms = best(lambda: ctx.sensitivity(m))
    nb = len(np.unique(data.rxID))
    out[name] = dict(nData=ctx.nData, nAC=ctx.nAC, J_bytes=16 * ctx.nData * ctx.nAC, batches=nb,
                     ms_J_device=round(dev_ms, 2), ms_J_host=round(host_ms, 2), ms_host_copy=round(host_ms - dev_ms, 2),
                     ms_sensitivity=round(sens_ms, 2), iters_fwd_max=st["iters_fwd_max"],
                     adj_iters_sum_per_batch=round(st["iters_adj_sum"] / nb, 1), adj_iters_max=st["iters_adj_max"],
                     fallback_solves=st["fallback_solves"], persist=ctx.persist_info()["placement_fallbacks"] == 0)
    del dJ
    ctx.close()
    torch.cuda.empty_cache()
print(json.dumps(out))
