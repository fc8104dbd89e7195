"""Bits of the Jacobian products and of the explicit Jacobian, for comparing two builds:
python -m scripts.gpu_products_bits [tiny ragged ...] [--detail]
-> two JSON lines (kept in profiles/products_refactor_bits.log).  Run with HMCMT_LIB_PATH pointing at each build in turn; equal
lines mean equal bits.

Line 1, "products": per problem, preconditioner precision (mixed, fp64) and product (jvp, jtvp, gn_hessvec) one SHA-256 over the raw
output bytes of, in this order, wrt in (sigma, lnsigma) x [the single entry point, the block entry point at nvec = 1, 5, 9].  Seeds
are fixed; the single call and the block of one get direction 0 of the block of nine, the block of five its first five.  nvec = 5
is a partial chunk of the contraction kernels' eight directions, nvec = 9 a full chunk plus one.  --detail: every output's own
digest instead of the combined one.
Line 2, "jacobian": per problem the SHA-256 of the explicit Jacobian's rows (wrt sigma, then lnsigma) of the data of the first two
receivers, in data order."""
import hashlib
import json
import sys

import numpy as np

from hmcmt2d_amd.lib import HipContext
from tests import tipper_ref as TR
from tests.helpers import make_problem, ragged_problem, rhophase_problem

PROBLEMS = ("tiny", "ragged", "rhophase_tiny", "tipper", "cfg2", "cfg3")
NVEC = (1, 5, 9)


def problem(name):
    """the problems of tests/test_gpu_jvp.py's _case, without their oracle Jacobians"""
    if name.startswith("rhophase_"):
        return rhophase_problem(name.split("_")[1])[:4]
    if name == "tipper":
        return TR.tipper_problem("tiny", "Impedance", with_impedance=False)
    return ragged_problem(23, 17, 3, 3, 3, 4) if name == "ragged" else make_problem(name)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def products(ctx, m, detail):
    rng = np.random.default_rng(31)
    V = rng.standard_normal((max(NVEC), ctx.nAC))
    U = (rng.standard_normal((max(NVEC), ctx.nData)) + 1j * rng.standard_normal((max(NVEC), ctx.nData))).view(np.float64)
    out = {}
    for prec in ("mixed", "fp64"):
        ctx.set_options(fdm_precision=prec)
        ctx.linearize(m)
        for name, X, nout in (("jvp", V, 2 * ctx.nData), ("jtvp", U, ctx.nAC), ("gn_hessvec", V, ctx.nAC)):
            parts = {}
            for wrt in ("sigma", "lnsigma"):
                parts[f"{wrt}/single"] = ctx._product("hmcmt_" + name, np.ascontiguousarray(X[0]), wrt)
                for k in NVEC:
                    parts[f"{wrt}/block{k}"] = ctx._product_block(f"hmcmt_{name}_block", np.ascontiguousarray(X[:k]), wrt, nout)
            out[f"{prec}/{name}"] = {k: sha(a) for k, a in parts.items()} if detail else sha(*parts.values())
    return out


def jacobian_rows(ctx, m):
    rx = np.asarray(ctx.args.rxID)[:ctx.nData]
    mine = np.flatnonzero(np.isin(rx, np.unique(rx)[:2]))
    runs = np.split(mine, np.flatnonzero(np.diff(mine) != 1) + 1)
    ctx.set_options(fdm_precision="mixed")
    return sha(*[ctx.jacobian(m, rows=(int(r[0]), int(r[-1]) + 1), wrt=wrt) for wrt in ("sigma", "lnsigma") for r in runs])


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or PROBLEMS
    detail = "--detail" in sys.argv
    prod, jac = {}, {}
    for n in names:
        mesh, data, inv, m = problem(n)
        ctx = HipContext(mesh, data, inv)
        prod[n] = products(ctx, m, detail)
        jac[n] = jacobian_rows(ctx, m)
        ctx.close()
    print(json.dumps({"products": prod}))
    print(json.dumps({"jacobian": jac}))
