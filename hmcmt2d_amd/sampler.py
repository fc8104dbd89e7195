"""Host-side mirror of the reference sampler API on top of the HIP library.

Same function names, argument order and return values as HMCMT/src/HMCSampler/HMCSampler.jl:
`compDataGradient` (:277-330), `getHamiltonian` (:358-397), `proposeLeapfrog` (:206-269),
`getKineticEnergy` / `getKineticGradient` (:407-431), `getMomentumVector` (:441-453),
`setMassMatrix` (:463-489), `checkParameterBound` (:515-559), `runHMCSampler` (:72-196) and
`parallelHMCSampler` (parallelHMC.jl:10-49).  The only compute they do themselves is O(nparam)
vector arithmetic; the forward / adjoint solves go through `HipContext` (include/hmcmt.h).

Differences that are deliberate and documented:
  * random numbers come from an explicit `numpy.random.Generator` (the reference uses Julia's
    unseeded global RNG, so sample-level parity with it is impossible by construction);
  * `getHamiltonian` reuses the forward response of the last gradient evaluation when it was
    computed at the same model (the reference repeats an identical forward solve,
    HMCSampler.jl:251 vs :364); `reuse_forward=False` restores the reference's cost structure;
  * a non-finite model raises instead of spinning forever in the bound reflection (:546-548).
"""
from __future__ import annotations

import os
import time
import weakref
import numpy as np

from .lib import HipContext
from .structs import HMCParameter, HMCStatus, initHMCParameter, initHMCStatus

_contexts: dict = {}          # (id(invParam), device) -> HipContext; entries die with their InvDataModel (weakref.finalize)


def default_device() -> int:
    """The GPU of this process: an explicit HMCMT_DEVICE first (the same precedence as julia/HMCMTHip.jl's
    defaultDevice), else LOCAL_RANK under torch.distributed.run / torchrun (one process per GPU), else 0.  The
    reference's counterpart is the worker id of `pmap` (parallelHMC.jl:23-40)."""
    for var in ("HMCMT_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v not in (None, ""):
            return int(v)
    return 0


def _drop_context(key):
    ctx = _contexts.pop(key, None)
    if ctx is not None:
        ctx.close()


def get_context(mtMesh, mtData, invParam, device_id=None, **opts) -> HipContext:
    """One HIP context per (InvDataModel, device), created lazily on `device_id` (default: this process's GPU,
    `default_device()`).  The cache entry is tied to the life of `invParam` (a recycled id() can never return a
    context built for another problem) and is rebuilt when different solver options are requested."""
    dev = default_device() if device_id is None else int(device_id)
    key = (id(invParam), dev)
    ctx = _contexts.get(key)
    if ctx is not None and (ctx._owner() is not invParam or (opts and opts != ctx._opts)):
        _drop_context(key)
        ctx = None
    if ctx is None:
        ctx = HipContext(mtMesh, mtData, invParam, device_id=dev, **opts)
        ctx._cache = None
        ctx._opts = dict(opts)
        ctx._owner = weakref.ref(invParam)
        ctx.device_id = dev
        _contexts[key] = ctx
        weakref.finalize(invParam, _drop_context, key)
    return ctx


def cu_shares_for(chains_per_gpu, nlocal):
    """CU shares (hmcmt_next_cu_share) for `nlocal` chains of this rank under chains_per_gpu: the largest of 4, 2, 1 that exceeds
    neither -- every share in use, none idle (parallelHMC.jl:23-45 runs np chains over fewer workers the same way)."""
    return max(sh for sh in (4, 2, 1) if sh <= max(1, min(int(chains_per_gpu), int(nlocal))))


def release_context(invParam, device_id=None):
    for key in [k for k in _contexts if k[0] == id(invParam) and (device_id is None or k[1] == int(device_id))]:
        _drop_context(key)


def _check_solver(hmcprior):
    if hmcprior.linearSolver.lower() not in ("", "hip"):
        raise ValueError(f"linearsolver {hmcprior.linearSolver!r}: this package only has the HIP path "
                         "(use `linearsolver: hip`)")


# --------------------------------------------------------------------------------------------
def findMAP(mtMesh, mtData, invParam, hmcprior, m0=None, ctx: HipContext | None = None, maxiter=50, **options):
    """The MAP model of D + M on the GPU (hmcmt_map_*: projected L-BFGS, model, gradient and history device-resident) -> (model,
    MAPStatus).  Starts from invParam.strModel when m0 is None; regParam and the bounds are hmcprior's; options: history,
    max_backtracks, c1, shrink, curv_eps, gtol.  A run may end STALLED well above the minimum where the reference's gradient is not the
    derivative of its misfit (boundaries close to the receivers); it never accepts a rise.  To start a chain at the model, write it into
    invParam.strModel, from which runHMCSampler runs its first trajectory; fileio's model writer saves it like any other model."""
    from .lib import MAP_STATUS, MAP_RUNNING, map_options
    from .structs import MAPStatus
    _check_solver(hmcprior)
    map_options(**options)                                   # (ValueError before anything touches the device)
    if int(maxiter) < 0:
        raise ValueError("maxiter must not be negative")
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    nparam = len(invParam.strModel)
    start = np.asarray(invParam.strModel if m0 is None else m0, dtype=np.float64)
    ctx.set_prior(invParam.refModel, invParam.Wm, np.ones(nparam))
    lo, hi = np.log(hmcprior.sigBounds[0]), np.log(hmcprior.sigBounds[1])
    recs = [ctx.map_begin(start, hmcprior.regParam, lo, hi, **options)]
    if recs[0]["status"] == MAP_RUNNING and maxiter > 0:
        recs += ctx.map_run(int(maxiter))
    model, _, pred = ctx.map_state()
    ctx.map_end()
    col = lambda k, t=float: np.array([r[k] for r in recs], dtype=t)
    st = MAPStatus(MAP_STATUS[recs[-1]["status"]], int(recs[-1]["iter"]), int(col("nfevals", int).sum()), col("phi"), col("D"), col("M"),
                   col("pg_inf"), col("pg_2"), col("alpha"), col("backtracks", int), col("resets", int), col("npairs", int),
                   col("pair_stored", bool), col("nbound", int), col("nfevals", int), pred)
    return model, st


# --------------------------------------------------------------------------------------------
def compDataGradient(mtMesh, mtData, invParam, hmcprior, ctx: HipContext | None = None):
    """m = invParam.strModel -> (predData, dataMisfit, dataGrad)."""
    _check_solver(hmcprior)
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    m = np.asarray(invParam.strModel, dtype=np.float64)
    pred, misfit, grad = ctx.grad(m)
    sigma = invParam.bgModel.copy()
    sigma[invParam.activeIdx] += np.exp(m)
    mtMesh.sigma = sigma                                   # HMCSampler.jl:294
    ctx._cache = (m.copy(), pred, misfit)
    return pred, misfit, grad


def compJacMat(mtMesh, mtData, invParam, ctx: HipContext | None = None, wrt="sigma"):
    """The data Jacobian at m = invParam.strModel (compJacMat.jl): (nData, nAC), d data / d sigma of the active cells
    (wrt="lnsigma": d / d ln sigma); complex for DataType Impedance, real for Rho_Pha."""
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    return ctx.jacobian(np.asarray(invParam.strModel, dtype=np.float64), wrt=wrt)


def compJacTMat(mtMesh, mtData, invParam, ctx: HipContext | None = None, wrt="sigma"):
    """J^T as the reference's compJacTMat.jl orients it: (nAC, nData)."""
    return compJacMat(mtMesh, mtData, invParam, ctx=ctx, wrt=wrt).T


def compJacMatVec(mtMesh, mtData, invParam, v, ctx: HipContext | None = None, wrt="sigma"):
    """compJacMat(m) @ v at m = invParam.strModel without forming J (the tangent-linear route: one solve): the data layout of
    predData.  Linearises the context at m; further products at the same point: ctx.jvp / ctx.jtvp / ctx.gn_hessvec."""
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    ctx.linearize(np.asarray(invParam.strModel, dtype=np.float64))
    return ctx.jvp(np.asarray(v, dtype=np.float64), wrt=wrt)


def compJacTMatVec(mtMesh, mtData, invParam, datVec, ctx: HipContext | None = None, wrt="sigma"):
    """real(compJacTMatVec(.., datVec, ..)) of the reference (compJacTMatVec.jl:8) for a free data vector: Re(J^T conj(datVec))
    at m = invParam.strModel, [nAC].  compDataGradient's gradient is exp(m) * compJacTMatVec(.., dataW**2 * (pred - obs))."""
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    ctx.linearize(np.asarray(invParam.strModel, dtype=np.float64))
    return ctx.jtvp(datVec, wrt=wrt)


def compJacMatMat(mtMesh, mtData, invParam, V, ctx: HipContext | None = None, wrt="sigma"):
    """compJacMat(m) @ V.T for the rows of V (nvec, nAC) at m = invParam.strModel, (nvec, nData): the whole block in one solve
    (HipContext.jvp_block).  Linearises the context at m; further blocks at the same point: ctx.jvp_block / ctx.jtvp_block /
    ctx.gn_hessvec_block."""
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    V = HipContext.block_input(V, ctx.nAC, "compJacMatVec")
    ctx.linearize(np.asarray(invParam.strModel, dtype=np.float64))
    return ctx.jvp_block(V, wrt=wrt)


def compJacTMatMat(mtMesh, mtData, invParam, U, ctx: HipContext | None = None, wrt="sigma"):
    """Re(J^T conj(U_j)) for the rows of U (nvec, nData) at m = invParam.strModel, (nvec, nAC): one adjoint-type solve for the
    block (HipContext.jtvp_block)."""
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    U = HipContext.block_input(U, ctx.nData, "compJacTMatVec", complex_in=True)
    ctx.linearize(np.asarray(invParam.strModel, dtype=np.float64))
    return ctx.jtvp_block(U, wrt=wrt)


def compDataMisfit(predData, invParam):
    res = invParam.dataW * (predData - invParam.obsData)
    return 0.5 * float(np.real(np.vdot(res, res)))


def getKineticEnergy(momentum, hmcParam: HMCParameter):
    return 0.5 * float(np.dot(momentum, hmcParam.invM * momentum))


def getKineticGradient(momentum, hmcParam: HMCParameter):
    return hmcParam.invM * momentum


def getMomentumVector(nparam, hmcParam: HMCParameter, rng):
    mp = np.clip(rng.standard_normal(nparam), -2.5, 2.5)   # clipped N(0,1), HMCSampler.jl:444-447
    return hmcParam.sqrtM * mp


def setMassMatrix(nparam, scaling=1.0):
    """setMassMatrix(nparam, scaling) -> (invM, sqrtM) diagonals (HMCSampler.jl:463-474); setMassMatrix(invParam, ctx) -> the
    non-diagonal mass M = Wm (:478-489) as operators of `ctx` (hmcmt_set_mass / hmcmt_mass_apply): invM * p = Wm^-1 p,
    sqrtM * z = L z with L = chol(Wm).L.  The second form registers invParam's prior on ctx (refModel, Wm) and factors Wm."""
    if hasattr(nparam, "Wm"):
        return _wm_mass(nparam, scaling)
    mass = scaling * np.ones(nparam)
    return 1.0 / mass, np.sqrt(mass)


class MassOperator:
    """One half of the non-diagonal mass matrix: `op * v` applies M^-1 (op = HMCMT_MASS_OP_INV) or L (HMCMT_MASS_OP_SQRT)
    through the context, so getKineticEnergy, getKineticGradient and getMomentumVector run unchanged."""

    def __init__(self, ctx, op):
        self.ctx, self.op = ctx, op

    def __mul__(self, v):
        return self.ctx.mass_apply(self.op, np.asarray(v, dtype=np.float64))


def _wm_mass(invParam, ctx):
    from .lib import HMCMT_MASS_WM, HMCMT_MASS_OP_INV, HMCMT_MASS_OP_SQRT
    n = len(invParam.strModel)
    ctx.set_prior(invParam.refModel, invParam.Wm, np.ones(n))
    ctx.set_mass(HMCMT_MASS_WM)
    return MassOperator(ctx, HMCMT_MASS_OP_INV), MassOperator(ctx, HMCMT_MASS_OP_SQRT)


def checkParameterBound(model, momentum, hmcprior):
    """Reflect at the ln(sigma) bounds and flip the momentum (vectorised; same fixed point as the
    reference's per-element while loop)."""
    lo, hi = np.log(hmcprior.sigBounds[0]), np.log(hmcprior.sigBounds[1])
    if not (np.all(np.isfinite(model)) and hi > lo):
        raise FloatingPointError("non-finite model value in checkParameterBound")
    for _ in range(500):
        below, above = model < lo, model > hi
        if not (below.any() or above.any()):
            return model, momentum
        model = np.where(below, 2.0 * lo - model, model)
        momentum = np.where(below, -momentum, momentum)
        above = model > hi
        model = np.where(above, 2.0 * hi - model, model)
        momentum = np.where(above, -momentum, momentum)
    raise FloatingPointError("bound reflection did not terminate")


def getHamiltonian(mtData, mtMesh, invParam, hmcprior, hmcParam: HMCParameter,
                   ctx: HipContext | None = None, reuse_forward=True):
    """(dataMisfit, kinetic, hamiltonian, mnorm, predData) at invParam.strModel."""
    _check_solver(hmcprior)
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    m = np.asarray(invParam.strModel, dtype=np.float64)
    cache = getattr(ctx, "_cache", None)
    if reuse_forward and cache is not None and np.array_equal(cache[0], m):
        pred, misfit = cache[1], cache[2]
    else:
        pred, misfit = ctx.forward(m)
        ctx._cache = (m.copy(), pred, misfit)
    kp = getKineticEnergy(hmcParam.momentum, hmcParam)
    mprior = m - invParam.refModel
    mnorm = 0.5 * float(mprior @ (invParam.Wm @ mprior)) * hmcprior.regParam
    return misfit, kp, misfit + kp + mnorm, mnorm, pred


def proposeLeapfrog(hmcParamCurrent: HMCParameter, mtMesh, mtData, invParam, hmcprior, rng=None,
                    intstep=None, ctx: HipContext | None = None):
    """Leapfrog trajectory; L ~ U{timestep[0]..timestep[1]} unless `intstep` is given."""
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    currModel = hmcParamCurrent.rhomodel
    currMomentum = hmcParamCurrent.momentum
    invParam.strModel = currModel.copy()
    _, _, dataGrad = compDataGradient(mtMesh, mtData, invParam, hmcprior, ctx)
    hmcprior.nfevals += 1
    refModel, Wm = invParam.refModel, invParam.Wm
    dataGrad = dataGrad + (Wm @ (currModel - refModel)) * hmcprior.regParam
    dt = hmcprior.dt
    propMomentum = currMomentum - 0.5 * dt * dataGrad
    propModel = currModel.copy()
    if intstep is None:
        intstep = int(rng.integers(hmcprior.timestep[0], hmcprior.timestep[1] + 1))
    maxStepSize = 3.0
    for k in range(1, intstep + 1):
        dm = dt * getKineticGradient(propMomentum, hmcParamCurrent)
        dmMax = np.max(np.abs(dm))
        if dmMax > maxStepSize:
            dm = dm / dmMax * maxStepSize
        propModel = propModel + dm
        propModel, propMomentum = checkParameterBound(propModel, propMomentum, hmcprior)
        invParam.strModel = propModel.copy()
        _, _, dataGrad = compDataGradient(mtMesh, mtData, invParam, hmcprior, ctx)
        hmcprior.nfevals += 1
        dataGrad = dataGrad + (Wm @ (propModel - refModel)) * hmcprior.regParam
        delta = dt * dataGrad
        propMomentum = propMomentum - (delta if k < intstep else 0.5 * delta)
    return propModel, propMomentum


def proposeLeapfrogDevice(hmcParamCurrent: HMCParameter, mtMesh, mtData, invParam, hmcprior, rng=None,
                          intstep=None, ctx: HipContext | None = None):
    """Same contract as proposeLeapfrog, with the whole trajectory kept on the GPU
    (`hmcmt_leapfrog`): only (m, p) go in and (m', p', predData, misfit) come out.  The prior
    (refModel, Wm, mass) must have been registered with `ctx.set_prior`."""
    ctx = ctx or get_context(mtMesh, mtData, invParam)
    if intstep is None:
        intstep = int(rng.integers(hmcprior.timestep[0], hmcprior.timestep[1] + 1))
    lo, hi = np.log(hmcprior.sigBounds[0]), np.log(hmcprior.sigBounds[1])
    m1, p1, pred, misfit, mnorm, nf = ctx.leapfrog(hmcParamCurrent.rhomodel, hmcParamCurrent.momentum, hmcprior.dt,
                                                   intstep, hmcprior.regParam, lo, hi)
    hmcprior.nfevals += nf
    invParam.strModel = m1.copy()
    sigma = invParam.bgModel.copy()
    sigma[invParam.activeIdx] += np.exp(m1)
    mtMesh.sigma = sigma
    ctx._cache = (m1.copy(), pred, misfit)                 # getHamiltonian reuses the proposal's forward
    return m1, p1


def _run_fingerprint(invParam, hmcprior, shape):
    """What a checkpoint belongs to: sizes, sampler settings, data, weights and reference model (sha256)."""
    import hashlib
    h = hashlib.sha256()
    h.update(np.asarray(shape, dtype=np.int64).tobytes())
    h.update(np.asarray([hmcprior.dt, hmcprior.regParam, *hmcprior.timestep, *hmcprior.sigBounds], dtype=np.float64).tobytes())
    for a in (invParam.obsData, invParam.dataW, invParam.refModel):
        h.update(np.ascontiguousarray(a).tobytes())
    if hmcprior.massType != "diagonal":                  # (only then: checkpoints of diagonal runs stay valid)
        h.update(b"massType=" + str(hmcprior.massType).encode())
    return h.hexdigest()


def _save_checkpoint(path, it, done, hmcmodel, hmcdata, stats, cur, start, rng, invParam, hmcprior):
    """Flushes samples `done + 1 .. it` and the loop state.  Two files: `path + ".samples"`, append-only records of one
    sample each (model column, predicted-data column) -- a flush writes only the new samples, so a run costs O(N) I/O,
    not O(N^2 / k) -- and `path`, the small state (counters, statistics, current model / momentum, RNG state, the run's
    fingerprint), replaced atomically AFTER the samples are on disk (flush + fsync before os.replace; a crash between
    the two leaves surplus records that a resume ignores)."""
    import json
    import os
    with open(path + ".samples", "r+b" if os.path.exists(path + ".samples") else "w+b") as f:
        rec = (hmcmodel.shape[0] + 2 * hmcdata.shape[0]) * 8
        f.seek(done * rec)
        f.truncate()
        for j in range(done + 1, it + 1):
            f.write(np.ascontiguousarray(hmcmodel[:, j - 1]).tobytes())
            f.write(np.ascontiguousarray(hmcdata[:, j]).tobytes())
        f.flush()
        os.fsync(f.fileno())
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        np.savez(f, it=it, data0=hmcdata[:, 0], hmstats=stats.hmstats[:, :it + 1],
                 acceptstats=stats.acceptstats[:it], counts=np.array([stats.nAccept, stats.nReject, hmcprior.nfevals]),
                 rhomodel=cur.rhomodel, momentum=cur.momentum, start=np.array(start),
                 fingerprint=np.array(_run_fingerprint(invParam, hmcprior, hmcmodel.shape)),
                 rng=np.array(json.dumps(rng.bit_generator.state)))
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def _load_checkpoint(path, hmcmodel, hmcdata, stats, cur, rng, invParam, hmcprior):
    import json
    with np.load(path) as g:
        if str(g["fingerprint"]) != _run_fingerprint(invParam, hmcprior, hmcmodel.shape):
            raise ValueError(f"{path}: checkpoint of a different run (sizes, dt / timestep / regParam / sigBounds, data, "
                             "weights or reference model differ)")
        it = int(g["it"])
        nparam, ndata = hmcmodel.shape[0], hmcdata.shape[0]
        raw = np.fromfile(path + ".samples", dtype=np.float64, count=it * (nparam + 2 * ndata))
        if raw.size != it * (nparam + 2 * ndata):
            raise ValueError(f"{path}.samples holds fewer than the {it} samples the state file records")
        raw = raw.reshape(it, nparam + 2 * ndata)
        hmcmodel[:, :it] = raw[:, :nparam].T
        hmcdata[:, 1:it + 1] = raw[:, nparam:].copy().view(np.complex128).T
        hmcdata[:, 0] = g["data0"]
        stats.hmstats[:, :it + 1] = g["hmstats"]
        stats.acceptstats[:it] = g["acceptstats"]
        stats.nAccept, stats.nReject, hmcprior.nfevals = (int(c) for c in g["counts"])
        cur.rhomodel, cur.momentum = g["rhomodel"].copy(), g["momentum"].copy()
        rng.bit_generator.state = json.loads(str(g["rng"]))
        return it, tuple(float(x) for x in g["start"])


def mergeMoments(list_of_moments):
    """(count, mean, m2) of the union of sample sets given by their own (count, mean, m2): Chan's pairwise formula, applied from
    left to right.  m2 is the sum of squared deviations from the mean; empty sets (count 0) are passed over."""
    n, mean, m2 = 0, None, None
    for nb, mb, qb in list_of_moments:
        nb = int(nb)
        if nb == 0:
            continue
        mb, qb = np.asarray(mb, dtype=np.float64), np.asarray(qb, dtype=np.float64)
        if n == 0:
            n, mean, m2 = nb, mb.copy(), qb.copy()
            continue
        tot = n + nb
        delta = mb - mean
        mean = mean + delta * (nb / tot)
        m2 = m2 + qb + delta * delta * (n * nb / tot)
        n = tot
    if n == 0:
        raise ValueError("mergeMoments: no samples")
    return n, mean, m2


def gelmanRubin(list_of_moments):
    """Per-cell potential scale reduction R-hat (Gelman & Rubin 1992) of m >= 2 chains of equal length n >= 2 from their
    (count, mean, m2): W = mean_j s_j^2 with s_j^2 = m2_j / (n - 1), B = n / (m - 1) * sum_j (mean_j - grand mean)^2,
    R-hat = sqrt(((n - 1) / n * W + B / n) / W).  A cell that never moved in any chain (W == 0) gives nan."""
    counts = [int(c) for c, _, _ in list_of_moments]
    m = len(counts)
    if m < 2 or len(set(counts)) != 1 or counts[0] < 2:
        raise ValueError("gelmanRubin: at least two chains of the same count >= 2")
    n = counts[0]
    means = np.stack([np.asarray(mu, dtype=np.float64) for _, mu, _ in list_of_moments])
    W = np.stack([np.asarray(q, dtype=np.float64) for _, _, q in list_of_moments]).sum(axis=0) / (n - 1) / m
    B = n / (m - 1) * ((means - means.mean(axis=0)) ** 2).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(((n - 1) / n * W + B / n) / W)


def sitePPDTargets(mtMesh, invParam, yCoord, zCoord):
    """Active-cell indices for the histograms under sites: for every (y, z) of yCoord x zCoord the cell whose centre is nearest,
    separately in y and in z, among the rows below the air -- the reference's model2DInterp ("interpolate to the nearest node, not
    by linear interpolation", HMCSampler.jl:684-711); a tie goes to the lower index.  int64[len(yCoord) * len(zCoord)], depth
    fastest.  A point whose cell is not active (fixed by the inversion setup) raises ValueError."""
    yCoord, zCoord = np.atleast_1d(np.asarray(yCoord, dtype=np.float64)), np.atleast_1d(np.asarray(zCoord, dtype=np.float64))
    yNode = np.concatenate([[0.0], np.cumsum(mtMesh.yLen)]) - mtMesh.origin[0]
    zNode = np.concatenate([[0.0], np.cumsum(mtMesh.zLen)]) - mtMesh.origin[1]
    yCen = yNode[:-1] + np.diff(yNode) / 2
    zCen = zNode[:-1] + np.diff(zNode) / 2
    ny, nair = len(mtMesh.yLen), len(mtMesh.airLayer)
    cell2act = np.full(ny * len(mtMesh.zLen), -1, dtype=np.int64)
    cell2act[np.asarray(invParam.activeIdx)] = np.arange(len(invParam.activeIdx))
    out = np.empty(len(yCoord) * len(zCoord), dtype=np.int64)
    for j, y in enumerate(yCoord):
        iy = int(np.argmin(np.abs(yCen - y)))                      # (argmin: the first of equal distances)
        for k, z in enumerate(zCoord):
            iz = nair + int(np.argmin(np.abs(zCen[nair:] - z)))
            a = cell2act[iz * ny + iy]
            if a < 0:
                raise ValueError(f"sitePPDTargets: the cell nearest to (y, z) = ({y:g}, {z:g}) -- column {iy}, row {iz} -- is not active")
            out[j * len(zCoord) + k] = a
    return out


def mergeHistograms(list_of_hists):
    """The histogram of the union of sample sets -- several chains -- from their own (count, counts, (nbins, lo, hi), targets): counts
    and counters add (int64).  Histograms of different bins or targets are refused (ValueError)."""
    if not list_of_hists:
        raise ValueError("mergeHistograms: no histogram")
    count0, counts0, bins0, targets0 = list_of_hists[0]
    bins0, targets0 = tuple(bins0), np.asarray(targets0)
    total, acc = int(count0), np.asarray(counts0).astype(np.int64)
    for count, counts, bins, targets in list_of_hists[1:]:
        if tuple(bins) != bins0 or not np.array_equal(np.asarray(targets), targets0) or np.shape(counts) != acc.shape:
            raise ValueError("mergeHistograms: the histograms differ in (nbins, lo, hi) or in their targets")
        total += int(count)
        acc = acc + np.asarray(counts).astype(np.int64)
    return total, acc, bins0, targets0.copy()


def histQuantiles(hist, q):
    """Quantiles q (each in [0, 1]) of every row of hist = (count, counts, (nbins, lo, hi), targets), [nq, ntarget] in ln sigma, by
    the library's definition (hmcmt_chain_hist_quantiles): with x = q * count, the first bin b with counts_b > 0 whose inclusive
    cumulative count reaches x, and lo + w * (b + (x - cum_{b-1}) / counts_b), w = (hi - lo) / nbins."""
    count, counts, (nbins, lo, hi), _ = hist
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if int(count) < 1:
        raise ValueError("histQuantiles: the histogram holds no sample")
    if not np.all((q >= 0) & (q <= 1)):
        raise ValueError("histQuantiles: every q must lie in [0, 1]")
    counts = np.asarray(counts).astype(np.int64)
    cum = np.cumsum(counts, axis=1)
    w = (float(hi) - float(lo)) / int(nbins)
    rows = np.arange(counts.shape[0])
    out = np.empty((len(q), counts.shape[0]))
    for i, qi in enumerate(q):
        x = float(qi) * float(int(count))
        b = np.argmax((counts > 0) & (cum.astype(np.float64) >= x), axis=1)
        cb = counts[rows, b]
        out[i] = float(lo) + w * (b.astype(np.float64) + (x - (cum[rows, b] - cb).astype(np.float64)) / cb.astype(np.float64))
    return out


def histToLog10Rho(hist):
    """hist in ln sigma -> (edges[nbins + 1] in log10 of resistivity (Ohm-m), ascending, counts[ntarget, nbins] to match):
    log10 rho = -m / ln 10 turns the axis round, so the bins come out in reverse order."""
    _, counts, (nbins, lo, hi), _ = hist
    w = (float(hi) - float(lo)) / int(nbins)
    edges_m = float(lo) + w * np.arange(int(nbins) + 1)
    edges_m[-1] = float(hi)
    return (-edges_m / np.log(10.0))[::-1].copy(), np.asarray(counts)[:, ::-1].copy()


def acovOf(x, maxlag):
    """The biased autocovariance estimates c_k = (1/N) sum_{t=k}^{N-1} (x_t - xbar)(x_{t-k} - xbar), k = 0 .. maxlag, of the chain(s)
    x[N] or x[ntarget, N] (rows = cells, columns = samples, as hmcmodel): acov[maxlag + 1] or acov[maxlag + 1, ntarget], lag-major as
    the library returns them (hmcmt_chain_acov); c_k = 0 for k >= N."""
    x = np.asarray(x, dtype=np.float64)
    rows = np.atleast_2d(x)
    N, K = rows.shape[1], int(maxlag)
    if N < 1 or K < 1:
        raise ValueError("acovOf: needs at least one sample and maxlag >= 1")
    d = rows - rows.mean(axis=1, keepdims=True)
    out = np.zeros((K + 1, rows.shape[0]))
    for k in range(min(K, N - 1) + 1):
        out[k] = (d[:, k:] * d[:, :N - k]).sum(axis=1) / N
    return out[:, 0] if x.ndim == 1 else out


def _initial_positive_sequence(gamma):
    """Geyer's rule on the pair sums gamma[npairs, ntarget]: (tau, window)."""
    npairs, nt = gamma.shape
    tau, window = np.empty(nt), np.zeros(nt, dtype=np.int32)
    for j in range(nt):
        s, M, ended = 0.0, 0, False
        for m in range(npairs):
            G = gamma[m, j]
            if not G > 0.0:
                ended = True
                break
            s += G
            M += 1
        tau[j] = -1.0 + 2.0 * s
        window[j] = M if ended else -M
    return tau, window


def _npairs(K, N):
    nlag = min(K, N - 1)
    return (nlag - 1) // 2 + 1 if nlag >= 1 else 0


def _ess_of_tau(tau, n):
    lg = max(1.0, float(np.log10(n)))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = n / tau
    return np.where((tau <= 1.0 / lg) | (r > n * lg), n * lg, r)


def essFromAcov(acov, count):
    """(tau, ess, window) from acov[maxlag + 1(, ntarget)] of `count` samples by the library's rule (hmcmt_chain_ess): Geyer's initial
    positive sequence over Gamma_m = (c_2m + c_2m+1) / c_0, tau = -1 + 2 sum Gamma_m, ess = min(N / tau, N max(1, log10 N)) (the cap
    also when tau <= 1 / max(1, log10 N)), window = +pairs when a non-positive pair ended the sum and -pairs when the lags ran out;
    a constant cell (c_0 > 0 false) has tau = N, ess = 1, window = 0."""
    a = np.asarray(acov, dtype=np.float64)
    a2 = a.reshape(a.shape[0], -1)
    N, K = int(count), a2.shape[0] - 1
    if N < 1 or K < 1:
        raise ValueError("essFromAcov: needs count >= 1 and at least the lags 0 and 1")
    moved = a2[0] > 0.0
    P = _npairs(K, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        gamma = np.where(moved, (a2[0:2 * P:2] + a2[1:2 * P:2]) / a2[0], 0.0)
    tau, window = _initial_positive_sequence(gamma)
    ess = _ess_of_tau(tau, N)
    tau, ess, window = np.where(moved, tau, float(N)), np.where(moved, ess, 1.0), np.where(moved, window, 0).astype(np.int32)
    if a.ndim == 1:
        return float(tau[0]), float(ess[0]), int(window[0])
    return tau, ess, window


def mcseOfMean(ess_stats, moments):
    """Monte-Carlo standard error of the posterior mean of every target of hmcstats.ess: sqrt(m2 / count / ess) with
    moments = (count, mean, m2) = hmcstats.moments (the posterior variance m2 / count over the effective sample size)."""
    count, _, m2 = moments
    t = np.asarray(ess_stats["targets"])
    return np.sqrt(np.asarray(m2)[t] / float(count) / np.asarray(ess_stats["ess"]))


def mergeAcov(list_of_ess):
    """The effective sample size of several chains of equal count N from their hmcstats.ess, in the BDA3 / Stan form: with the
    per-chain c^_k = c_k N / (N - 1), W = mean_c c^_0, B / N = var_c(mean_c, ddof=1) (0 for one chain),
    var+ = W (N - 1) / N + B / N and rho_k = 1 - (W - mean_c c^_k) / var+, the initial positive sequence over rho_2m + rho_2m+1,
    tau = -1 + 2 sum, ess = C N / tau capped at C N max(1, log10(C N)).  Chains of different counts, lags or targets: ValueError.
    Returns a dict: count (= C N), nchains, maxlag, targets, mean, rho, tau, ess, window."""
    if not list_of_ess:
        raise ValueError("mergeAcov: no chain")
    first = list_of_ess[0]
    N, K, t0 = int(first["count"]), int(first["maxlag"]), np.asarray(first["targets"])
    for e in list_of_ess[1:]:
        if int(e["count"]) != N or int(e["maxlag"]) != K or not np.array_equal(np.asarray(e["targets"]), t0):
            raise ValueError("mergeAcov: the chains differ in count, maxlag or targets")
    if N < 2:
        raise ValueError("mergeAcov: needs at least two samples per chain")
    C = len(list_of_ess)
    chat = np.array([np.asarray(e["acov"], dtype=np.float64) for e in list_of_ess]) * (N / (N - 1.0))      # [C, K + 1, ntarget]
    means = np.array([np.asarray(e["mean"], dtype=np.float64) for e in list_of_ess])
    W = chat[:, 0].mean(axis=0)
    BN = means.var(axis=0, ddof=1) if C > 1 else np.zeros_like(W)
    varp = W * (N - 1.0) / N + BN
    moved = varp > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(moved, 1.0 - (W - chat.mean(axis=0)) / varp, 0.0)
    P = _npairs(K, N)
    tau, window = _initial_positive_sequence(rho[0:2 * P:2] + rho[1:2 * P:2])
    ess = _ess_of_tau(tau, C * N)
    return {"count": C * N, "nchains": C, "maxlag": K, "targets": t0.copy(), "mean": means.mean(axis=0), "rho": rho,
            "tau": np.where(moved, tau, float(C * N)), "ess": np.where(moved, ess, 1.0),
            "window": np.where(moved, window, 0).astype(np.int32)}


def _corr_of(cov, var, rows):
    """cov / sqrt(var_row var_cell) clamped into [-1, 1]; 0 where a variance is not positive (hmcmt_chain_corr's rule)"""
    vr, va = np.asarray(var)[rows][:, None], np.asarray(var)[None, :]
    ok = (vr > 0.0) & (va > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(ok, cov / np.sqrt(np.where(ok, vr * va, 1.0)), 0.0)
    return np.clip(c, -1.0, 1.0)


def covOf(x, rows=None):
    """The library's covariance estimator (hmcmt_chain_cov, include/hmcmt.h) from a sample history x[nparam, N] (rows = cells, columns =
    samples, as hmcmodel): the biased two-pass cov[r, a] = (1/N) sum_t (x[rows[r], t] - xbar[rows[r]]) (x[a, t] - xbar[a]) of the cells
    `rows` (0-based; None: every cell, the full matrix) with every cell.  Returns a dict like hmcstats.cov: count, rows, mean[nparam],
    var[nparam], cov[nrow, nparam], corr[nrow, nparam]."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("covOf: needs x[nparam, N] with at least one sample")
    n, N = x.shape
    r = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    mean = x.mean(axis=1)
    d = x - mean[:, None]
    var = (d * d).sum(axis=1) / N
    cov = (d[r] @ d.T) / N
    return {"count": N, "rows": r, "mean": mean, "var": var, "cov": cov, "corr": _corr_of(cov, var, r)}


def mergeCov(list_of_cov):
    """Pools the hmcstats.cov (or covOf) of several chains over the same rows: N = sum N_c, xbar = sum N_c xbar_c / N and, with
    d_c = xbar_c - xbar, cov = sum N_c (cov_c + d_c[rows] d_c[cells]) / N (var likewise); corr is recomputed from the pooled cov and
    var.  Chains of different rows or sizes: ValueError.  Returns a dict: count, nchains, rows, mean, var, cov, corr."""
    chains = [c for c in list_of_cov if c is not None and int(c["count"]) > 0]
    if not chains:
        raise ValueError("mergeCov: no chain with a counted sample")
    r = np.asarray(chains[0]["rows"], dtype=np.int64)
    for c in chains[1:]:
        if not np.array_equal(np.asarray(c["rows"]), r) or np.shape(c["cov"]) != np.shape(chains[0]["cov"]):
            raise ValueError("mergeCov: the chains differ in rows or size")
    Ns = np.array([float(c["count"]) for c in chains])
    N = Ns.sum()
    means = np.array([np.asarray(c["mean"], dtype=np.float64) for c in chains])
    mean = (Ns[:, None] * means).sum(axis=0) / N
    var, cov = np.zeros_like(mean), np.zeros(np.shape(chains[0]["cov"]))
    for Nc, mc, c in zip(Ns, means, chains):
        d = mc - mean
        var += Nc * (np.asarray(c["var"], dtype=np.float64) + d * d)
        cov += Nc * (np.asarray(c["cov"], dtype=np.float64) + d[r][:, None] * d[None, :])
    var /= N
    cov /= N
    return {"count": int(round(N)), "nchains": len(chains), "rows": r.copy(), "mean": mean, "var": var, "cov": cov,
            "corr": _corr_of(cov, var, r)}


# ---- the row sketch of the committed models (hmcmt_chain_sketch_*, include/hmcmt.h) in numpy --------------------------------------------
def _sketch_shrink(B, ell):
    """one shrink of a full buffer B[2 ell, n] in place: with K = B B' = V diag(d) V', d descending, delta = max(d[ell], 0) and
    c_i = sqrt((d_i - delta) / d_i) where d_i > delta (else 0), rows 0 .. ell - 1 become c_i v_i' B and the rest zero.  Returns delta."""
    d, V = np.linalg.eigh(B @ B.T)
    d, V = d[::-1], V[:, ::-1]
    delta = max(float(d[ell]), 0.0)
    big = d[:ell] > delta
    c = np.where(big, np.sqrt(np.where(big, d[:ell] - delta, 0.0) / np.where(big, d[:ell], 1.0)), 0.0)
    B[:ell] = (c[:, None] * V[:, :ell].T) @ B
    B[ell:] = 0.0
    return delta


def _sketch_dict(ell, B, fill, count, shrinks, Delta, x0, tot, q, given):
    N = float(max(count, 1))
    return {"count": int(count), "ell": int(ell), "fill": int(fill), "shrinks": int(shrinks), "Delta": float(Delta),
            "pivot_given": int(bool(given)), "x0": x0, "tot": tot, "q": q, "mean": x0 + tot / N, "var": (q - tot * tot / N) / N,
            "rows": B[:fill].copy()}


def sketchOf(x, ell, pivot=None):
    """The library's frequent-directions sketch (hmcmt_chain_sketch_begin, include/hmcmt.h) of a sample history x[nparam, N] (columns =
    committed models, as hmcmodel), in numpy with numpy.linalg.eigh: rows y_t = x_t - x0 (x0 = pivot, or the first column) enter a
    buffer of 2 ell rows, which is shrunk to ell rows whenever it is full.  Returns a dict like hmcstats.sketch without the principal
    components: count, ell, fill, shrinks, Delta, pivot_given, x0, tot, q, mean, var, rows[fill, nparam].  With A the N rows y_t:
    0 <= A'A - rows'rows <= Delta I and Delta <= |A - A_k|_F^2 / (ell - k) for every k < ell."""
    x = np.asarray(x, dtype=np.float64)
    ell = int(ell)
    if x.ndim != 2 or x.shape[1] < 1 or not 2 <= ell <= 64:
        raise ValueError("sketchOf: needs x[nparam, N] with at least one sample and 2 <= ell <= 64")
    n, N = x.shape
    x0 = x[:, 0].copy() if pivot is None else np.array(pivot, dtype=np.float64)
    if x0.shape != (n,) or not np.isfinite(x0).all():
        raise ValueError(f"sketchOf: pivot must hold {n} finite entries")
    B, tot, q = np.zeros((2 * ell, n)), np.zeros(n), np.zeros(n)
    fill, shrinks, Delta = 0, 0, 0.0
    for t in range(N):
        y = x[:, t] - x0
        tot += y
        q += y * y
        B[fill] = y
        fill += 1
        if fill == 2 * ell:
            Delta += _sketch_shrink(B, ell)
            shrinks += 1
            fill = ell
    return _sketch_dict(ell, B, fill, N, shrinks, Delta, x0, tot, q, pivot is not None)


def _sketch_sums(sketch, who):
    """(N, ybar[nparam]) of a sketch dict: from its x0 and tot, or from mean - x0"""
    N = int(sketch["count"])
    if sketch.get("tot") is not None:
        return N, np.asarray(sketch["tot"], dtype=np.float64) / N
    if sketch.get("x0") is None:
        raise ValueError(f"{who}: the sketch carries neither tot nor its pivot x0")
    return N, np.asarray(sketch["mean"], dtype=np.float64) - np.asarray(sketch["x0"], dtype=np.float64)


def _sketch_eig(W, rank):
    """the `rank` largest positive eigenpairs (theta descending, U[r, n] rows) of W' J W, J = diag(1, ..., 1, -1), by the Gram route
    of hmcmt_chain_pca: G = W W' = Q Lambda Q' with Lambda_i > 1e-10 Lambda_max kept, S = Lambda^1/2 Q' J Q Lambda^1/2 = Z Theta Z',
    U = (Q Lambda^-1/2 Z_sel)' W; each direction's entry of largest magnitude is positive"""
    lamG, Q = np.linalg.eigh(W @ W.T)
    if not lamG[-1] > 0.0:
        return np.zeros(0), np.zeros((0, W.shape[1]))
    keep = lamG > 1e-10 * lamG[-1]
    lamG, Q = lamG[keep], Q[:, keep]
    J = np.ones(W.shape[0])
    J[-1] = -1.0
    sq = np.sqrt(lamG)
    S = sq[:, None] * (Q.T @ (J[:, None] * Q)) * sq[None, :]
    th, Z = np.linalg.eigh(0.5 * (S + S.T))
    order = [i for i in np.argsort(-th, kind="stable") if th[i] > 0.0][:int(rank)]
    U = np.ascontiguousarray(((Q / sq[None, :]) @ Z[:, order]).T @ W)
    for k in range(len(order)):
        if U[k, np.argmax(np.abs(U[k]))] < 0:
            U[k] = -U[k]
    return th[order], U


def pcaFromSketch(sketch, rank=8):
    """(lam[r], U[r, nparam], err) from a sketch dict (sketchOf, mergeSketches, hmcstats.sketch): the leading eigenpairs of the centred
    covariance estimate (rows'rows - N ybar ybar') / N by hmcmt_chain_pca's Gram route in numpy, lam descending, and err = Delta / N:
    every lam[k] lies within err of the k-th eigenvalue of the exact (biased) covariance of the counted commits."""
    N, ybar = _sketch_sums(sketch, "pcaFromSketch")
    if N < 2 or not 1 <= int(rank):
        raise ValueError("pcaFromSketch: needs a sketch of two commits at least and rank >= 1")
    W = np.vstack([np.asarray(sketch["rows"], dtype=np.float64), np.sqrt(float(N)) * ybar])
    th, U = _sketch_eig(W, rank)
    return th / N, U, float(sketch["Delta"]) / N


def mergeSketches(list_of_sketches):
    """Pools the sketches of several chains (hmcstats.sketch, sketchOf): they must share ell and a GIVEN pivot, byte for byte, since
    their rows are differences from it.  The rows are stacked into one buffer of 2 ell rows, shrunk whenever it is full; tot, q, N and
    Delta add, and Delta also takes the merge's own shrinks, so the pooled guarantee 0 <= A'A - rows'rows <= Delta I holds for the
    concatenated rows.  Returns a dict like sketchOf's, with nchains."""
    chains = [c for c in list_of_sketches if c is not None and int(c["count"]) > 0]
    if not chains:
        raise ValueError("mergeSketches: no chain with a counted sample")
    ell = int(chains[0]["ell"])
    x0 = np.ascontiguousarray(chains[0]["x0"], dtype=np.float64)
    for c in chains:
        if not int(c["pivot_given"]) or c.get("x0") is None or c.get("tot") is None or c.get("q") is None:
            raise ValueError("mergeSketches: every sketch needs a given pivot and its x0, tot and q")
        if int(c["ell"]) != ell or np.ascontiguousarray(c["x0"], dtype=np.float64).tobytes() != x0.tobytes():
            raise ValueError("mergeSketches: the sketches differ in ell or in their pivot")
    n = x0.size
    B, tot, q = np.zeros((2 * ell, n)), np.zeros(n), np.zeros(n)
    fill, shrinks, Delta, N = 0, 0, 0.0, 0
    for c in chains:
        tot += np.asarray(c["tot"], dtype=np.float64)
        q += np.asarray(c["q"], dtype=np.float64)
        N += int(c["count"])
        Delta += float(c["Delta"])
        shrinks += int(c["shrinks"])
        for row in np.asarray(c["rows"], dtype=np.float64):
            B[fill] = row
            fill += 1
            if fill == 2 * ell:
                Delta += _sketch_shrink(B, ell)
                shrinks += 1
                fill = ell
    out = _sketch_dict(ell, B, fill, N, shrinks, Delta, x0.copy(), tot, q, True)
    out["nchains"] = len(chains)
    return out


def lowRankMassFromSketch(sketch, invM=None, rank=8, cutoff=2.0):
    """(invM[nparam], U[r, nparam], lam[r]) in the convention of lowRankMassFromSamples, from a sketch dict instead of a sample
    history: the scales are `invM` where given, else the library's window rule on the sketch's variance; the directions are the
    eigenpairs of S^-1 C S^-1, C = (rows'rows - N ybar ybar') / (N - 1), found in the sketch's span by hmcmt_chain_pca's Gram route.
    At most `rank` pairs with lam > cutoff are kept, largest first.  Where nothing was shrunk it is lowRankMassFromSamples of the
    same samples up to rounding; behind shrinks every lam is low by at most Delta / (N - 1) / min(invM).  The result can be handed to
    runHMCSampler(mass_lowrank=...)."""
    N, ybar = _sketch_sums(sketch, "lowRankMassFromSketch")
    if N < 2 or int(rank) < 0:
        raise ValueError("lowRankMassFromSketch: needs a sketch of two commits at least and rank >= 0")
    nparam = ybar.size
    if invM is None:
        s2 = np.asarray(sketch["var"], dtype=np.float64) * (N / (N - 1.0)) * (N / (N + 5.0)) + 1e-3 * 5.0 / (N + 5.0)
    else:
        s2 = np.array(invM, dtype=np.float64)
        if s2.shape != (nparam,) or not (np.isfinite(s2).all() and (s2 > 0).all()):
            raise ValueError(f"lowRankMassFromSketch: invM must hold {nparam} finite positive entries")
    W = np.vstack([np.asarray(sketch["rows"], dtype=np.float64), np.sqrt(float(N)) * ybar]) / np.sqrt(s2)[None, :]
    th, U = _sketch_eig(W, max(int(rank), 1))
    lam = th / (N - 1.0)
    keep = [k for k in range(len(lam)) if lam[k] > cutoff][:int(rank)]
    return s2, np.ascontiguousarray(U[keep]), lam[keep]


ADAPT_KEYS = ("nwarmup", "mass", "delta", "gamma", "t0", "kappa", "init_buffer", "term_buffer", "base_window", "dt_min", "dt_max", "lowrank")


def lowRankMassFromSamples(samples, rank=8, cutoff=2.0, invM=None):
    """(invM[nparam], U[r, nparam], lam[r]) of the low-rank-plus-diagonal mass M^-1 = S (I + U' (diag(lam) - I) U) S, S = diag(sqrt(invM)),
    estimated from samples[nparam, N] (columns = models, N >= 2) -- the arguments of HipContext.set_mass_lowrank and of
    runHMCSampler(mass_lowrank=...), U with one direction per ROW.  The scales are `invM` where given, else the library's own window
    rule (hmcmt_chain_adapt_begin, step 4): var N / (N + 5) + 1e-3 * 5 / (N + 5) with the unbiased sample variance.  The directions
    are the principal ones of the scaled, centred samples Z = (samples - mean) / s / sqrt(N - 1): the eigenpairs of the N x N matrix
    Z'Z lifted to U = Z v / sigma, lam = sigma^2 the variance along the direction in units of the scales.  At most `rank` pairs with
    lam > cutoff are kept, largest first -- r may be 0; each direction's entry of largest magnitude is positive.  Needs no device.
    With N << nparam the pure sampling noise of Z'Z has eigenvalues near nparam / N, far above a cutoff of 2, so the trailing
    directions kept are noise; lowRankMassFromDrawsAndGrads, which also takes the gradients, does not have that floor."""
    X = np.asarray(samples, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] < 2:
        raise ValueError("lowRankMassFromSamples: samples must be [nparam, N] with N >= 2")
    if int(rank) < 0:
        raise ValueError("lowRankMassFromSamples: rank must not be negative")
    nparam, N = X.shape
    mean = X.mean(axis=1)
    if invM is None:
        s2 = X.var(axis=1, ddof=1) * (N / (N + 5.0)) + 1e-3 * 5.0 / (N + 5.0)
    else:
        s2 = np.array(invM, dtype=np.float64)
        if s2.shape != (nparam,) or not (np.isfinite(s2).all() and (s2 > 0).all()):
            raise ValueError(f"lowRankMassFromSamples: invM must hold {nparam} finite positive entries")
    Z = (X - mean[:, None]) / np.sqrt(s2)[:, None] / np.sqrt(N - 1.0)
    w, v = np.linalg.eigh(Z.T @ Z)                          # (ascending)
    keep = [i for i in np.argsort(w)[::-1] if w[i] > cutoff][:int(rank)]
    lam = w[keep]
    U = np.ascontiguousarray(((Z @ v[:, keep]) / np.sqrt(lam)).T)
    for k in range(len(keep)):
        if U[k, np.argmax(np.abs(U[k]))] < 0:
            U[k] = -U[k]
    return s2, U, lam


def lowRankMassFromDrawsAndGrads(samples, grads, invM=None, rank=8, cutoff=2.0, gamma=1e-5):
    """(invM[nparam], U[r, nparam], lam[r]) of the low-rank-plus-diagonal mass from samples[nparam, N] AND the gradients of the potential
    at them, grads[nparam, N] (columns = models, 4 <= N): the estimator the library's warm-up runs (hmcmt_chain_adapt_lowrank,
    include/hmcmt.h), in numpy.  With W = [Zd; Zg] the centred draws over s and the centred gradients times s, both over sqrt(N - 1),
    it finds in the span of W the symmetric positive definite Sigma with Sigma cov(grad) Sigma = cov(draws) -- for a Gaussian the
    covariance itself, whatever N -- and keeps at most `rank` of its eigenpairs with theta > cutoff or theta < 1 / cutoff, by
    |ln theta| descending.  gamma > 0 is added to both projected covariances.  The scales are `invM` where given, else the window rule
    of lowRankMassFromSamples.  r may be 0; each direction's entry of largest magnitude is positive.  Needs no device.  With
    numpy.linalg.eigh on the graded matrices involved, theta carries about six digits at the default gamma (the library's Jacobi
    eigensolver nine): ample for a mass matrix, not for comparing bits."""
    X, Gr = np.asarray(samples, dtype=np.float64), np.asarray(grads, dtype=np.float64)
    if X.ndim != 2 or X.shape != Gr.shape or X.shape[1] < 4:
        raise ValueError("lowRankMassFromDrawsAndGrads: samples and grads must both be [nparam, N] with N >= 4")
    if int(rank) < 0 or not cutoff > 1.0 or not gamma > 0.0:
        raise ValueError("lowRankMassFromDrawsAndGrads: need rank >= 0, cutoff > 1 and gamma > 0")
    nparam, N = X.shape
    if invM is None:
        s2 = X.var(axis=1, ddof=1) * (N / (N + 5.0)) + 1e-3 * 5.0 / (N + 5.0)
    else:
        s2 = np.array(invM, dtype=np.float64)
        if s2.shape != (nparam,) or not (np.isfinite(s2).all() and (s2 > 0).all()):
            raise ValueError(f"lowRankMassFromDrawsAndGrads: invM must hold {nparam} finite positive entries")
    s = np.sqrt(s2)
    W = np.vstack([((X - X.mean(axis=1)[:, None]) / s[:, None]).T, ((Gr - Gr.mean(axis=1)[:, None]) * s[:, None]).T]) / np.sqrt(N - 1.0)
    K = W @ W.T
    d, V = np.linalg.eigh(K)
    keep = d > 1e-10 * d.max()
    T = (V[:, keep] / np.sqrt(d[keep])).T
    Pd, Pg = T @ K[:, :N], T @ K[:, N:]
    m = T.shape[0]
    Cd, Cg = Pd @ Pd.T + gamma * np.eye(m), Pg @ Pg.T + gamma * np.eye(m)
    g, Q = np.linalg.eigh(Cg)                              # (in Cg's eigenbasis its powers are diagonal scalings)
    sg = np.sqrt(g)
    Cq = Q.T @ Cd @ Q
    e, Z = np.linalg.eigh(sg[:, None] * (0.5 * (Cq + Cq.T)) * sg[None, :])
    Sq = ((Z * np.sqrt(e)) @ Z.T) / sg[:, None] / sg[None, :]
    theta, Yq = np.linalg.eigh(0.5 * (Sq + Sq.T))
    order = np.argsort(-np.abs(np.log(theta)), kind="stable")
    sel = [i for i in order if theta[i] > cutoff or theta[i] < 1.0 / cutoff][:int(rank)]
    U = np.ascontiguousarray((W.T @ (T.T @ (Q @ Yq[:, sel]))).T)
    for k in range(len(sel)):
        if U[k, np.argmax(np.abs(U[k]))] < 0:
            U[k] = -U[k]
    return s2, U, theta[sel]


def adaptLowrankPlan(adapt, hmcprior):
    """The options of HipContext.chain_adapt_lowrank of runHMCSampler's adapt={"lowrank": ...} as a dict, or None where the key is
    absent, None or False; needs no device.  True means the defaults.  ValueError unless the warm-up adapts the diagonal mass
    (massType "diagonal" and mass=True, which adaptPlan may have turned off for a short warm-up), and for a value out of range."""
    from .lib import ADAPT_LOWRANK_KEYS, adapt_lowrank_options
    lowrank = adapt.get("lowrank")
    if lowrank is None or lowrank is False:
        return None
    if lowrank is not True and not isinstance(lowrank, dict):
        raise ValueError("runHMCSampler: adapt lowrank must be True or a dict with the keys rank, max_samples, cutoff, gamma")
    if hmcprior.massType != "diagonal":
        raise ValueError(f"runHMCSampler: adapt lowrank needs massType \"diagonal\", not {hmcprior.massType!r}")
    _, opts = adaptPlan(adapt, hmcprior)
    if not opts["adapt_mass"]:
        raise ValueError("runHMCSampler: adapt lowrank needs mass=True (and a warm-up of at least 20 steps): it upgrades the adaptation of the diagonal mass")
    o = adapt_lowrank_options(lowrank)
    return {k: getattr(o, k) for k in ADAPT_LOWRANK_KEYS}


def adaptPlan(adapt, hmcprior):
    """(nwarmup, options of HipContext.chain_adapt_begin) of runHMCSampler's adapt={...}; needs no device.  nwarmup defaults to
    hmcprior.burninsamples and may not exceed it: the posterior moments would mix in warm-up samples.  mass defaults to True for
    massType "diagonal".  Where none of init_buffer / term_buffer / base_window is given and Stan's 75 / 50 / 25 do not fit
    nwarmup, Stan's fallback holds: 15 % / 10 % / the rest, and below 20 warm-up steps the step size alone is adapted."""
    unknown = set(adapt) - set(ADAPT_KEYS)
    if unknown:
        raise ValueError(f"runHMCSampler: adapt has no key {sorted(unknown)} ({', '.join(ADAPT_KEYS)})")
    diagonal = hmcprior.massType == "diagonal"
    nwarmup = int(adapt.get("nwarmup", hmcprior.burninsamples))
    if nwarmup < 1:
        raise ValueError(f"runHMCSampler: adapt needs nwarmup >= 1, not {nwarmup} (default: hmcprior.burninsamples)")
    if nwarmup > hmcprior.burninsamples:
        raise ValueError(f"runHMCSampler: adapt nwarmup = {nwarmup} exceeds hmcprior.burninsamples = {hmcprior.burninsamples}: "
                         "the posterior moments would mix in warm-up samples")
    mass = bool(adapt.get("mass", diagonal))
    if mass and not diagonal:
        raise ValueError(f"runHMCSampler: adapt mass=True needs massType \"diagonal\", not {hmcprior.massType!r}")
    opts = {k: adapt[k] for k in ("delta", "gamma", "t0", "kappa", "dt_min", "dt_max") if k in adapt}
    windows = {k: int(adapt[k]) for k in ("init_buffer", "term_buffer", "base_window") if k in adapt}
    if mass and not windows:
        if nwarmup < 20:
            mass = False
        elif 75 + 50 + 25 > nwarmup:
            init, term = int(0.15 * nwarmup), int(0.1 * nwarmup)
            windows = {"init_buffer": init, "term_buffer": term, "base_window": nwarmup - init - term}
    opts.update(windows)
    opts["adapt_mass"] = int(mass)
    return nwarmup, opts


# ---- the optional outputs of the device chain: one entry of CHAIN_OUTPUTS each ---------------------------------------------------------
class ChainOutput:
    """One optional output of runHMCSampler(device_chain=True): the keyword `name` fills HMCStatus.`field`; `keys` are the keys its
    dict accepts (a flag has none and arrives as {}) and `why` says why it needs the device chain.  `check(value, hmcprior)` refuses
    what can be refused without a context.  `begin(ctx, value, env)` makes the library's begin call(s) -- behind the chain's second
    chain_begin, which would end them, and in front of the first momentum -- and returns what `read(ctx, state, stats, env)`, behind
    the last step, turns into the field's value.  env: nparam, lo, hi (ln of hmcprior.sigBounds), nsamples, hmcprior.  An output that
    watches every step has `step(ctx, state, it, rec)`, called between the chain_step of sample `it` and the next momentum.  The
    docstring of an entry is its paragraph of runHMCSampler's."""
    name = field = why = None
    keys = ()
    step = None

    def check(self, value, hmcprior):
        unknown = set(value) - set(self.keys)
        if unknown:
            raise ValueError(f"runHMCSampler: {self.name} has no key {sorted(unknown)} ({', '.join(self.keys)})")

    # chain_checkpoint=: `dump(state)` is the host state as a dict of arrays and strings for the file (the library's part is in the
    # blob), `resume(ctx, value, env, saved)` the state behind HipContext.chain_restore, in place of begin -- it makes no begin call.
    # An output whose state follows from its value alone needs neither: its `plan(value, env)` is the state, and begin adds the call.
    def dump(self, state):
        return {}

    def resume(self, ctx, value, env, saved):
        return self.plan(value, env)

    def plan(self, value, env):
        return None


def _cells(given, nparam=None):
    """a keyword's list of active cells as the library takes it; None: every cell (spelled out where nparam is given)"""
    if given is None:
        return None if nparam is None else np.arange(nparam, dtype=np.int64)
    return np.asarray(given, dtype=np.int64)


class _Histograms(ChainOutput):
    """`hist={...}` (with device_chain): per-cell histograms of ln sigma, streamed in the chain's commit like the moments, so that
    marginal distributions and credible intervals need no sample history.  Keys, all optional: `targets` (active-cell indices, default
    every cell; `sitePPDTargets` gives the cells under sites), `nbins` (300, the reference's npBins), `lo`, `hi` (ln of
    hmcprior.sigBounds).  hmcstats.hist = (count, counts[ntarget, nbins], (nbins, lo, hi), targets): see histQuantiles,
    histToLog10Rho, mergeHistograms, fileio.writeSitePPD, fileio.getPosteriorQuantileModels."""
    name, field, keys, why = "hist", "hist", ("targets", "nbins", "lo", "hi"), "it is streamed in the device chain's commit"

    def plan(self, value, env):
        targets = _cells(value.get("targets"), env.nparam)
        return (int(value.get("nbins", 300)), float(value.get("lo", env.lo)), float(value.get("hi", env.hi))), targets

    def begin(self, ctx, value, env):
        bins, targets = self.plan(value, env)
        ctx.chain_hist_begin(targets, *bins)
        return bins, targets

    def read(self, ctx, state, stats, env):
        return ctx.chain_hist() + (state[0], state[1].copy())


class _DataMoments(ChainOutput):
    """`data_moments=True` (with device_chain): hmcstats.dataMoments = (count, mean[ndata], m2[ndata]) of the predicted data at the
    samples the moments count -- the posterior-predictive spread.  Neither this nor `hist` changes the order of the random draws."""
    name, field, why = "data_moments", "dataMoments", "it is streamed in the device chain's commit"

    def begin(self, ctx, value, env):
        ctx.chain_data_moments_begin()

    def read(self, ctx, state, stats, env):
        return ctx.chain_data_moments()


class _EffectiveSampleSize(ChainOutput):
    """`ess={...}` (with device_chain): per-cell lagged autocovariances streamed in the commit, and from them the integrated
    autocorrelation time and the effective sample size, computed on the GPU.  Keys, both optional: `targets` (default every cell) and
    `maxlag` (63).  hmcstats.ess is a dict: count, maxlag, targets, mean, acov[maxlag + 1, ntarget], tau, ess, window (hmcmt_chain_ess,
    include/hmcmt.h: window < 0 means the lags ran out and tau is a lower bound), and `misfit`, the same estimator applied here to the
    data misfit of the counted samples.  A chain that ends inside its burn-in gives count 0 and None for the rest.  See acovOf, essFromAcov, mcseOfMean, mergeAcov, fileio.getESSModel.  The draws keep their order."""
    name, field, keys, why = "ess", "ess", ("targets", "maxlag"), "the autocovariances are streamed in the device chain's commit"

    def plan(self, value, env):
        return _cells(value.get("targets")), int(value.get("maxlag", 63))

    def begin(self, ctx, value, env):
        targets, maxlag = self.plan(value, env)
        ctx.chain_acov_begin(targets, maxlag)
        return targets, maxlag

    def read(self, ctx, state, stats, env):
        targets, maxlag = state
        # (a chain that ends inside its burn-in has counted nothing: the read-outs need a commit, the rest of the result stands)
        count = ctx.chain_acov_count()
        (_, mean, acov), (tau, e, window) = (ctx.chain_acov(), ctx.chain_ess()) if count > 0 else ((0, None, None), (None, None, None))
        out = {"count": count, "maxlag": maxlag, "targets": _cells(targets, env.nparam).copy(), "mean": mean, "acov": acov, "tau": tau,
               "ess": e, "window": window, "misfit": None}
        D = stats.hmstats[0, 1 + env.hmcprior.burninsamples:]  # the data misfit of the counted samples: the same estimator on the host
        if len(D):
            a = acovOf(D, maxlag)
            t1, e1, w1 = essFromAcov(a, len(D))
            out["misfit"] = {"count": len(D), "mean": float(D.mean()), "acov": a, "tau": t1, "ess": e1, "window": w1}
        return out


class _Covariance(ChainOutput):
    """`cov={...}` (with device_chain): the posterior covariance and correlation between cells, streamed in the commit as cross moments
    and folded in by a batched kernel, so that trade-offs between cells need no sample history.  Keys, both optional: `rows` (the
    active-cell indices whose rows of the matrix are kept; default every cell, the full nparam x nparam matrix) and `batch` (commits
    per update kernel, 1 .. 16, default 8; the results do not depend on it).  hmcstats.cov is a dict: count, rows, mean[nparam],
    var[nparam], cov[nrow, nparam], corr[nrow, nparam] (biased estimator; hmcmt_chain_cov, include/hmcmt.h).  A chain that ends inside
    its burn-in gives count 0 and None for the rest.  See covOf, mergeCov, fileio.getCorrelationModel.  The draws keep their order."""
    name, field, keys, why = "cov", "cov", ("rows", "batch"), "the cross moments are streamed in the device chain's commit"

    def plan(self, value, env):
        return _cells(value.get("rows"))

    def begin(self, ctx, value, env):
        rows = self.plan(value, env)
        ctx.chain_cov_begin(rows, int(value.get("batch", 0)))
        return rows

    def read(self, ctx, rows, stats, env):
        # (as for ess: a chain that ends inside its burn-in has counted nothing)
        count = ctx.chain_cov_count()
        (_, mean, var, c), corr = (ctx.chain_cov(), ctx.chain_corr()) if count > 0 else ((0, None, None, None), None)
        return {"count": count, "rows": _cells(rows, env.nparam).copy(), "mean": mean, "var": var, "cov": c, "corr": corr}


class _WarmUp(ChainOutput):
    """`adapt={...}` (with device_chain): a warm-up over the first `nwarmup` samples (default hmcprior.burninsamples, and never more: the
    moments count behind the burn-in) tunes the step size by dual averaging towards the acceptance `delta` (0.8) and, with `mass`
    (default True for massType "diagonal"), the diagonal of M^-1 by Stan's windowed variance of the chain's own samples, on the GPU
    (hmcmt_chain_adapt_begin, include/hmcmt.h).  Further keys, all optional: gamma, t0, kappa, init_buffer, term_buffer, base_window,
    dt_min, dt_max; see adaptPlan for the window defaults.  hmcprior.dt is the start and is not modified.  hmcstats.adapt is a dict:
    nwarmup, dt[nsamples] (the step size each sample's trajectory used), alpha[nsamples], dt_final, invM (the final diagonal, None
    without mass) and windows, a list of (end_step, n).  `lowrank` (True, or a dict with rank, max_samples, cutoff, gamma; needs mass):
    every window end also estimates the directions and factors of the low-rank mass from the window's draws and gradients
    (hmcmt_chain_adapt_lowrank, include/hmcmt.h; no pilot run, no sample history); hmcstats.adapt["lowrank"] then holds the final
    invM, U[r, nparam], lam[r] and `windows`, the hmcmt_adapt_lowrank_info of every closed window as a dict."""
    name, field, keys, why = "adapt", "adapt", ADAPT_KEYS, "the warm-up runs in the device chain"

    def check(self, value, hmcprior):
        adaptPlan(value, hmcprior)
        adaptLowrankPlan(value, hmcprior)

    def begin(self, ctx, value, env):                       # (the warm-up: hmcprior.dt is its start and stays as it is)
        nwarmup, opts = adaptPlan(value, env.hmcprior)
        lowrank = adaptLowrankPlan(value, env.hmcprior)
        ctx.chain_adapt_begin(nwarmup, **opts)
        if lowrank is not None:
            ctx.chain_adapt_lowrank(**lowrank)
        return {"nwarmup": nwarmup, "mass": opts["adapt_mass"], "info": ctx.chain_adapt_info(), "dt": np.full(env.nsamples, np.nan),
                "alpha": np.zeros(env.nsamples), "windows": [], "lowrank": None if lowrank is None else []}

    def step(self, ctx, state, it, rec):
        before, state["info"] = state["info"], ctx.chain_adapt_info()
        state["dt"][it - 1] = before["dt"]
        # (a NUTS sample's record carries the alpha the warm-up was fed: the mean over the tree's leaves)
        state["alpha"][it - 1] = rec["alpha"] if "alpha" in rec else (1.0 if rec["hdif"] > 0 else float(np.exp(rec["hdif"])))
        if before["active"] and before["next_window_end"] == before["step"]:      # (this step was its window's last)
            state["windows"].append((it, before["window_count"] + 1))
            if state["lowrank"] is not None:
                row = ctx.chain_adapt_lowrank_info()
                if row["windows"] > len(state["lowrank"]):                        # (a window of fewer than two samples closes nothing)
                    state["lowrank"].append(row)

    def dump(self, state):
        import json
        return {"dt": state["dt"], "alpha": state["alpha"], "windows": np.array(state["windows"], dtype=np.int64).reshape(-1, 2),
                "info": np.array(json.dumps(state["info"])), "lowrank": np.array(json.dumps(state["lowrank"]))}

    def resume(self, ctx, value, env, saved):
        import json
        nwarmup, opts = adaptPlan(value, env.hmcprior)
        return {"nwarmup": nwarmup, "mass": opts["adapt_mass"], "info": json.loads(str(saved["info"])), "dt": saved["dt"].copy(),
                "alpha": saved["alpha"].copy(), "windows": [tuple(int(v) for v in w) for w in saved["windows"]],
                "lowrank": json.loads(str(saved["lowrank"]))}

    def read(self, ctx, state, stats, env):
        out = {"nwarmup": state["nwarmup"], "dt": state["dt"], "alpha": state["alpha"], "dt_final": state["info"]["dt"],
               "invM": ctx.chain_mass_diag() if state["mass"] else None, "windows": state["windows"]}
        if state["lowrank"] is not None:
            invM, U, lam = ctx.chain_mass_lowrank()
            out["lowrank"] = {"invM": invM, "U": U, "lam": lam, "windows": state["lowrank"]}
        return out


class _Sketch(ChainOutput):
    """`sketch={...}` (with device_chain): a frequent-directions row sketch of the committed models, streamed in the commit, and from
    it the leading principal components of the posterior covariance -- the joint structure that `cov` gives only as a full matrix --
    in 2 ell rows of nparam doubles.  Keys, all optional: `ell` (2 .. 64, default 32: directions kept through every shrink), `rank`
    (1 .. 32, default 8: components returned) and `pivot` (nparam values the rows are differences from; default the first counted
    model; sketches of several chains merge only under one given pivot).  hmcstats.sketch is a dict: count, ell, fill, shrinks, Delta,
    pivot_given, x0, tot, q, mean, var, rows[fill, nparam], lam[r], U[r, nparam], err and explained = lam / var.sum().  Every lam[k]
    lies within err = Delta / count of the exact k-th eigenvalue of the counted samples' covariance (hmcmt_chain_pca, include/hmcmt.h).
    A chain that ends inside its burn-in gives count 0 and None for the arrays; one counted sample gives no components.  Where
    the library refuses the components (HMCMT_EBREAKDOWN: directions not orthonormal to 1e-8, which a requested component whose
    variance is lost in rounding beside the first can cause; ask for a smaller rank) lam, U and err stay None and `pca_error` holds
    the library's message: pcaFromSketch still works on the rest.  The sketch
    adds one wait per ell counted samples.  See sketchOf, pcaFromSketch, mergeSketches, lowRankMassFromSketch, fileio.getPCAModels.
    The draws keep their order."""
    name, field, keys, why = "sketch", "sketch", ("ell", "rank", "pivot"), "the sketch is streamed in the device chain's commit"

    def check(self, value, hmcprior):
        super().check(value, hmcprior)
        from .lib import MASS_RANK_MAX, SKETCH_ELL_MAX
        if not 2 <= int(value.get("ell", 32)) <= SKETCH_ELL_MAX or not 1 <= int(value.get("rank", 8)) <= MASS_RANK_MAX:
            raise ValueError(f"runHMCSampler: sketch needs 2 <= ell <= {SKETCH_ELL_MAX} and 1 <= rank <= {MASS_RANK_MAX}")

    def plan(self, value, env):
        pivot = value.get("pivot")
        return int(value.get("ell", 32)), int(value.get("rank", 8)), None if pivot is None else np.array(pivot, dtype=np.float64)

    def begin(self, ctx, value, env):
        state = self.plan(value, env)
        ctx.chain_sketch_begin(state[0], state[2])
        return state

    def read(self, ctx, state, stats, env):
        out = ctx.chain_sketch_info()
        out.update({k: None for k in ("x0", "tot", "q", "mean", "var", "rows", "lam", "U", "err", "explained", "pca_error")})
        if out["count"] > 0:
            out.update(ctx.chain_sketch())
        if out["count"] > 1:
            from .lib import HmcmtError
            try:
                out["lam"], out["U"], out["err"] = ctx.chain_pca(state[1])
            except HmcmtError as e:
                if e.code != -11:                            # (HMCMT_EBREAKDOWN: the sketch stands, the components are refused)
                    raise
                out["pca_error"] = str(e)
            else:
                total = float(out["var"].sum())
                out["explained"] = out["lam"] / total if total > 0 else np.zeros_like(out["lam"])
        return out


CHAIN_OUTPUTS = (_Histograms(), _DataMoments(), _EffectiveSampleSize(), _Covariance(), _Sketch(), _WarmUp())


def _check_mass_lowrank(mass_lowrank, nparam):
    """runHMCSampler's mass_lowrank=(invM, U, lam) -> (invM, (invM, U, lam) or None when U has no row): shapes and values checked
    here, before the context is touched"""
    from .lib import HMCMT_MASS_RANK_MAX, lowrank_mass_arrays
    try:
        invM, U, lam = mass_lowrank
    except (TypeError, ValueError):
        raise ValueError("runHMCSampler: mass_lowrank must be (invM, U, lam)") from None
    if invM is None:
        raise ValueError("runHMCSampler: mass_lowrank needs its invM (the scales)")
    invM, U, lam = lowrank_mass_arrays(nparam, invM, U, lam)
    if U.shape[0] > HMCMT_MASS_RANK_MAX:
        raise ValueError(f"runHMCSampler: mass_lowrank has {U.shape[0]} directions, more than HMCMT_MASS_RANK_MAX = {HMCMT_MASS_RANK_MAX}")
    if not (np.isfinite(invM).all() and (invM > 0).all() and np.isfinite(lam).all() and (lam > 0).all() and np.isfinite(U).all()):
        raise ValueError("runHMCSampler: mass_lowrank needs finite positive invM and lam and a finite U")
    return invM, ((invM, U, lam) if U.shape[0] else None)


def _chain_fingerprint(invParam, hmcprior, nparam, outputs, invM, mass_lowrank, library_rng, nuts):
    """What a chain_checkpoint file belongs to: _run_fingerprint's run (sizes, sampler settings, data, weights, reference model) and the
    device chain's keywords -- the burn-in, library_rng, nuts, every output's value, invM / mass_lowrank."""
    import hashlib

    def canon(v):
        if isinstance(v, dict):
            return "{" + ",".join(f"{k!r}:{canon(v[k])}" for k in sorted(v)) + "}"
        if isinstance(v, (list, tuple)) and not all(isinstance(x, (bool, int, float, np.integer, np.floating)) for x in v):
            return "[" + ",".join(canon(x) for x in v) + "]"
        if isinstance(v, (list, tuple, np.ndarray)):         # numbers: a list and an array of the same values are the same keyword
            a = np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.int64 if a.dtype.kind in "biu" else np.float64)
            return f"<{a.dtype.str}{a.shape}{hashlib.sha256(a.tobytes()).hexdigest()}>"
        if isinstance(v, (bool, np.bool_)):
            return repr(bool(v))
        if isinstance(v, (int, np.integer)):
            return repr(int(v))
        if isinstance(v, (float, np.floating)):
            return repr(float(v))
        return repr(v)

    h = hashlib.sha256()
    h.update(_run_fingerprint(invParam, hmcprior, (nparam, hmcprior.totalsamples)).encode())
    h.update(canon({"burnin": int(hmcprior.burninsamples), "library_rng": library_rng, "nuts": nuts, "outputs": outputs, "invM": invM,
                    "mass_lowrank": mass_lowrank}).encode())
    return h.hexdigest()


class _ChainCheckpoint:
    """runHMCSampler's chain_checkpoint=path, chain_checkpoint_every=k: ONE file, replaced atomically behind every k-th sample and
    behind the last (tmp file, flush, fsync, os.replace, as _save_checkpoint does).  It holds the library's blob
    (HipContext.chain_save), the host's part -- sample index, hmstats, acceptstats, the counters, the first column of hmcdata, the NUTS
    records, every output's host state (ChainOutput.dump), for the host-fed loop the numpy generator's state in front of the next
    momentum's draw, for the seeded loop the current state's D and M (the next column of hmstats) -- and the run's fingerprint."""

    def __init__(self, path, every, fingerprint):
        self.path, self.every, self.fingerprint = path, int(every), fingerprint

    def due(self, it, nsamples):
        return it == nsamples or (self.every > 0 and it % self.every == 0)

    def save(self, ctx, it, stats, hmcprior, data0, begun, rng_state=None, energy=(0.0, 0.0)):
        import json
        import os
        fields = {"blob": ctx.chain_save(), "it": it, "data0": data0, "hmstats": stats.hmstats[:, :it + 1], "acceptstats": stats.acceptstats[:it],
                  "counts": np.array([stats.nAccept, stats.nReject, hmcprior.nfevals]), "fingerprint": np.array(self.fingerprint),
                  "rng": np.array(json.dumps(rng_state)), "energy": np.array(energy, dtype=np.float64)}
        if stats.nuts is not None:
            fields.update({f"nuts_{f}": stats.nuts[f][:it] for f, _ in NUTS_FIELDS})
        for out, state in begun:
            fields.update({f"out_{out.name}_{k}": v for k, v in out.dump(state).items()})
        tmp = self.path + ".tmp"
        with open(tmp, "wb") as f:
            np.savez(f, **fields)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, self.path)

    def load(self):
        """The file's fields as a dict, or None where there is no file; ValueError for a file of another run."""
        import os
        if not os.path.exists(self.path):
            return None
        with np.load(self.path) as g:
            if "fingerprint" not in g.files or str(g["fingerprint"]) != self.fingerprint:
                raise ValueError(f"{self.path}: chain checkpoint of a different run (sizes, dt / timestep / regParam / sigBounds, burn-in, data, "
                                 "weights, reference model, library_rng, nuts, an output's value, invM or mass_lowrank differ)")
            return {k: g[k] for k in g.files}

    def restore(self, ctx, g, stats, hmcprior, begun_of):
        """The chain and the host's part from a loaded file: returns (it, the outputs' states, the generator's state or None, (D, M))."""
        import json
        ctx.chain_restore(g["blob"])
        it = int(g["it"])
        stats.hmstats[:, :it + 1] = g["hmstats"]
        stats.acceptstats[:it] = g["acceptstats"]
        stats.nAccept, stats.nReject, hmcprior.nfevals = (int(c) for c in g["counts"])
        if stats.nuts is not None:
            for f, _ in NUTS_FIELDS:
                stats.nuts[f][:it] = g[f"nuts_{f}"]
        begun = begun_of(lambda out: {k[len(f"out_{out.name}_"):]: v for k, v in g.items() if k.startswith(f"out_{out.name}_")})
        return it, begun, json.loads(str(g["rng"])), tuple(float(v) for v in g["energy"])


def _homogeneous_start(invParam, rhoref, rng, verbose):
    """The random homogeneous start / reference model (HMCSampler.jl:100-109) of both loops: draws rhoref where none is given, sets
    invParam.strModel and invParam.refModel to it and returns (strModel, rhoref)."""
    rho0 = 1.0 / np.exp(invParam.strModel[0])
    if rhoref is None:
        rhoref = np.round(rho0 * 0.5 + (rho0 * 1.5 - rho0 * 0.5) * rng.random())
    if verbose:
        print(f"Homogeneous starting model with a resistivity of {rhoref} Ωm is used.")
    strModel = np.log(np.ones(len(invParam.strModel)) / rhoref)
    invParam.strModel = strModel.copy()
    invParam.refModel = strModel.copy()
    return strModel, rhoref


def _check_library_rng(library_rng):
    """runHMCSampler's library_rng=(seed, stream) as two ints in the library's ranges (uint64, uint32); ValueError otherwise"""
    try:
        seed, stream = (int(v) for v in library_rng)
    except (TypeError, ValueError):
        raise ValueError("runHMCSampler: library_rng must be (seed, stream)") from None
    if not (0 <= seed < 2 ** 64 and 0 <= stream < 2 ** 32):
        raise ValueError(f"runHMCSampler: library_rng needs 0 <= seed < 2^64 and 0 <= stream < 2^32; got {(seed, stream)}")
    return seed, stream


def _sample_line(it, rec):
    return (f"iterNo={it:6d} dtMisfit={rec['D1']:8.3e} mNorm={rec['M1']:8.3e} KEnergy={rec['K1']:8.3e} "
            f"HEnergy={rec['D1'] + rec['K1'] + rec['M1']:8.3e} {'accepted' if rec['accepted'] else 'rejected'} "
            f"p={min(1.0, float(np.exp(min(rec['hdif'], 0.0)))):.3f}")


def _nuts_line(it, rec):
    return (f"iterNo={it:6d} dtMisfit={rec['D']:8.3e} mNorm={rec['M']:8.3e} depth={rec['depth']} leaves={rec['nleaves']:4d} "
            f"stop={rec['stop']} selected={rec['selected']:5d} alpha={rec['alpha']:.3f}")


LIBRARY_RNG_BLOCK = 16      # samples per chain_run call where a progress line is wanted
NUTS_KEYS = ("max_depth",)
NUTS_FIELDS = (("depth", np.int32), ("nleaves", np.int32), ("stop", np.int32), ("dirs", np.uint32), ("selected", np.int64), ("alpha", np.float64))


def _check_nuts(nuts, hmcprior, library_rng):
    """runHMCSampler's nuts={"max_depth": d} -> d, refused before the context is touched: it is a sampling mode of the seeded device
    chain (hmcmt_chain_nuts_run), which draws the tree's numbers itself"""
    from .lib import NUTS_DEPTH_MAX
    if not isinstance(nuts, dict) or set(nuts) - set(NUTS_KEYS):
        raise ValueError(f"runHMCSampler: nuts must be a dict with the keys {NUTS_KEYS}")
    if library_rng is None:
        raise ValueError("runHMCSampler: nuts needs library_rng=(seed, stream) (the tree's draws are the library's)")
    try:
        depth = int(nuts.get("max_depth", NUTS_DEPTH_MAX))
    except (TypeError, ValueError):
        raise ValueError("runHMCSampler: nuts max_depth must be an integer") from None
    if not 1 <= depth <= NUTS_DEPTH_MAX:
        raise ValueError(f"runHMCSampler: nuts needs 1 <= max_depth <= {NUTS_DEPTH_MAX}, not {depth}")
    if hmcprior.massType != "diagonal":
        raise ValueError(f"runHMCSampler: nuts needs massType \"diagonal\" (optionally with mass_lowrank), not {hmcprior.massType!r}")
    return depth


def _run_seeded_chain(ctx, hmcprior, library_rng, verbose, keep_samples, watching, stats, hmcmodel, hmcdata, start, nuts=None, first=0, flush=None):
    """The loop of _run_device_chain with the library's own random numbers (library_rng = (seed, stream)): chain_seed, then the samples
    through chain_run -- one call for the whole run, blocks of LIBRARY_RNG_BLOCK with verbose (the lines of a block are printed behind
    it), single samples where an output watches every step.  Column `it` of hmstats takes its K from the record of sample it + 1 (K0
    is the kinetic energy of the momentum that sample drew); the last column's is the next draw's, read back through chain_normals and
    chain_momentum, which leaves the generator where it is.  nuts (a max_depth): the samples are NUTS samples through chain_nuts_run
    -- hmcprior.timestep is not used --, and stats.nuts takes their tree records (made by the caller).  first > 0: a chain restored
    behind sample `first`, seed included, with `start` its D and M there.  flush = (due(it), save(it)): a block ends where a
    checkpoint is due, and the file is written behind it."""
    if first == 0:
        ctx.chain_seed(*library_rng)
    nsamples = hmcprior.totalsamples
    Lmin, Lmax = int(hmcprior.timestep[0]), int(hmcprior.timestep[1])
    block = 1 if watching else (LIBRARY_RNG_BLOCK if verbose else max(nsamples, 1))
    D, M = start
    it = first
    while it < nsamples:
        n = min(block, nsamples - it)
        if flush is not None:
            n = next(k for k in range(1, n + 1) if k == n or flush[0](it + k))
        if nuts is not None:
            recs, models, preds = ctx.chain_nuts_run(n, nuts, outputs=keep_samples)
        else:
            recs, models, preds = ctx.chain_run(n, Lmin, Lmax, outputs=keep_samples)
        for k, rec in enumerate(recs):
            if nuts is not None:
                for f, _ in NUTS_FIELDS:
                    stats.nuts[f][it] = rec[f]
            stats.hmstats[:, it] = [D, M, rec["K0"], D + M + rec["K0"]]
            it += 1
            for out, state in watching:
                out.step(ctx, state, it, rec)
            hmcprior.nfevals += rec["nfevals"]
            if rec["accepted"]:
                stats.nAccept += 1
                stats.acceptstats[it - 1] = True
            else:
                stats.nReject += 1
            if verbose:
                print(_sample_line(it, rec) if nuts is None else _nuts_line(it, rec))
            D, M = rec["D"], rec["M"]
            if keep_samples:
                hmcmodel[:, it - 1] = models[k]
                hmcdata[:, it] = preds[k] if rec["accepted"] else hmcdata[:, it - 1]
        if flush is not None and flush[0](it):
            flush[1](it, None, (D, M))
    seed, stream, t = ctx.chain_rng_state()
    K = ctx.chain_momentum(ctx.chain_normals(t))             # (host-fed: t stays)
    stats.hmstats[:, nsamples] = [D, M, K, D + M + K]
    stats.rng = (seed, stream, t)


def _run_device_chain(mtMesh, mtData, invParam, hmcprior, rng, rhoref, ctx, verbose, keep_samples, outputs, invM, mass_lowrank=None,
                      library_rng=None, nuts=None, chain_checkpoint=None, chain_checkpoint_every=0):
    """runHMCSampler's loop through the chain API of the library (hmcmt_chain_*): model, momentum, predicted data and the posterior
    moments stay on the GPU; per sample nparam normals go up and one record comes back (plus the sample, with keep_samples).
    Draws from `rng` in the host loop's order: the first momentum's normals, rhoref; per sample L, u, the next momentum's normals.
    `outputs`: keyword -> value of the entries of CHAIN_OUTPUTS that are on.  `mass_lowrank`: checked (invM, U, lam) with at least one
    direction, set behind the prior.  `chain_checkpoint`: the file of _ChainCheckpoint; where it exists the chain is restored from it
    (HipContext.chain_restore in place of both chain_begins and the outputs' begins) and the loop goes on behind the saved sample."""
    from types import SimpleNamespace
    from .lib import HMCMT_MASS_WM
    nparam, ndata = len(invParam.strModel), len(invParam.obsData)
    diagonal = hmcprior.massType == "diagonal"
    fileModel = np.asarray(invParam.strModel, dtype=np.float64).copy()    # the file's start model stays the chain's state (:88)
    z = rng.standard_normal(nparam)                         # getMomentumVector's draw (:90)
    strModel, rhoref = _homogeneous_start(invParam, rhoref, rng, verbose)
    if invM is not None:
        invM = np.ascontiguousarray(invM, dtype=np.float64)
        if invM.shape != (nparam,) or not (np.isfinite(invM).all() and (invM > 0).all()):
            raise ValueError(f"runHMCSampler: invM must hold {nparam} finite positive entries")
    ctx.set_prior(invParam.refModel, invParam.Wm, invM if invM is not None else (setMassMatrix(nparam, 1.0)[0] if diagonal else np.ones(nparam)))
    if not diagonal:
        ctx.set_mass(HMCMT_MASS_WM)
    if mass_lowrank is not None:
        ctx.set_mass_lowrank(None, mass_lowrank[1], mass_lowrank[2])      # (the scales: the prior's invM, set just above)
    lo, hi = np.log(hmcprior.sigBounds[0]), np.log(hmcprior.sigBounds[1])
    nsamples = hmcprior.totalsamples
    env = SimpleNamespace(nparam=nparam, lo=lo, hi=hi, nsamples=nsamples, hmcprior=hmcprior)
    nkeep = nsamples if keep_samples else 0
    hmcmodel = np.zeros((nparam, nkeep))
    hmcdata = np.zeros((ndata, nkeep + 1), dtype=np.complex128)
    stats: HMCStatus = initHMCStatus(nsamples)
    if nuts is not None:
        stats.nuts = {"max_depth": nuts, **{f: np.zeros(nsamples, dtype=t) for f, t in NUTS_FIELDS}}
    on = [out for out in CHAIN_OUTPUTS if out.name in outputs]
    ck = saved = None
    if chain_checkpoint:
        ck = _ChainCheckpoint(chain_checkpoint, chain_checkpoint_every,
                              _chain_fingerprint(invParam, hmcprior, nparam, outputs, invM, mass_lowrank, library_rng, nuts))
        saved = ck.load()
    first, rng_state = 0, None
    if saved is not None:
        first, begun, rng_state, energy = ck.restore(ctx, saved, stats, hmcprior,
                                             lambda state_of: [(out, out.resume(ctx, outputs[out.name], env, state_of(out))) for out in on])
        hmcdata[:, 0] = saved["data0"]
        if verbose:
            print(f"resuming the device chain behind sample {first} of {nsamples} ({chain_checkpoint})")
    else:
        # the reference takes its first Hamiltonian at the homogeneous model (:100-112) and its first trajectory from the file's
        startD, startM = ctx.chain_begin(strModel, hmcprior.dt, hmcprior.regParam, lo, hi, burnin=hmcprior.burninsamples)
        hmcdata[:, 0] = ctx.chain_state()[2]
        if not np.array_equal(fileModel, strModel):
            ctx.chain_begin(fileModel, hmcprior.dt, hmcprior.regParam, lo, hi, burnin=hmcprior.burninsamples)
            ctx.chain_set_energy(startD, startM)
        # (behind the second begin: a begin ends the accumulators)
        begun = [(out, out.begin(ctx, outputs[out.name], env)) for out in on]
    watching = [(out, state) for out, state in begun if out.step is not None]
    flush = None if ck is None else ((lambda it: ck.due(it, nsamples)),
                                     (lambda it, state, energy=(0.0, 0.0): ck.save(ctx, it, stats, hmcprior, hmcdata[:, 0], begun, state, energy)))
    if library_rng is not None:
        # (z, drawn above so that rhoref is the draw it is without the keyword, is not used: every momentum is the library's)
        start = (startD, startM) if first == 0 else energy
        _run_seeded_chain(ctx, hmcprior, library_rng, verbose, keep_samples, watching, stats, hmcmodel, hmcdata, start, nuts, first, flush)
        stats.moments = ctx.chain_moments()
        for out, state in begun:
            setattr(stats, out.field, out.read(ctx, state, stats, env))
        return hmcmodel, stats, hmcdata
    if first == 0:
        startK = ctx.chain_momentum(z)
        stats.hmstats[:, 0] = [startD, startM, startK, startD + startM + startK]
    else:
        # the momentum of sample first + 1, drawn again from the generator's state in front of it: column `first` holds its K already
        rng.bit_generator.state = rng_state
        ctx.chain_momentum(rng.standard_normal(nparam))
    for it in range(first + 1, nsamples + 1):
        L = int(rng.integers(hmcprior.timestep[0], hmcprior.timestep[1] + 1))
        u = rng.random()
        rec, model, pred = ctx.chain_step(L, u, outputs=keep_samples)
        for out, state in watching:
            out.step(ctx, state, it, rec)
        hmcprior.nfevals += rec["nfevals"]
        if rec["accepted"]:
            stats.nAccept += 1
            stats.acceptstats[it - 1] = True
        else:
            stats.nReject += 1
        if verbose:
            print(_sample_line(it, rec))
        rng_state = rng.bit_generator.state if flush is not None and flush[0](it) else None
        startK = ctx.chain_momentum(rng.standard_normal(nparam))
        stats.hmstats[:, it] = [rec["D"], rec["M"], startK, rec["D"] + rec["M"] + startK]
        if keep_samples:
            hmcmodel[:, it - 1] = model
            hmcdata[:, it] = pred if rec["accepted"] else hmcdata[:, it - 1]      # (:164-168: a rejection repeats the column)
        if rng_state is not None:
            flush[1](it, rng_state)
    stats.moments = ctx.chain_moments()
    for out, state in begun:
        setattr(stats, out.field, out.read(ctx, state, stats, env))
    return hmcmodel, stats, hmcdata


def runHMCSampler(mtMesh, mtData, invParam, hmcprior, rng=None, rhoref=None, ctx: HipContext | None = None,
                  verbose=False, reuse_forward=True, device_leapfrog=False, device_id=None,
                  checkpoint=None, checkpoint_every=0, device_chain=False, keep_samples=True, hist=None, data_moments=False, ess=None,
                  cov=None, sketch=None, adapt=None, invM=None, mass_lowrank=None, library_rng=None, nuts=None, chain_checkpoint=None,
                  chain_checkpoint_every=0):
    """Returns (hmcmodel[nparam, nsamples], hmcstats, hmcdata[ndata, nsamples+1]).  The chain runs on GPU `device_id`
    (default: `default_device()`, i.e. LOCAL_RANK) unless a context is passed in.

    `device_chain=True`: the loop runs through the library's chain API (hmcmt_chain_*) -- the chain's state never leaves the GPU,
    the random numbers are drawn here in the same order, so a seed gives the same chain as the host loop to solver tolerance.
    hmcstats.moments = (count, mean, m2) then holds the streaming posterior moments of the samples behind hmcprior.burninsamples
    (fileio.getPosteriorModelFromMoments).  `keep_samples=False` (with device_chain): no sample comes back -- hmcmodel has zero
    columns and hmcdata its first column only; the moments are the result.  `checkpoint=` is refused with device_chain (ValueError):
    a device chain is checkpointed with `chain_checkpoint=`.

    `chain_checkpoint=path`, `chain_checkpoint_every=k` (with device_chain and keep_samples=False): behind every k-th sample and
    behind the last, ONE file is replaced atomically.  It holds the library's blob of the chain (hmcmt_chain_save, include/hmcmt.h:
    state, moments, generator, the mass in force, every accumulator, the warm-up), the host's part (sample index, hmstats, acceptstats,
    the counters, the NUTS records, the outputs' host state, the numpy generator's state) and the run's fingerprint.  If the file
    exists when the sampler starts, the chain RESUMES behind the saved sample (hmcmt_chain_restore: no evaluation; the first resumed
    sample evaluates its start gradient, so hmcprior.nfevals is one more per resume) and draws the numbers the uninterrupted run
    would have -- both loops, host-fed and library_rng, with and without nuts.  The resumed chain is the uninterrupted one bit for
    bit on a context whose gradient is a function of the model alone (warm_start "cold", a fixed sweep count), else to solver
    tolerance: its first solves start cold.  A file of a different run -- _run_fingerprint's run, or another burn-in, library_rng,
    nuts, output value, invM or mass_lowrank -- is refused (ValueError), and so is the keyword with keep_samples=True: a sample
    history belongs to the host loop's `checkpoint=`.  A flush waits for the chain and writes the whole blob: choose k by the
    blob's size.
    The optional outputs of the device chain -- hist=, data_moments=, ess=, cov=, sketch=, adapt= -- are one entry of CHAIN_OUTPUTS each, and
    each entry's docstring is its paragraph here:
    {CHAIN_OUTPUTS}
    `invM=array` (with device_chain): the diagonal of M^-1 the chain starts with instead of ones, for example an earlier run's
    adapted mass.  The draws keep their order.
    `mass_lowrank=(invM, U, lam)` (with device_chain and massType "diagonal"): the low-rank-plus-diagonal mass of
    HipContext.set_mass_lowrank, for example lowRankMassFromSamples of a pilot run -- invM[nparam] the scales, U[r, nparam] the
    directions, lam[r].  The draws keep their order.  With r = 0 it is `invM=invM`.  Not together with invM= or adapt={"mass": True};
    an adapt without "mass" adapts the step size alone.

    `library_rng=(seed, stream)` (with device_chain): the chain draws its own random numbers in the library -- Philox4x32-10 by
    counter (hmcmt_chain_seed, include/hmcmt.h): the momenta on the GPU, L and u on the host side of the library -- and runs through
    hmcmt_chain_run: one call for the run (blocks of 16 samples with verbose, single samples with adapt=), one wait and no upload per
    sample.  The chain is a function of (seed, stream) and the problem alone, the same from Python and from julia/HMCMTHip.jl;
    hmcstats.rng = (seed, stream, t) is the generator's whole state behind the run, t the index of the next draw.  `rng` still draws
    rhoref, and nothing else.  Every other keyword works unchanged.

    `nuts={"max_depth": d}` (with device_chain and library_rng; massType "diagonal", with or without invM= / mass_lowrank=): the
    No-U-turn sampler of the library (hmcmt_chain_nuts_run, include/hmcmt.h) chooses every sample's trajectory length; d in 1 .. 10
    bounds the tree at 2^d - 1 leapfrog steps and hmcprior.timestep is not used.  It is a sampling mode, not an output: the commit,
    the optional outputs and adapt= (fed the tree's mean acceptance) work unchanged.  hmcstats.nuts holds max_depth and, per sample,
    depth, nleaves, stop (0 max_depth, 1 U-turn inside the new subtree, 2 U-turn of the tree, 3 divergence), dirs, selected and alpha;
    acceptstats marks the samples whose selected state is not the start.

    `checkpoint` (a file path) with `checkpoint_every` = k > 0: the chain's state -- samples so far, statistics, current
    model and momentum, the RNG state -- is flushed every k samples; if the file exists when the sampler starts, the
    chain RESUMES behind its last flushed sample and draws the same random numbers an uninterrupted run would have
    (the reference keeps every sample in memory until the chain ends, HMCSampler.jl:785-828: a crash loses the run;
    SURVEY section 5 lists this as the one piece of fault tolerance worth adding).  The resumed chain is the
    uninterrupted chain to solver tolerance, not bit for bit, on a real GPU context: the iterative solves of the first
    resumed trajectory start cold instead of from the interrupted run's field history (bit-identical with a
    deterministic direct-solve context, tests/test_host.py).  A checkpoint of a different run -- other sizes, dt,
    timestep, regParam, sigBounds, data, weights or reference model -- is refused."""
    _check_solver(hmcprior)
    if device_chain and checkpoint:
        raise ValueError("runHMCSampler: checkpoint is not available with device_chain=True (use the host loop or device_leapfrog=True; "
                         "a device chain with keep_samples=False is checkpointed with chain_checkpoint=)")
    if chain_checkpoint and not (device_chain and not keep_samples):
        raise ValueError("runHMCSampler: chain_checkpoint needs device_chain=True and keep_samples=False (a sample history belongs to the "
                         "host loop's checkpoint=)")
    if not keep_samples and not device_chain:
        raise ValueError("runHMCSampler: keep_samples=False needs device_chain=True (only the device chain streams the posterior moments)")
    # (every refusal before the context is touched and the first number is drawn)
    outputs = {k: v for k, v in (("hist", hist), ("data_moments", {} if data_moments else None), ("ess", ess), ("cov", cov), ("sketch", sketch), ("adapt", adapt)) if v is not None}
    on = [out for out in CHAIN_OUTPUTS if out.name in outputs]
    needing = [(out.name, out.why) for out in on] + [(k, "it is the device chain's mass") for k, v in (("invM", invM), ("mass_lowrank", mass_lowrank))
                                                     if v is not None]
    if library_rng is not None:
        needing.append(("library_rng", "the library's generator feeds the device chain"))
    if nuts is not None:
        needing.append(("nuts", "the No-U-turn sampler is the device chain's"))
    if needing and not device_chain:
        raise ValueError("runHMCSampler: %s needs device_chain=True (%s)" % needing[0])
    if library_rng is not None:
        library_rng = _check_library_rng(library_rng)
    if nuts is not None:
        nuts = _check_nuts(nuts, hmcprior, library_rng)
    if mass_lowrank is not None:
        if hmcprior.massType != "diagonal":
            raise ValueError(f"runHMCSampler: mass_lowrank needs massType \"diagonal\", not {hmcprior.massType!r}")
        if invM is not None:
            raise ValueError("runHMCSampler: mass_lowrank carries its own invM; not together with invM=")
        if adapt is not None:
            if adapt.get("mass"):
                raise ValueError("runHMCSampler: adapt mass=True adapts a diagonal mass; not together with mass_lowrank")
            outputs["adapt"] = {**adapt, "mass": False}
    for out in on:
        out.check(outputs[out.name], hmcprior)
    if invM is not None and hmcprior.massType != "diagonal":
        raise ValueError(f"runHMCSampler: invM needs massType \"diagonal\", not {hmcprior.massType!r}")
    if mass_lowrank is not None:
        invM, mass_lowrank = _check_mass_lowrank(mass_lowrank, len(invParam.strModel))
    rng = rng or np.random.default_rng()
    ctx = ctx or get_context(mtMesh, mtData, invParam, device_id=device_id)
    if device_chain:
        return _run_device_chain(mtMesh, mtData, invParam, hmcprior, rng, rhoref, ctx, verbose, keep_samples, outputs, invM, mass_lowrank,
                                 library_rng, nuts, chain_checkpoint, chain_checkpoint_every)
    nparam, ndata = len(invParam.strModel), len(invParam.obsData)
    cur = initHMCParameter(nparam)
    diagonal = hmcprior.massType == "diagonal"             # (:80-86)
    if diagonal:
        cur.invM, cur.sqrtM = setMassMatrix(nparam, 1.0)
    else:
        cur.invM, cur.sqrtM = setMassMatrix(invParam, ctx)
    cur.rhomodel = invParam.strModel.copy()               # file start model stays the chain state (:88)
    cur.momentum = getMomentumVector(nparam, cur, rng)
    prop = HMCParameter(nparam, cur.rhomodel.copy(), cur.momentum.copy(), cur.invM, cur.sqrtM)
    _homogeneous_start(invParam, rhoref, rng, verbose)     # (behind the first momentum's normals, as the reference draws)
    startD, startK, startH, startM, predData = getHamiltonian(mtData, mtMesh, invParam, hmcprior, cur, ctx,
                                                              reuse_forward)
    if device_leapfrog:
        ctx.set_prior(invParam.refModel, invParam.Wm, cur.invM if diagonal else np.ones(nparam))
        if not diagonal:
            from .lib import HMCMT_MASS_WM
            ctx.set_mass(HMCMT_MASS_WM)                    # (the factor of setMassMatrix is kept: same Wm)
    nsamples = hmcprior.totalsamples
    hmcmodel = np.zeros((nparam, nsamples))
    hmcdata = np.zeros((ndata, nsamples + 1), dtype=np.complex128)
    stats: HMCStatus = initHMCStatus(nsamples)
    stats.hmstats[:, 0] = [startD, startM, startK, startH]
    hmcdata[:, 0] = predData
    first = 1
    flushed = 0
    if checkpoint:
        import os
        if os.path.exists(checkpoint):
            done, (startD, startM, startK, startH) = _load_checkpoint(checkpoint, hmcmodel, hmcdata, stats, cur, rng,
                                                                      invParam, hmcprior)
            first = done + 1
            flushed = done
            if verbose:
                print(f"resuming behind sample {done} of {nsamples} ({checkpoint})")
    for it in range(first, nsamples + 1):
        propose = proposeLeapfrogDevice if device_leapfrog else proposeLeapfrog
        propModel, propMomentum = propose(cur, mtMesh, mtData, invParam, hmcprior, rng, None, ctx)
        prop.rhomodel, prop.momentum = propModel.copy(), propMomentum.copy()
        finishD, finishK, finishH, finishM, predData = getHamiltonian(mtData, mtMesh, invParam, hmcprior, prop,
                                                                      ctx, reuse_forward)
        hdif = startH - finishH
        aratio = rng.random()
        if hdif > 0 or aratio < np.exp(hdif):
            cur.rhomodel, cur.momentum = propModel.copy(), propMomentum.copy()
            startD, startM = finishD, finishM
            stats.nAccept += 1
            stats.acceptstats[it - 1] = True
            hmcdata[:, it] = predData
        else:
            stats.nReject += 1
            hmcdata[:, it] = hmcdata[:, it - 1]
        if verbose:
            print(f"iterNo={it:6d} dtMisfit={finishD:8.3e} mNorm={finishM:8.3e} KEnergy={finishK:8.3e} "
                  f"HEnergy={finishH:8.3e} {'accepted' if stats.acceptstats[it - 1] else 'rejected'} "
                  f"p={min(1.0, float(np.exp(min(hdif, 0.0)))):.3f}")
        cur.momentum = getMomentumVector(nparam, cur, rng)
        startK = getKineticEnergy(cur.momentum, cur)
        startH = startD + startM + startK
        stats.hmstats[:, it] = [startD, startM, startK, startH]
        hmcmodel[:, it - 1] = cur.rhomodel
        if checkpoint and checkpoint_every > 0 and (it % checkpoint_every == 0 or it == nsamples):
            _save_checkpoint(checkpoint, it, flushed, hmcmodel, hmcdata, stats, cur, (startD, startM, startK, startH), rng,
                             invParam, hmcprior)
            flushed = it
    return hmcmodel, stats, hmcdata


if runHMCSampler.__doc__:                                   # (python -OO has none)
    runHMCSampler.__doc__ = runHMCSampler.__doc__.replace("{CHAIN_OUTPUTS}", "\n    ".join(type(out).__doc__ for out in CHAIN_OUTPUTS))


# --------------------------------------------------------------------------------------------
SKETCH_INFO_KEYS = ("count", "ell", "fill", "shrinks", "Delta", "pivot_given")


def gatherBlockFields(nparam, ncols, nsamples, ndata, with_moments, sketch_ell=0):
    """One chain's block in parallelHMCSampler's all-gather: its fields in order, (name, number of doubles).  Their sum is the block.
    sketch_ell > 0 (the chains run with sketch={...}): the chain's row sketch behind the rest -- its six counters (SKETCH_INFO_KEYS),
    x0, tot, q and room for its 2 ell rows."""
    fields = [("model", nparam * ncols), ("hmstats", 4 * (nsamples + 1)), ("acceptstats", nsamples), ("data", 2 * ndata * (ncols + 1)),
              ("secs_and_flag", 2)]
    fields += [("count", 1), ("mean", nparam), ("m2", nparam)] if with_moments else []
    if sketch_ell:
        fields += [("sketch_info", len(SKETCH_INFO_KEYS)), ("sketch_x0", nparam), ("sketch_tot", nparam), ("sketch_q", nparam),
                   ("sketch_rows", 2 * int(sketch_ell) * nparam)]
    return fields


def _sketch_pack(sk, ell, nparam):
    """a chain's hmcstats.sketch as the five sketch fields of its gather block (a chain that counted nothing: zeros but for ell)"""
    rows = np.zeros((2 * ell, nparam))
    if sk is None or int(sk["count"]) == 0:
        return {"sketch_info": [0, ell, 0, 0, 0.0, 0], "sketch_x0": np.zeros(nparam), "sketch_tot": np.zeros(nparam),
                "sketch_q": np.zeros(nparam), "sketch_rows": rows}
    rows[:int(sk["fill"])] = sk["rows"]
    return {"sketch_info": [float(sk[k]) for k in SKETCH_INFO_KEYS], "sketch_x0": sk["x0"], "sketch_tot": sk["tot"], "sketch_q": sk["q"],
            "sketch_rows": rows}


def _sketch_unpack(part, nparam):
    """the sketch dict of a gathered block (sketchOf's keys), or None for a chain that counted nothing"""
    info = part["sketch_info"]
    count, ell, fill, shrinks, pivot_given = (int(round(info[i])) for i in (0, 1, 2, 3, 5))
    if count == 0:
        return None
    return _sketch_dict(ell, part["sketch_rows"].reshape(2 * ell, nparam), fill, count, shrinks, float(info[4]), part["sketch_x0"].copy(),
                        part["sketch_tot"].copy(), part["sketch_q"].copy(), pivot_given)


def _block_views(buf, fields):
    """name -> that field's stretch of the block `buf` (a view)"""
    return dict(zip([name for name, _ in fields], np.split(buf, np.cumsum([size for _, size in fields])[:-1])))


def parallelHMCSampler(mtMesh, mtData, invParam, hmcprior, pids=None, seed=0, outdir=None, nchains=None,
                       run_chain=None, device_id=None, context_factory=None, chains_per_gpu=1, gather="torch", **sampler_kw):
    """Independent chains, one process per GPU (parallelHMC.jl:10-49).

    With `torch.distributed` initialised (backend "nccl" = RCCL over xGMI on the GPU box, "gloo" in
    CPU tests) rank r runs chains r, r+W, ... on ITS OWN GPU -- `device_id`, default `default_device()` =
    LOCAL_RANK; with the nccl backend the process's current device is set to it before the collective --
    with RNG stream (seed, chain), and the sample blocks are ALL-GATHERED so every rank holds every chain;
    rank 0 writes the per-chain files the reference writes.  Without a process group the chains run one
    after another.  `pids` is kept for signature parity: its length is the number of chains (default:
    world size).  `context_factory(mesh, data, inv, device_id)` replaces `get_context` (the CPU tests run
    the real sampler on an oracle-backed stand-in); `run_chain(chain_index, rng)` replaces the sampler.
    `chains_per_gpu` = 2 or 4 runs that many of the rank's chains CONCURRENTLY on its GPU, one context and one host
    thread each, every context confined to its share of the CUs of every XCD (HipContext(cu_share=...),
    hmcmt_next_cu_share: CU-masked streams): the persistent solve kernels of the chains are co-resident, each with its share of
    the system slots.  Measured at the headline size near the true model (bench.py `two_chains_per_gpu`,
    scripts/gpu_cu_share_probe.py): two chains on halves 1.13-1.15x the aggregate steps/s of one chain on the whole device, four
    on quarters 1.17x.  (The shares' streams are BLOCKING HIP streams: keep other GPU work of the process off the legacy
    default stream while chains sample, or it serialises them -- DESIGN 7.)  A mesh whose systems need
    more workgroups than a share's CUs per XCD hold (the stress size: 30 of 16) runs the launch-per-phase loop in each share.  The chains
    and their results are the same as run one after another (independent contexts, per-chain RNG streams; the same solver, so
    the same bits).  Rounds 2-3 ran the concurrent contexts on the launch-per-phase loop (1.34x then); round 4 had no mode that
    composed with the persistent kernel (0.95x).
    `gather="library"`: the sample blocks are all-gathered by the library's own RCCL entry point
    (hmcmt_allgather_samples, include/hmcmt.h -- what a non-Python host would call) instead of torch's; the process
    group then only carries the 128-byte RCCL id from rank 0 to the others.  Works without a process group too (one rank).
    Further keyword arguments go to runHMCSampler (e.g. device_leapfrog=True; `checkpoint=path` and `chain_checkpoint=path` become
    `path.chain<k>` per chain; device_chain=True, keep_samples=False and the device chain's optional outputs).  What those outputs
    fill -- every HMCStatus field of CHAIN_OUTPUTS -- is not gathered: it stays with the chain on the chain's own rank.  The one
    exception is `sketch={...}`: every chain is given the same pivot, the start model invParam.strModel (unless the keyword names
    one), each chain's sketch -- counters, x0, tot, q, rows: (2 ell + 3) nparam + 6 doubles -- travels behind its block, so every rank
    ends with every chain's hmcstats.sketch (another rank's chain without lam and U), and rank 0 pools them: the first chain's
    hmcstats.sketch["merged"] is mergeSketches of all chains with the pooled lam, U, err and explained (pcaFromSketch); None where
    fewer than two samples were counted in all.
    `library_rng=True` (with device_chain=True): chain c draws its numbers in the library as stream c of `seed`,
    runHMCSampler(library_rng=(seed, c)); its hmcstats.rng stays on the chain's own rank like the optional outputs.
    `nuts={"max_depth": d}` goes through to runHMCSampler with it; hmcstats.nuts stays on the chain's own rank too.
    Chains that carry posterior moments (HMCStatus.moments: device_chain=True, or a `run_chain` that sets them) have
    count, mean[nparam], m2[nparam] packed behind their block, so every rank ends with every chain's moments (mergeMoments,
    gelmanRubin).  A chain's block in the gather is, in doubles (the sum of gatherBlockFields, which packing and unpacking walk),
        nparam * ncols + 4 * (nsamples + 1) + nsamples + 2 * ndata * (ncols + 1) + 2   [+ 1 + 2 * nparam with moments],
    ncols = nsamples, or 0 with keep_samples=False: then 2 * nparam + 5 * nsamples + 2 * ndata + 7 instead of
    nparam * nsamples + ...  Without either keyword the layout is what it was.  With fewer chains than ranks, the ranks that run none
    take ncols and the moments flag from those that do (one all-reduce of two integers in front of the gather, only in that case).
    Returns (hmcmodel[list], hmcstats[list], hmcdata[list]) indexed by chain.
    """
    import copy
    try:
        import torch
        import torch.distributed as dist
        have_pg = dist.is_available() and dist.is_initialized()
    except Exception:                                       # pragma: no cover
        have_pg = False
    world, rank = (dist.get_world_size(), dist.get_rank()) if have_pg else (1, 0)
    dev_id = default_device() if device_id is None else int(device_id)
    use_cuda = have_pg and dist.get_backend() == "nccl"
    if use_cuda:
        torch.cuda.set_device(dev_id)                       # the collective below runs on this rank's own GPU
    if nchains is None:
        nchains = len(pids) if pids is not None else world
    mine = list(range(rank, nchains, world))
    results = {}

    # shares of every XCD's CUs = chains that actually run at a time: the largest of (4, 2, 1) that neither exceeds chains_per_gpu nor
    # the chains this rank has (chains_per_gpu = 4 with two local chains: halves, not quarters -- a quarter to a half of the GPU would
    # idle for the whole run), and that many worker threads (three chains on two shares: two at a time, then the third)
    shares = cu_shares_for(chains_per_gpu, len(mine))
    if int(chains_per_gpu) > 1 and int(chains_per_gpu) not in (2, 4):
        import warnings
        warnings.warn("chains_per_gpu must be 1, 2 or 4 (shares of every XCD's CUs): other values run concurrent contexts on the "
                      "launch-per-phase loop, slower than one chain after another")
    import threading
    free_shares, share_lock = list(range(shares)), threading.Lock()

    def one_chain(c):
        rng = np.random.default_rng([seed, c])
        t0 = time.time()
        if run_chain is not None:
            model, stats, data = run_chain(c, rng)
        else:
            inv_c, prior_c, mesh_c = copy.deepcopy(invParam), copy.deepcopy(hmcprior), copy.deepcopy(mtMesh)
            with share_lock:
                my_share = free_shares.pop(0) if shares > 1 else None
            try:
                # (the context is created INSIDE the try: a create that raises hands its share back, and the next chain fails with
                #  the real error instead of an IndexError on an empty list)
                ctx_kw = {} if my_share is None else {"cu_share": (my_share, shares)}
                ctx_c = context_factory(mesh_c, mtData, inv_c, dev_id) if context_factory is not None else \
                    get_context(mesh_c, mtData, inv_c, device_id=dev_id, **ctx_kw)
                kw = dict(sampler_kw)
                for key in ("checkpoint", "chain_checkpoint"):  # one checkpoint file per chain
                    if kw.get(key):
                        kw[key] = f"{kw[key]}.chain{c + 1}"
                if kw.get("library_rng") is True:               # the library's generator: chain c is stream c of the run's seed
                    kw["library_rng"] = (int(seed), c)
                if kw.get("sketch") is not None and kw["sketch"].get("pivot") is None:
                    # one pivot for every chain, the start model's: their sketches are pooled behind the gather (mergeSketches)
                    kw["sketch"] = {**kw["sketch"], "pivot": np.array(invParam.strModel, dtype=np.float64)}
                model, stats, data = runHMCSampler(mesh_c, mtData, inv_c, prior_c, rng, ctx=ctx_c, **kw)
            finally:
                release_context(inv_c)
                if my_share is not None:
                    with share_lock:
                        free_shares.append(my_share)
        results[c] = (model, stats, data, time.time() - t0)

    if chains_per_gpu > 1 and len(mine) > 1:
        from concurrent.futures import ThreadPoolExecutor
        # (one worker per share: a worker without a share of its own would pop an empty list -- chains_per_gpu = 3 has two)
        workers = shares if shares > 1 else int(chains_per_gpu)
        with ThreadPoolExecutor(max_workers=workers) as pool:      # (the library calls release the GIL)
            list(pool.map(one_chain, mine))
    else:
        for c in mine:
            one_chain(c)

    # the block layout: from this rank's chains; a rank without one takes it from the keywords, then from the other ranks (below)
    if results:
        model0, stats0 = next(iter(results.values()))[:2]
        nparam, ncols = model0.shape
        nsamples = len(stats0.acceptstats)
        with_moments = getattr(stats0, "moments", None) is not None
    else:
        nparam, nsamples = len(invParam.strModel), hmcprior.totalsamples
        ncols = nsamples if sampler_kw.get("keep_samples", True) else 0
        with_moments = bool(sampler_kw.get("device_chain")) and run_chain is None
    if have_pg and world > 1 and 0 < nchains < world:
        # ranks without a chain: what the keywords cannot tell (a `run_chain` that returns no columns or sets moments) comes from
        # the ranks that ran one -- two integers, and only in this case, which every rank sees alike
        lay = torch.tensor([ncols if results else -1, int(with_moments) if results else -1], dtype=torch.int64,
                           device=torch.device("cuda", dev_id) if use_cuda else torch.device("cpu"))
        dist.all_reduce(lay, op=dist.ReduceOp.MAX)
        ncols, with_moments = int(lay[0]), bool(lay[1])
    ndata = len(invParam.obsData)
    per = (nchains + world - 1) // world                   # chain slots per rank (padded)
    sketch_kw = sampler_kw.get("sketch")                    # (a keyword: every rank sees it alike)
    sketch_ell = int(sketch_kw.get("ell", 32)) if sketch_kw is not None else 0
    fields = gatherBlockFields(nparam, ncols, nsamples, ndata, with_moments, sketch_ell)
    blk = sum(size for _, size in fields)

    def pack(slot):
        c = rank + slot * world
        buf = np.zeros(blk)
        if c in results:
            model, stats, data, secs = results[c]
            part = {"model": model, "hmstats": stats.hmstats, "acceptstats": stats.acceptstats.astype(float),
                    "data": data.reshape(-1).view(np.float64), "secs_and_flag": [secs, 1.0]}
            if with_moments:
                part.update(zip(("count", "mean", "m2"), stats.moments))
            if sketch_ell:
                part.update(_sketch_pack(getattr(stats, "sketch", None), sketch_ell, nparam))
            for name, view in _block_views(buf, fields).items():
                view[:] = np.reshape(part[name], -1)
        return buf

    local = np.concatenate([pack(s) for s in range(per)]) if per else np.zeros(0)
    if gather == "library":
        from .lib import SampleComm
        uid = [SampleComm.unique_id() if rank == 0 else None]
        if have_pg and world > 1:
            dist.broadcast_object_list(uid, src=0)
        comm = SampleComm(dev_id, world, rank, uid[0])
        allbuf = comm.allgather(local).reshape(world, per, blk)
        comm.close()
    elif have_pg and world > 1:
        dev = torch.device("cuda", dev_id) if use_cuda else torch.device("cpu")
        send = torch.from_numpy(local).to(dev)
        recv = torch.empty(world * local.size, dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(recv, send)             # RCCL ring over xGMI on the GPU box
        allbuf = recv.cpu().numpy().reshape(world, per, blk)
    else:
        allbuf = local.reshape(1, per, blk)

    hmcmodel, hmcstats, hmcdata, secs = [None] * nchains, [None] * nchains, [None] * nchains, [0.0] * nchains
    for r in range(world):
        for s in range(per):
            c = r + s * world
            if c >= nchains:
                continue
            part = _block_views(allbuf[r, s], fields)
            acc = part["acceptstats"] > 0.5
            hmcmodel[c] = part["model"].reshape(nparam, ncols).copy()
            hmcdata[c] = part["data"].copy().view(np.complex128).reshape(ndata, ncols + 1)
            secs[c] = float(part["secs_and_flag"][0])
            hmcstats[c] = HMCStatus(int(acc.sum()), int((~acc).sum()), acc, part["hmstats"].reshape(4, nsamples + 1).copy())
            if with_moments:
                hmcstats[c].moments = (int(round(part["count"][0])), part["mean"].copy(), part["m2"].copy())
            if c in results:                                # (what the optional outputs fill is not gathered: a chain's own rank keeps it)
                for out in CHAIN_OUTPUTS:
                    setattr(hmcstats[c], out.field, getattr(results[c][1], out.field, None))
                hmcstats[c].rng = getattr(results[c][1], "rng", None)
            elif sketch_ell:                                 # another rank's chain: its sketch came with the block (no components)
                hmcstats[c].sketch = _sketch_unpack(part, nparam)
    if sketch_ell and rank == 0 and nchains > 0:
        # the chains share one pivot (one_chain): rank 0 pools their sketches and takes the pooled principal components.  The pooled
        # dict goes to the FIRST chain's hmcstats.sketch["merged"]; None where no chain counted two samples
        gathered = []
        for r in range(world):
            for s in range(per):
                if r + s * world < nchains:
                    gathered.append(_sketch_unpack(_block_views(allbuf[r, s], fields), nparam))
        merged = None
        counted = [g for g in gathered if g is not None]
        if sum(int(g["count"]) for g in counted) >= 2 and all(int(g["pivot_given"]) for g in counted):
            merged = mergeSketches(gathered)
            lam, U, err = pcaFromSketch(merged, int(sketch_kw.get("rank", 8)))
            total = float(merged["var"].sum())
            merged.update(lam=lam, U=U, err=err, explained=lam / total if total > 0 else np.zeros_like(lam))
        if hmcstats[0].sketch is None:
            hmcstats[0].sketch = {"count": 0}
        hmcstats[0].sketch["merged"] = merged
    if outdir is not None and rank == 0:
        from .fileio import outputHMCSamples
        for c in range(nchains):
            outputHMCSamples(hmcmodel[c], hmcstats[c], hmcdata[c], ichain=c + 1, cputime=secs[c], outdir=outdir)
    return hmcmodel, hmcstats, hmcdata
