"""Generates tests/golden/coprod2_mass_chain.npz: an HMC chain of the ORACLE (direct solves) on the reference's coprod2 example as
shipped (tests/golden/examples/coprod2) with `masstype: nondiagonal` appended to a copy of its start-up file -- the reference's
non-diagonal mass matrix M = Wm (setMassMatrix(invParam), HMCSampler.jl:478-489): sqrtM = L = chol(Wm).L, invM = Wm^-1 --, the
start-up file's own dt = 0.015 and L in [6, 10], reference model 100 ohm-m, numpy Generator seed 2025, 24 samples.  The chain loop
is oracle.runHMCSampler's, with the mass operators in place of its diagonal ones (the oracle's proposeLeapfrog and
getMomentumVector multiply by them: `invM * p`, `sqrtM * z`).  About ten minutes on one core:
`python tests/golden/make_chain_mass.py`.  Stored: the Hamiltonian terms and accept flags of every sample, the first five
samples and the last, nfevals -- what tests/test_gpu_mass.py holds the HIP sampler to."""
import copy
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
NSAMPLES, SEED, RHOREF = 24, 2025, 100.0


def nondiagonal_example(name, workdir):
    """(mesh, data, inv, prior) of a reference example directory whose start-up file, copied to `workdir`, gets the line
    `masstype: nondiagonal` appended; read through readstartupFile"""
    from hmcmt2d_amd.fileio import readstartupFile
    src = os.path.join(HERE, "examples", name)
    for f in os.listdir(src):
        shutil.copy(os.path.join(src, f), workdir)
    with open(os.path.join(workdir, "startupfile"), "a") as f:
        f.write("\nmasstype: nondiagonal\n")
    return readstartupFile(os.path.join(workdir, "startupfile"))


class WmInverse:
    """invM = Wm^-1 as an operator: `self * p` solves with Wm (one sparse LU)."""

    def __init__(self, Wm):
        self.lu = spla.splu(sp.csc_matrix(Wm))

    def __mul__(self, p):
        return self.lu.solve(np.asarray(p, dtype=np.float64))


def wm_mass(Wm):
    """(invM, sqrtM) of setMassMatrix(invParam): Wm^-1 and the lower Cholesky factor of Wm in the natural order"""
    L = np.linalg.cholesky(Wm.toarray())
    return WmInverse(Wm), sp.csr_matrix(L)


def run_chain(mesh, mtData, invParam, hmcprior, rng, rhoref):
    """oracle.runHMCSampler (HMCSampler.jl:72-196) with the non-diagonal mass"""
    from oracle import hmcmt_oracle as O
    nparam, ndata = len(invParam.strModel), len(invParam.obsData)
    invM, sqrtM = wm_mass(invParam.Wm)
    currModel = invParam.strModel.copy()
    currMomentum = O.getMomentumVector(nparam, sqrtM, rng)
    strModel = np.log(np.ones(nparam) / rhoref)
    invParam.strModel = strModel.copy()
    invParam.refModel = strModel.copy()
    s, _ = O.modelTransform(invParam.strModel)
    sigma = invParam.bgModel.copy(); sigma[invParam.activeIdx] += s
    mesh.sigma = sigma
    startD, startK, startH, startM, predData = O.getHamiltonian(mtData, mesh, invParam, hmcprior, currMomentum, invM)
    nsamples = hmcprior.totalsamples
    hmcmodel = np.zeros((nparam, nsamples))
    hmstats = np.zeros((4, nsamples + 1))
    accept = np.zeros(nsamples, dtype=bool)
    hmstats[:, 0] = [startD, startM, startK, startH]
    for it in range(1, nsamples + 1):
        L = int(rng.integers(hmcprior.timestep[0], hmcprior.timestep[1] + 1))
        propModel, propMomentum = O.proposeLeapfrog(currModel, currMomentum, invM, mesh, mtData, invParam, hmcprior, L, False)
        finishD, finishK, finishH, finishM, predData = O.getHamiltonian(mtData, mesh, invParam, hmcprior, propMomentum, invM)
        hdif = startH - finishH
        aratio = rng.random()
        if hdif > 0 or aratio < np.exp(hdif):
            currModel, currMomentum = propModel.copy(), propMomentum.copy()
            startD, startM = finishD, finishM
            accept[it - 1] = True
        currMomentum = O.getMomentumVector(nparam, sqrtM, rng)
        startK = O.getKineticEnergy(currMomentum, invM)
        startH = startD + startM + startK
        hmstats[:, it] = [startD, startM, startK, startH]
        hmcmodel[:, it - 1] = currModel
    return hmcmodel, hmstats, accept


if __name__ == "__main__":
    from oracle import hmcmt_oracle as O
    nmax = int(sys.argv[1]) if len(sys.argv) > 1 else None         # (a shorter trial run: nothing is written)
    with tempfile.TemporaryDirectory() as wd:
        mesh, data, inv, prior = nondiagonal_example("coprod2", wd)
    assert prior.massType == "nondiagonal"
    O.setupTensorMesh2D(mesh)
    prior.totalsamples = nmax or NSAMPLES
    t0 = time.time()
    hm, hs, acc = run_chain(mesh, data, copy.deepcopy(inv), prior, np.random.default_rng(SEED), RHOREF)
    print("chain done in %.0f s: accepted %d of %d, nfevals %d, misfit %.1f -> %.1f" % (
        time.time() - t0, int(acc.sum()), prior.totalsamples, prior.nfevals, hs[0, 0], hs[0, -1]))
    if not nmax:
        np.savez_compressed(os.path.join(HERE, "coprod2_mass_chain.npz"), hmstats=hs, acceptstats=acc, nfevals=prior.nfevals,
                            first=hm[:, :5], last=hm[:, -1])
