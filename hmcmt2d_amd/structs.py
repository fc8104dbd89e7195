"""Host-side data structures mirroring the reference's Julia structs field for field.

`TensorMesh2D`, `MTData`      <- HMCMT/src/HMCFileIO/HMCFileIO.jl:26-60
`HMCPrior`, `HMCParameter`,
`HMCStatus`, `InvDataModel`   <- HMCMT/src/HMCStruct/HMCStruct.jl:18-91, defaults :129-165

Index arrays (`rxID`, `freqID`, `dtID`) stay 1-based exactly as the reference reader stores
them (readMT2DData.jl:118-139); the C ABI converts.  Sparse operators of the reference
(`Face/Grad/AveCN/AveCF`, `activeCell`, `dataW`, `Wm`) are not materialised: the HIP library
builds the stencils from `yLen/zLen` directly, `activeCell` is kept as its column index list
`activeIdx` (0-based), `dataW` as its diagonal and `Wm` as a scipy CSR matrix.
"""
from __future__ import annotations

from dataclasses import dataclass, field
import numpy as np


@dataclass
class TensorMesh2D:
    yLen: np.ndarray              # cell widths in y
    zLen: np.ndarray              # cell heights in z, air layers first (top -> down)
    airLayer: np.ndarray          # air thicknesses as listed in the file (bottom -> up)
    gridSize: tuple               # (ny, nz_total)
    origin: np.ndarray            # (y0, z0); z0 already shifted by the air thickness
    sigma: np.ndarray             # cell conductivities, y fastest, air rows first
    Face: object = None           # kept for struct parity; unused by the HIP path
    Grad: object = None
    AveCN: object = None
    AveCF: object = None
    setup: bool = False


@dataclass
class MTData:
    rxLoc: np.ndarray             # (nRx, 2): y, z
    freqs: np.ndarray
    dataType: str                 # "Impedance" (the only type that works end-to-end)
    dataComp: list                # ["ZXY", "ZYX"]
    rxID: np.ndarray              # 1-based
    freqID: np.ndarray            # 1-based
    dtID: np.ndarray              # 1-based
    dataID: np.ndarray            # bool over (dt, rx, freq), dt fastest
    compTE: bool = True
    compTM: bool = True


@dataclass
class HMCPrior:
    burninsamples: int = 100
    totalsamples: int = 500
    sigBounds: list = field(default_factory=lambda: [0.01, 10.0])
    sigmastd: float = 0.05
    dt: float = 0.01
    timestep: list = field(default_factory=lambda: [10, 15])
    linearSolver: str = ""        # "" / "mumps" in the reference; "hip" selects this library
    massType: str = "diagonal"
    regParam: float = 1.0
    nfevals: int = 0


def initHMCPrior() -> HMCPrior:
    """HMCStruct.jl:129-140."""
    return HMCPrior()


@dataclass
class HMCParameter:
    nparam: int
    rhomodel: np.ndarray
    momentum: np.ndarray
    invM: np.ndarray              # diagonal of M^-1 (the reference's default "diagonal" mass)
    sqrtM: np.ndarray             # diagonal of M^1/2


def initHMCParameter(nparam: int) -> HMCParameter:
    """HMCStruct.jl:159-170."""
    return HMCParameter(nparam, np.zeros(nparam), np.zeros(nparam), np.zeros(nparam), np.zeros(nparam))


@dataclass
class HMCStatus:
    nAccept: int
    nReject: int
    acceptstats: np.ndarray       # bool[nsamples]
    hmstats: np.ndarray           # (4, nsamples+1): dataMisfit, mnorm, kinetic, hamiltonian
    moments: object = None        # (count, mean[nparam], m2[nparam]) of the samples behind the burn-in, when the chain ran
                                  # on the device (runHMCSampler(device_chain=True)); not a field of the reference's struct
    hist: object = None           # (count, counts[ntarget, nbins], (nbins, lo, hi), targets): runHMCSampler(device_chain=True, hist=...)
    dataMoments: object = None    # (count, mean[ndata], m2[ndata]) of the predicted data: runHMCSampler(..., data_moments=True)
    ess: object = None            # dict count, maxlag, targets, mean, acov, tau, ess, window, misfit: runHMCSampler(..., ess=...)
    cov: object = None            # dict count, rows, mean, var, cov, corr: runHMCSampler(..., cov=...)
    sketch: object = None         # dict count, ell, fill, shrinks, Delta, mean, var, rows, lam, U, err, explained: runHMCSampler(..., sketch=...)
    adapt: object = None          # dict nwarmup, dt, alpha, dt_final, invM, windows: runHMCSampler(..., adapt=...)
    rng: object = None            # (seed, stream, t) of the library's generator behind the run: runHMCSampler(..., library_rng=(seed, stream))
    nuts: object = None           # dict max_depth, depth, nleaves, stop, dirs, selected, alpha (per sample): runHMCSampler(..., nuts={"max_depth": d})


@dataclass
class MAPStatus:
    """What sampler.findMAP returns beside the model: the records of hmcmt_map_begin (row 0) and of every hmcmt_map_step, as arrays.
    Not a struct of the reference, which has no optimiser."""
    status: str                   # "RUNNING" (maxiter reached), "CONVERGED" or "STALLED" (no step lowers the objective)
    niter: int                    # accepted steps
    nfevals: int                  # gradient evaluations, the start's included
    phi: np.ndarray               # [nrec] D + M
    dataMisfit: np.ndarray        # [nrec] D
    mnorm: np.ndarray             # [nrec] M
    pgInf: np.ndarray             # [nrec] max norm of the projected gradient
    pg2: np.ndarray               # [nrec] its 2-norm
    alpha: np.ndarray             # [nrec] accepted step length (0: none)
    backtracks: np.ndarray        # [nrec] int
    resets: np.ndarray            # [nrec] int
    npairs: np.ndarray            # [nrec] int
    pairStored: np.ndarray        # [nrec] bool
    nbound: np.ndarray            # [nrec] int: cells held at a bound
    evals: np.ndarray             # [nrec] int: evaluations of each call
    predData: object = None       # predicted data at the returned model


def initHMCStatus(nsamples: int) -> HMCStatus:
    """HMCStruct.jl:144-155."""
    return HMCStatus(0, 0, np.zeros(nsamples, dtype=bool), np.zeros((4, nsamples + 1)))


@dataclass
class InvDataModel:
    obsData: np.ndarray           # complex128[nData]
    dataW: np.ndarray             # diagonal of the data weighting matrix, 1/|err|
    strModel: np.ndarray          # ln(sigma) on active cells
    refModel: np.ndarray
    activeIdx: np.ndarray         # 0-based cell ids of the active (non-fixed) cells
    bgModel: np.ndarray           # conductivity of the fixed cells, 0 elsewhere
    Wm: object                    # scipy.sparse CSR, (G A)^T (G A)
