"""Independent reference for the solve's operator q = A p and preconditioner z = P^-1 r, in plain numpy / scipy,
complex128.  Nothing here reads hmcmt2d_amd/csrc or tests/emul: the operator is the ORACLE's assembled matrix (Aii of
MT2DFwdSolver), the fast-diagonalisation stage is written from the separable form P = Mz(q) (x) Ty + (Tz(q) + i w Mz(s)) (x) My
of DESIGN 4.2 and solved by sparse LU, and the smoother is built from the oracle matrix's own diagonal.

Two forms of the FDM stage F:
  F_exact(s)        sparse LU of P with two steps of iterative refinement -- what the fp64 kernels and the host emulation apply;
  F_modal(s, V)     V . T_j^-1 . V' with the CALLER's eigenvector matrix and one complex tridiagonal per mode.  With the library's
                    V it reproduces F_exact; with bf16(V) it is the operator the mixed-precision kernels apply in exact arithmetic
                    (they round V to bfloat16 by design and keep everything else at fp32 class or better), so it holds them at
                    fp32 level where F_exact could hold them at the per-cent level only.
The eigenvalues of F_modal are Rayleigh quotients, never the library's `lam`.  They are taken from the matrix passed as `V_lam`
(default: V itself): the kernels form their tridiagonals from the eigenvalues of the UNROUNDED basis and round only the transform
matrices, and the Rayleigh quotient of a rounded column is no substitute -- the rounding error mixes in a little of every mode and
lam_max / lam_min is 1e5 and more on these meshes: measured, the quotients of bf16(V)'s columns are off by up to 0.5 % at 49 modes
and 12 % at 404.

Vectors are in the library's padded nodal layout [S][NZP][NYP] (node (iy, iz) at iz * NYP + iy, interior nodes 1 <= iy <= ny - 1,
1 <= iz <= nz - 1, zero elsewhere); systems s < nF are TE, the others TM, frequencies in the order of data.freqs."""
import copy
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.linalg import solve_banded

from tests.helpers import make_problem, ragged_problem

MU0 = 4e-7 * np.pi
OMEGA_J = 0.8                      # damping of the point-Jacobi sweeps
EPS = np.finfo(float).eps


def bf16(a):
    """float64 -> bfloat16 (round to nearest even) -> float64"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- the shapes of tests/test_precond_host.py and tests/test_gpu_precond.py ----

# 16-mode slabs with ONE column part: hmcmt_persist_envelope (pure arithmetic, no device) reports them from 34 rows on (air rows
# included) at every width up to 63 cells -- the 128 threads of the narrowest kernel sweep two chunks of eight rows per mode and
# half, and 17 rows per half need the four chunks of a 16-mode slab.  33 rows still run 32-mode slabs (cfg2 has 32).  53 cells
# wide: 64 padded nodes are FOUR slabs on the three row blocks' workgroups, so one workgroup solves two -- the case the tall
# headline-width mesh of tests/test_gpu_persist.py (200 x 157: 13 slabs on 12 workgroups) reaches at a hundred times the size.
SLAB16 = (53, 31, 2, 5, 4, 3)        # ragged_problem arguments: 31 earth rows + 3 air rows


SHAPES = {
    "cfg2": lambda: make_problem("cfg2"),
    "w301": lambda: ragged_problem(301, 19, 2, 6, 4, 3),
    "w100": lambda: ragged_problem(100, 23, 2, 6, 4, 3),
    "w200": lambda: ragged_problem(200, 23, 2, 6, 4, 3),
    "w405": lambda: ragged_problem(405, 23, 2, 6, 4, 3),
    "w270": lambda: ragged_problem(270, 14, 2, 4, 4, 3),
    "slab16": lambda: ragged_problem(*SLAB16),
}


def _tridiag(d, o):
    return sp.diags([o, d, o], [-1, 0, 1], format="csc")


class PrecondRef:
    def __init__(self, mesh, data, inv, m):
        from oracle import hmcmt_oracle as O
        self.ny, self.nz = (int(v) for v in mesh.gridSize)
        ny, nz = self.ny, self.nz
        self.nF = len(data.freqs)
        self.S = 2 * self.nF
        self.omega = 2 * np.pi * np.asarray(data.freqs, dtype=float)
        self.yLen, self.zLen = np.asarray(mesh.yLen, float), np.asarray(mesh.zLen, float)
        # conductivity as the oracle forms it (compDataGradient)
        sigma = np.asarray(inv.bgModel, dtype=float).copy()
        sigma[inv.activeIdx] += np.exp(np.asarray(m, dtype=float))
        self.sigma = sigma
        # the operator: the oracle's own assembly
        msh = copy.deepcopy(mesh)
        O.setupTensorMesh2D(msh)
        msh.sigma = sigma
        keep = {}
        O.MT2DFwdSolver(msh, data, keep=keep)
        self._Aii = keep["Aii"]
        self._freqs = list(data.freqs)
        # the separable background
        y, z = self.yLen, self.zLen
        self.my = 0.5 * (y[:-1] + y[1:])
        self.Ty = _tridiag(1 / y[:-1] + 1 / y[1:], -1 / y[1:-1])
        self.My = sp.diags(self.my, format="csc")
        sbar = np.exp(np.log(sigma.reshape(nz, ny)).mean(axis=1))              # geometric lateral mean per cell row
        self._bg = {}
        for mode, (q, s) in enumerate(((np.full(nz, 1 / MU0), sbar), (1 / sbar, np.full(nz, MU0)))):
            mzq = 0.5 * (z[:-1] * q[:-1] + z[1:] * q[1:])
            mzs = 0.5 * (z[:-1] * s[:-1] + z[1:] * s[1:])
            tzd = q[:-1] / z[:-1] + q[1:] / z[1:]
            tzo = -(q[1:-1] / z[1:-1])
            self._bg[mode] = (mzq, mzs, tzd, tzo)
        self._lu, self._P = {}, {}

    # -- layout --
    def pack(self, x, NZP, NYP):
        """interior values [S][nz-1][ny-1] -> the padded nodal layout"""
        out = np.zeros((x.shape[0], NZP, NYP), complex)
        out[:, 1:self.nz, 1:self.ny] = x
        return out

    def interior(self, x):
        return np.asarray(x)[..., 1:self.nz, 1:self.ny]

    # -- operator --
    def operator(self, s):
        mode, f = ("TE", s) if s < self.nF else ("TM", s - self.nF)
        return self._Aii[(mode, self._freqs[f])]

    def spmv(self, s, p):
        """p, result: interior values [nz-1][ny-1]"""
        return (self.operator(s) @ p.reshape(-1)).reshape(p.shape)

    def spmv_scale(self, s, p):
        """(|A| |p|)_i: the scale of the componentwise error of q = A p"""
        return (abs(self.operator(s)) @ np.abs(p.reshape(-1))).reshape(p.shape)

    def spmv_error(self, s, p, q):
        """max_i |q_i - (A p)_i| / (|A| |p|)_i in units of eps; where the scale is zero (no impulse within reach) q must be zero"""
        d, scale = np.abs(q - self.spmv(s, p)), self.spmv_scale(s, p)
        reach = scale > 0
        assert not d[~reach].any()
        return float((d[reach] / scale[reach]).max() / EPS)

    # -- FDM stage --
    def P(self, s):
        if s not in self._P:
            mzq, mzs, tzd, tzo = self._bg[s >= self.nF]
            w = self.omega[s % self.nF]
            Tzz = _tridiag(tzd + 1j * w * mzs, tzo.astype(complex))
            self._P[s] = (sp.kron(sp.diags(mzq), self.Ty) + sp.kron(Tzz, self.My)).tocsc()
        return self._P[s]

    def F_exact(self, s):
        P = self.P(s)
        if s not in self._lu:
            self._lu[s] = spla.splu(P)
        lu = self._lu[s]

        def F(t):
            b = t.reshape(-1)
            x = lu.solve(b)
            for _ in range(2):
                x = x + lu.solve(b - P @ x)
            return x.reshape(t.shape)
        return F

    def rayleigh(self, V):
        """Rayleigh quotients v_j' Ty v_j / v_j' My v_j of the columns of V [node][mode]"""
        return np.einsum("ij,ij->j", V, self.Ty @ V) / np.einsum("ij,ij->j", V, self.my[:, None] * V)

    def F_modal(self, s, V, V_lam=None):
        lam = self.rayleigh(V if V_lam is None else V_lam)
        mzq, mzs, tzd, tzo = self._bg[s >= self.nF]
        w = self.omega[s % self.nF]
        n = self.nz - 1
        bands = []
        for l in lam:
            ab = np.zeros((3, n), complex)
            ab[0, 1:] = tzo
            ab[1] = l * mzq + tzd + 1j * w * mzs
            ab[2, :-1] = tzo
            bands.append(ab)

        def F(t):
            Y = t @ V                                           # [iz][mode]
            for j, ab in enumerate(bands):
                Y[:, j] = solve_banded((1, 1), ab, Y[:, j])
            return Y @ V.T
        return F

    def backward_error(self, s, z, t):
        """|| P z - t ||_inf / || |P| |z| + |t| ||_inf"""
        P = self.P(s)
        zz, tt = z.reshape(-1), t.reshape(-1)
        return float(np.abs(P @ zz - tt).max() / (abs(P) @ np.abs(zz) + np.abs(tt)).max())

    # -- the smoothed preconditioner --
    def precond(self, s, r, F, sweeps):
        """sweeps 0: F alone; 1 / 2: that many damped point-Jacobi sweeps on each side of F (inner damping 1)"""
        if sweeps == 0:
            return F(r)
        A = self.operator(s)
        D = (OMEGA_J / A.diagonal()).reshape(r.shape)
        Ax = lambda x: (A @ x.reshape(-1)).reshape(r.shape)
        z = D * r
        for _ in range(sweeps - 1):
            z = z + D * (r - Ax(z))
        z = z + F(r - Ax(z))
        for _ in range(sweeps):
            z = z + D * (r - Ax(z))
        return z


@functools.lru_cache(maxsize=None)
def reference(name):
    """(mesh, data, inv, m, PrecondRef) of a shape of SHAPES: built once per process, shared by the tests, never modified"""
    mesh, data, inv, m = SHAPES[name]()
    return mesh, data, inv, m, PrecondRef(mesh, data, inv, m)


# ---- test vectors ----

PS_OWN = 14      # interior rows per row block of the persistent kernel (checked against persist_info by the GPU tests)


def seams(ny, nz, NYP, row_blocks=None, column_parts=1):
    """(rows, cols): the interior rows / columns on both sides of every place where the kernels' tiling changes hands.  Rows: the
    row blocks of PS_OWN rows and, inside a block, the strip boundaries of the two- and four-strip kernels (tile rows 5|6, 11|12,
    17|18 of 24 with five halo rows in front).  Columns: the split of the two column parts (16 * ceil(NYP / 32)), the outer edges of
    the eight halo columns each part keeps of the other, and the 32-column K-group boundaries next to the split.  Without
    persist_info (host tests) row_blocks follows from nz and the column split is taken as if the mesh had two parts."""
    nb = -(-(nz - 1) // PS_OWN) if row_blocks is None else row_blocks
    rows = {1, nz - 1}
    for b in range(nb):
        iz0 = 1 + PS_OWN * b
        rows.update((iz0 - 1, iz0, iz0 + 1, iz0 + 6, iz0 + 7, iz0 + 12, iz0 + 13))
    c0 = 16 * ((NYP + 31) // 32)
    cols = {1, ny - 1, c0 - 1, c0, c0 - 9, c0 - 8, c0 + 7, c0 + 8, 32 * (c0 // 32) - 1, 32 * (c0 // 32), 32 * (c0 // 32 + 1) - 1, 32 * (c0 // 32 + 1)}
    if column_parts == 1 and row_blocks is not None:
        cols = {1, ny - 1, 15, 16, ny // 2, ny // 2 + 1}
    return sorted(r for r in rows if 1 <= r <= nz - 1), sorted(c for c in cols if 1 <= c <= ny - 1)


def make_vectors(S_, NZP, NYP, ny, nz, rows, cols, seed=3):
    """Three vectors in the padded nodal layout, zero on boundary and padding nodes: random complex; the smooth double-cumsum
    vector of tests/test_gpu_persist.py; unit impulses (phases differ per system) at the crossings of `rows` and `cols`."""
    rng = np.random.default_rng(seed)
    x = np.zeros((S_, NZP, NYP), complex)
    x[:, 1:nz, 1:ny] = rng.standard_normal((S_, nz - 1, ny - 1)) + 1j * rng.standard_normal((S_, nz - 1, ny - 1))
    smooth = np.cumsum(np.cumsum(x, axis=1), axis=2) / 50.0 * (np.abs(x) > 0)
    imp = np.zeros_like(x)
    for s in range(S_):
        for r in rows:
            for c in cols:
                imp[s, r, c] = np.exp(1j * (0.7 * s + 0.3 * r + 0.11 * c))
    return {"random": x, "smooth": smooth, "impulses": imp}


def seam_mask(NZP, NYP, ny, nz, row_blocks=None, column_parts=1):
    """the interior nodes of the two rows on either side of every row-block seam and, with two column parts, of the two columns on
    either side of the split"""
    nb = -(-(nz - 1) // PS_OWN) if row_blocks is None else row_blocks
    mk = np.zeros((NZP, NYP), bool)
    for b in range(1, nb):
        mk[PS_OWN * b:PS_OWN * b + 2, :] = True
    if column_parts == 2:
        c0 = 16 * ((NYP + 31) // 32)
        mk[:, c0 - 1:c0 + 1] = True
    inner = np.zeros_like(mk)
    inner[1:nz, 1:ny] = True
    return mk & inner


def relmax_seams(a, b, mask):
    """relmax restricted to the nodes of `mask`: a seam error is measured against the values AT the seam"""
    return float(np.abs(a - b)[mask].max() / np.abs(b)[mask].max()) if mask.any() else 0.0


def bf16_distance(ref, V, x):
    """Per system: relmax of F_modal(bf16(V)) against F_modal(V) on the vector x (padded layout) -- what the one deliberate
    approximation of the mixed-precision kernels, the rounded eigenbasis, amounts to in exact arithmetic."""
    Vb = bf16(V)
    return [relmax(ref.F_modal(s, Vb, V)(ref.interior(x[s])), ref.F_modal(s, V)(ref.interior(x[s]))) for s in range(ref.S)]
