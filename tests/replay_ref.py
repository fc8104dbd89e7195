"""Field replay: the reference for everything AROUND the two solves, evaluated from the fields a context returns.

The oracle computes its fields with its own direct solves, so an end-to-end comparison sees the receiver, source and
gradient-tail kernels only through the solve error (1e-10 of the largest component).  Here the oracle's own functions are
fed the fields fetched from the implementation under test -- HipContext.fields() / .fields(adjoint=True), or the host
emulation's X / Lam -- and no solve takes place:

  data      oracle.compFieldsAtRxTE / TM on the two receiver rows of the fetched fields, then _compMTResp (tipper:
            tests/tipper_ref.tipper_table on the same fields);
  misfit    0.5 sum |W (pred - obs)|^2 of the implementation's own pred, in long double;
  adjoint   oracle.compJacTMatVec with datVec = W^2 (pred - obs) and, in place of each factorisation, an object whose
            solve(rhs) returns the fetched lambda and records || A lambda - rhs || / || rhs || with the oracle's assembled
            Aii (complex symmetric: A^T = A).  rhs is sVec[ii], the interior adjoint source of that system;
  gradient  the same call's terms (keep), split into three shares per active cell:
              (a) TE cell terms                PTv of the TE systems
              (b) TM cell terms + Q-terms      PTv + BTvii2 of the TM systems, QTv of both
              (c) boundary-derivative terms    BTvii + BTvio (TE), BTvii1 + BTvio (TM)
            each with its absolute-summand total A_i: the sum of the magnitudes of the complex products the share of
            cell i is added up from (a: w area/4 |e lambda| per corner node; b: the edge products |grad h| |grad lambda|
            of the interior and of the boundary part separately, as the oracle adds them, and |Q| |v| per datum; c:
            |dBC| |w| per boundary node).

The oracle's documented approximations stay as they are: the kernels mirror them.  In particular
BTvii2 uses the oracle's own epsilon-free boundary values of getBCderivTM, not the fetched ones (substituting them
changes the term by 2e-4).  The kernels compute those values themselves (the 1-D recurrences, out of scope here), which
limits share (b): see BC_REL.

A tipper datum is presented to compJacTMatVec as a ZXY datum of a virtual receiver nRx + r whose rows of L and Q are
tipper_ref.tipper_te's -- one TE system per frequency then carries the impedance's and the tipper's sources together, as
on the device.

BARS (tests/test_replay_host.py fixes the constants: reference against the host emulation, every problem below)
  data, misfit, (a), (b)   C_x 2^-53 A_i, C_x = 4 x the largest ratio seen there (fma contraction and reduction order on
                           the device are what the factor 4 is for); for (b) in the cells with an edge on the mesh boundary
                           plus 4 x the reference's spread of its boundary values and BC_REL x the boundary part of A_i
  adjoint residual         4 x options.tol
  (c)                      4 x the reference's own spread (dense against structured dBC; sigma one ulp up, one ulp down
                           and with two seeded draws of random signs) + C_BND 2^-53 A_i + the rounding of the two
                           gradients it is the difference of
"""
from __future__ import annotations

import contextlib
import copy

import numpy as np
import scipy.sparse as sp

from hmcmt2d_amd import synthetic as S, invsetup as I
from hmcmt2d_amd.structs import MTData
from oracle import hmcmt_oracle as O
from tests import tipper_ref as TR

U = 2.0 ** -53

# 4 x the largest ratio |emulation - replay| / (2^-53 A_i) that tests/test_replay_host.py sees over P1 .. P6 (asserted there to
# stay below a quarter of these; the measured values are in DESIGN.md 4.5a)
C_DATA = 45.0          # 11.1 at P6-130 (2.3 .. 8.8 elsewhere)
C_MISFIT = 140.0       # 34.7 at P2: 1800 terms added one after the other (at most 6.8 elsewhere)
C_TE = 18.0            # 4.34 at P4
C_TM = 2.0             # 0.45 at P1, cells without an edge on the mesh boundary (the total holds |G| |h| per edge end, as the
                       # oracle's sparse products add them, where the kernels subtract the two ends first)
# Share (b) in the cells WITH an edge on the mesh boundary is limited by the reference: BTvii2 takes getBCderivTM's boundary
# values, which the kernels compute themselves (1-D recurrences through every layer, out of scope here).  What the bar adds
# for it: 4 x the reference's own spread of those values (sigma one ulp up / down / random signs) carried through the term,
# and BC_REL x the boundary part of A_i for the rest (4 x 1.61e-11 at P4; at most 9.3e-14 elsewhere).
BC_REL = 6.5e-11
# Share (c): what the emulation's boundary-derivative terms differ by from the reference's beyond 4 x the reference's own
# spread, in units of 2^-53 A_i: 1.08e6 at P4 (1.3e-10 A_i), 3.3e5 at P1, 2.7e5 at P2, at most 7.4e4 elsewhere, in the first earth rows --
# the two implementations of the 1-D sensitivity, which this check does not separate from their contraction.
C_BND = 4.4e6
DEEP_ROWS = 3          # rows where the oracle's 1-D sensitivity is ill-conditioned (App. B.7): no cap on bar (c) there
CAP_C = 1e-7           # elsewhere bar (c) stays below this fraction of the cell's boundary-term magnitude A_i


# ------------------------------------------------------------------------------------------------------------ problems
def _mesh_nodes(mesh):
    yN = np.concatenate([[0.0], np.cumsum(mesh.yLen)]) - mesh.origin[0]
    zN = np.concatenate([[0.0], np.cumsum(mesh.zLen)]) - mesh.origin[1]
    return yN, zN


def receivers(mesh, n, rng):
    """n receivers, seeded uniform over the whole mesh width; the first four forced: onto the first and the last interior
    node, into the first and the last cell column."""
    yN, _ = _mesh_nodes(mesh)
    rx = yN[0] + (yN[-1] - yN[0]) * (0.002 + 0.996 * rng.random(n))
    rx[:4] = [yN[1], yN[-2], yN[0] + 0.37 * mesh.yLen[0], yN[-1] - 0.41 * mesh.yLen[-1]]
    return np.sort(rx)


def _finish(mesh, data, rng, fixed_cell=False, mask=None, obs=None, err=None):
    ny, nt = mesh.gridSize
    nair = len(mesh.airLayer)
    if mask is not None:
        data.dataID = mask.copy()
        data.rxID, data.freqID, data.dtID = data.rxID[mask], data.freqID[mask], data.dtID[mask]
    n = len(data.rxID)
    comp = np.array(data.dataComp)[data.dtID - 1]
    if obs is None:
        if data.dataType == "Impedance":
            sgn = np.where(comp == "ZXY", 1.0, np.where(comp == "ZYX", -1.0, 0.0))
            amp = np.where(comp == "TZY", 0.0, 0.02)
            obs = (amp + 0.01 * rng.standard_normal(n)) * np.where(sgn == 0.0, 1.0, sgn) * (1 + 1j)
            err = np.where(comp == "TZY", 2e-2, 2e-3)
        else:
            rho = np.char.startswith(comp, "Rho")
            obs = np.where(rho, 100.0 * (1 + 0.1 * rng.standard_normal(n)),
                           np.where(comp == "PhsXY", 45.0, -135.0) + 2.0 * rng.standard_normal(n))
            err = np.where(rho, 5.0, 1.0)
    mesh.sigma = np.concatenate([np.full(ny * nair, S.SIG_AIR), np.full(ny * (nt - nair), 0.01)])
    fix = [S.SIG_AIR]
    if fixed_cell:
        mesh.sigma[ny * nair + 5] = 0.3
        fix.append(0.3)
    inv = I.setupInverseDataModel(mesh, fix, 0.0, 0.0, obs, err)
    m = np.log(0.01) + 0.4 * rng.standard_normal(len(inv.strModel))
    return mesh, data, inv, m


def _tiny_mesh():
    return S.make_mesh(12, 8, npad_y=3, npad_z=3, nair=3)


def _wide_mesh():
    return S.make_mesh(70, 10, npad_y=5, npad_z=4, nair=2)


def problem(name):
    """(mesh, data, inv, m) of P1 .. P6 (the table in tests/test_gpu_replay.py)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "P1":
        mesh = _tiny_mesh()
        return _finish(mesh, S.make_data_layout(S.log_freqs(3), receivers(mesh, 4, rng)), rng)
    if name == "P2":
        mesh = _tiny_mesh()
        return _finish(mesh, S.make_data_layout(S.log_freqs(3), receivers(mesh, 300, rng)), rng)
    if name in ("P3-256", "P3-257"):
        mesh = _wide_mesh()
        return _finish(mesh, S.make_data_layout([3.7], receivers(mesh, int(name[3:]), rng)), rng)
    if name == "P4":
        mesh = S.make_mesh(136, 14, npad_y=7, npad_z=8, nair=7)
        data = S.make_data_layout([0.2, 0.02], receivers(mesh, 300, rng))
        mask = rng.random(len(data.rxID)) > 0.25
        mask[(data.rxID == 17) & (data.freqID == 1) & (data.dtID == 1)] = False        # no TE datum at one frequency
        mask[(data.rxID == 17) & (data.freqID == 1) & (data.dtID == 2)] = True
        mask[data.rxID == 150] = False                                               # a receiver without data
        return _finish(mesh, data, rng, fixed_cell=True, mask=mask)
    if name == "P5":
        mesh = _tiny_mesh()
        rng2 = np.random.default_rng(sum(map(ord, "P2")))                             # P2's survey
        return _finish(mesh, S.make_rhophase_layout(S.log_freqs(3), receivers(mesh, 300, rng2)), rng)
    if name in ("P6-128", "P6-130", "P6-130T"):
        mesh = _wide_mesh()
        nrx = 128 if name == "P6-128" else 130
        return _finish(mesh, S.make_tipper_layout([3.7], receivers(mesh, nrx, rng), with_impedance=not name.endswith("T")), rng)
    raise KeyError(name)


PROBLEMS = ("P1", "P2", "P3-256", "P3-257", "P4", "P5", "P6-128", "P6-130", "P6-130T")


# ------------------------------------------------------------------------------------------------------------ the replay
class _Fetched:
    """Stands in for a factorisation: solve(rhs) returns the fetched field and records the residual."""

    def __init__(self, Aii, lam_ii):
        self.Aii, self.lam, self.res, self.rhs = Aii, lam_ii, None, None

    def solve(self, rhs):
        self.rhs = np.array(rhs)
        nr = np.linalg.norm(rhs)
        self.res = float(np.linalg.norm(self.Aii @ self.lam - rhs) / nr) if nr > 0 else 0.0
        return self.lam.copy()


class Replay:
    def __init__(self, mesh, data, inv, m):
        self.mesh = copy.deepcopy(mesh)
        self.data, self.inv, self.m = data, inv, np.asarray(m, dtype=float)
        self.sigma = TR.sigma_of(inv, self.m)
        self.mesh.sigma = self.sigma.copy()
        O.setupTensorMesh2D(self.mesh)
        self.ny, self.nz = self.mesh.gridSize
        self.yN, self.zN = _mesh_nodes(self.mesh)
        self.zid = O._find_zid(self.zN, data.rxLoc[0, 1])
        self.nF, self.nR = len(data.freqs), data.rxLoc.shape[0]
        self.ii, self.io = O.getBoundaryIndex(self.ny, self.nz)
        self.ntip = sum(c in TR.TIPPER for c in data.dataComp)
        if self.ntip and data.dataType != "Impedance":
            raise NotImplementedError("RealTZY / ImagTZY")
        self._Aii = None

    # -- data ---------------------------------------------------------------------------------------------------------
    def pred(self, exTE, hxTM):
        """The data of the fetched forward fields, in the masked table order (complex; real for Rho_Pha)."""
        d, ny, zid = self.data, self.ny, self.zid
        id0 = slice(zid * (ny + 1), (zid + 1) * (ny + 1))
        id1 = slice((zid + 1) * (ny + 1), (zid + 2) * (ny + 1))
        sigma1, zLen1 = self.sigma[zid * ny:(zid + 1) * ny], self.mesh.zLen[zid]
        resp = {}
        for mode, F, fn in (("XY", exTE, O.compFieldsAtRxTE), ("YX", hxTM, O.compFieldsAtRxTM)):
            if not any(mode in c for c in d.dataComp):
                continue
            r = np.zeros((self.nF, self.nR, 2))
            for f, freq in enumerate(d.freqs):
                omega = 2 * np.pi * freq
                F01 = np.stack([F[id0, f], F[id1, f]], axis=1)
                En, Hd = fn(omega, d.rxLoc, self.yN, zLen1, sigma1, F01)
                r[f] = O._compMTResp(omega, En, Hd, d.dataType)
            resp[mode] = r
        T = TR.tipper_table(self.mesh, d, exTE) if self.ntip else None
        cols = []
        for c in d.dataComp:
            if c == "TZY":
                cols.append(T)
            elif c in ("ZXY", "ZYX"):
                cols.append(resp[c[1:]][:, :, 0] + 1j * resp[c[1:]][:, :, 1])
            else:
                cols.append(resp[c[-2:]][:, :, 0 if c.startswith("Rho") else 1] + 0j)
        table = np.stack(cols, axis=2).reshape(-1)[np.asarray(d.dataID, dtype=bool)]
        return table if d.dataType == "Impedance" else table.real.copy()

    def misfit(self, pred):
        r = (self.inv.dataW * (np.asarray(pred) - self.inv.obsData)).astype(np.clongdouble)
        return 0.5 * np.sum(r.real * r.real + r.imag * r.imag, dtype=np.longdouble)

    # -- gradient -----------------------------------------------------------------------------------------------------
    def Aii(self):
        """{(mode, freq): the oracle's assembled interior matrix} (its forward solver's, kept)."""
        if self._Aii is None:
            keep = {}
            O.MT2DFwdSolver(self.mesh, TR.full_impedance(self.data), keep=keep)
            self._Aii = keep["Aii"]
        return self._Aii

    def _layout(self):
        """The data as compJacTMatVec takes them: tipper data as ZXY data of the virtual receivers nRx .. 2 nRx-1."""
        d = self.data
        if not self.ntip:
            return d
        comps = list(d.dataComp[:len(d.dataComp) - self.ntip]) or ["ZXY"]
        if "ZXY" not in comps:
            comps = ["ZXY"] + comps
        tip = np.array([d.dataComp[k - 1] in TR.TIPPER for k in d.dtID])
        dt = np.array([comps.index("ZXY" if t else d.dataComp[k - 1]) + 1 for k, t in zip(d.dtID, tip)], dtype=np.int64)
        return MTData(np.vstack([d.rxLoc, d.rxLoc]), d.freqs, "Impedance", comps, d.rxID + self.nR * tip, d.freqID, dt,
                      None, True, any("YX" in c for c in comps))

    @contextlib.contextmanager
    def _recording(self, rec):
        """The oracle's receiver rows (with the tipper's for the virtual receivers) and boundary contractions, recorded."""
        te, tm, dbct = O.getDataFuncSensTE, O.getDataFuncSensTM, O._dBCT_times
        nR, ntip = self.nR, self.ntip

        def rows_te(omega, rx, F01, dataType):
            L, Q = te(omega, rx, F01, dataType)
            if ntip:
                LT, QT = TR.tipper_te(omega, rx, F01)[1:]
                L, Q = sp.vstack([L[:nR], LT[nR:]]).tocsr(), sp.vstack([Q[:nR], QT[nR:]]).tocsr()
            rec[("TE", omega)] = (L, Q)
            return L, Q

        def rows_tm(omega, rx, F01, dataType):
            L, Q = tm(omega, rx, F01, dataType)
            rec[("TM", omega)] = (L, Q)
            return L, Q

        def contract(freq, yLen, zLen, sigma, source, activeIdx, vecs):
            outs, bc = dbct(freq, yLen, zLen, sigma, source, activeIdx, vecs)
            ny, nz = len(yLen), len(zLen)
            _, dL, dR, dM = O.getBCDerivParts(freq, yLen, zLen, sigma, source)
            A = np.zeros((nz, ny))
            for v in vecs:
                A[:, 0] += np.abs(dL).T @ np.abs(v[ny + 1:ny + nz + 1])
                A[:, -1] += np.abs(dR).T @ np.abs(v[ny + nz + 1:ny + 2 * nz + 1])
                vb = np.abs(v[ny + 2 * nz + 1:])
                colw = np.zeros(ny)
                colw[:-1] += yLen[:-1] / (yLen[:-1] + yLen[1:]) * vb
                colw[1:] += yLen[1:] / (yLen[:-1] + yLen[1:]) * vb
                A += np.abs(dM)[:, None] * colw[None, :]
            rec[("bnd", source, freq)] = A.reshape(-1)[activeIdx]
            rec[("vecs", source, freq)] = [np.array(v) for v in vecs]
            return outs, bc

        O.getDataFuncSensTE, O.getDataFuncSensTM, O._dBCT_times = rows_te, rows_tm, contract
        try:
            yield
        finally:
            O.getDataFuncSensTE, O.getDataFuncSensTM, O._dBCT_times = te, tm, dbct

    def _jtv(self, fields, lam, pred, rec):
        d = self._layout()
        datVec = self.inv.dataW * (self.inv.dataW * (np.asarray(pred) - self.inv.obsData))     # (HMCSampler.jl:298-304)
        fake = {mode: [_Fetched(self.Aii()[(mode, f)], lam[mi][self.ii, k]) for k, f in enumerate(self.data.freqs)]
                for mi, mode in enumerate(("TE", "TM"))}
        keep = {}
        with self._recording(rec):
            O.compJacTMatVec(fields[0], fields[1], datVec, self.mesh, d, self.inv.activeIdx, fake["TE"], fake["TM"], False, keep)
        return keep.get("terms", {}), fake, d, datVec

    def _spread(self, rec, terms, dMsigF, Gii, Gio):
        """The reference's own spread per active cell (before the chain rule): of the boundary-derivative terms -- the dense
        dBC against the structured one, the 1-D sensitivities at sigma one ulp up, one ulp down and with seeded random
        signs, contracted with the recorded boundary weights -- and, from the same calls' boundary values, of BTvii2."""
        mesh, act = self.mesh, self.inv.activeIdx
        n = len(act)
        sigmas = [np.nextafter(self.sigma, np.inf), np.nextafter(self.sigma, 0.0)]
        for seed in (1, 2):
            up = np.random.default_rng(seed).random(self.sigma.size) < 0.5
            sigmas.append(np.where(up, sigmas[0], sigmas[1]))
        variants = [np.zeros(n, dtype=complex) for _ in range(len(sigmas) + 2)]       # [0] the base, [1] dense, then sigmas
        sp_b = np.zeros(n)
        for (mode, k), t in terms.items():
            src, freq = "E" if mode == "TE" else "H", self.data.freqs[k]
            vecs = rec[("vecs", src, freq)]
            outs, bc0 = O._dBCT_times(freq, mesh.yLen, mesh.zLen, self.sigma, src, act, vecs)
            variants[0] += outs[0] + outs[1]
            dBC = O.getBCDerivMatrix(freq, mesh.yLen, mesh.zLen, self.sigma, src)[0][:, act]
            variants[1] += dBC.T @ vecs[0] + dBC.T @ vecs[1]
            for q, s in enumerate(sigmas):
                outs, bc = O._dBCT_times(freq, mesh.yLen, mesh.zLen, s, src, act, vecs)
                variants[2 + q] += outs[0] + outs[1]
                if mode == "TM":
                    sp_b = np.maximum(sp_b, dMsigF.T @ (np.abs(Gio @ (bc - bc0)) * np.abs(Gii @ t["eVal"])))
        sp_c = np.zeros(n)
        for v in variants[1:]:
            sp_c = np.maximum(sp_c, np.abs(v.real - variants[0].real))
        return sp_c, sp_b, variants[0].real

    @staticmethod
    def _share_c(terms, n):
        c = np.zeros(n)
        for (mode, _), t in terms.items():
            c += (t["BTvii"] + t["BTvio"]).real if mode == "TE" else (t["BTvii1"] + t["BTvio"]).real
        return c

    def gradient(self, fields, lam, pred, spread=True):
        """Shares and summand totals of the gradient w.r.t. m = ln sigma per active cell, the adjoint residual of every
        system that carries data, the systems that carry none.  fields = (exTE, hxTM), lam likewise, (nNode, nFreq)."""
        inv, mesh, ny = self.inv, self.mesh, self.ny
        n = len(inv.activeIdx)
        rec = {}
        terms, fake, d, datVec = self._jtv(fields, lam, pred, rec)
        act = O.activeCellMatrix(inv.activeIdx, ny * self.nz)
        Grad = mesh.Grad
        Gii, Gio = Grad[:, self.ii], Grad[:, self.io]
        dMsigCN = (mesh.AveCN[self.ii, :] @ mesh.Face @ act).tocsr()
        dMsigF = abs(mesh.AveCF @ mesh.Face @ O.sdiag(-1.0 / self.sigma ** 2) @ act).tocsr()
        a, b, A_a, A_b, A_bc, A_c = (np.zeros(n) for _ in range(6))
        res, nodata = {}, []
        comps = list(d.dataComp)
        for mi, mode in enumerate(("TE", "TM")):
            for k, freq in enumerate(self.data.freqs):
                if (mode, k) not in terms:
                    nodata.append((mode, k))
                    continue
                t, omega = terms[(mode, k)], 2 * np.pi * freq
                res[(mode, k)] = fake[mode][k].res
                ev = t["eVal"]
                if mode == "TE":
                    a += t["PTv"].real
                    A_a += omega * (dMsigCN.T @ np.abs(fields[0][self.ii, k] * ev))
                    A_c += rec[("bnd", "E", freq)]
                else:
                    b += (t["PTv"] + t["BTvii2"]).real
                    gl = abs(Gii) @ np.abs(ev)
                    bpart = dMsigF.T @ ((abs(Gio) @ np.abs(t["bc_sens"])) * gl)
                    A_b += dMsigF.T @ ((abs(Gii) @ np.abs(fields[1][self.ii, k])) * gl) + bpart
                    A_bc += bpart
                    A_c += rec[("bnd", "H", freq)]
                b += t["QTv"].real
                # |Q|^T |v| with compJacTMatVec's own choice of rows (pick)
                Q = abs(rec[(mode, omega)][1]).tocsr()
                indF = np.nonzero(d.freqID == k + 1)[0]
                names = (("RhoXY", "PhsXY") if mode == "TE" else ("RhoYX", "PhsYX")) if O._is_rho_phase(d.dataType) else \
                    (("ZXY",) if mode == "TE" else ("ZYX",))
                for j, cn in enumerate(names):
                    idd = indF[d.dtID[indF] == comps.index(cn) + 1]
                    A_b += (Q[d.rxID[idd] - 1 + j * d.rxLoc.shape[0], :].T @ np.abs(datVec[idd]))[inv.activeIdx]
        c = self._share_c(terms, n)
        e = np.exp(self.m)
        out = dict(terms=terms, a=e * a, b=e * b, c=e * c, A_a=e * A_a, A_b=e * A_b, A_bc=e * A_bc, A_c=e * A_c, res=res, nodata=nodata,
                   deep=(inv.activeIdx // ny) >= self.nz - DEEP_ROWS)
        if spread:
            sp_c, sp_b, c0 = self._spread(rec, terms, dMsigF, Gii, Gio)
            assert np.array_equal(c0, c)
            out["spread_c"], out["spread_b"] = e * sp_c, e * sp_b
        return out


# ------------------------------------------------------------------------------------------------------------ the bars
def bar_data(pred):
    return C_DATA * U * np.abs(pred)


def bar_misfit(misfit):
    return C_MISFIT * U * float(misfit)


def bar_ab(g):
    return C_TE * U * g["A_a"] + C_TM * U * g["A_b"] + 4.0 * g["spread_b"] + BC_REL * g["A_bc"]


def bar_c(g):
    """For the full gradient minus the one without boundary terms: both are rounded sums of all three shares (the last
    additions and the chain rule's product: two roundings each, of at most the whole total)."""
    return 4.0 * g["spread_c"] + C_BND * U * g["A_c"] + 4.0 * U * (g["A_a"] + g["A_b"] + g["A_c"])
