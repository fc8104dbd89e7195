"""Golden individual rows of the explicit Jacobian at the headline size: `python tests/golden/make_jac_rows.py` writes
tests/golden/cfg3_jacrows.npz (rows 1-3) and tests/golden/cfg3_jacrows2.npz (rows 4-6): two files, each under the repository's
1 MiB limit for a committed file (a row is 20000 complex doubles, 320 kB, and does not compress).

Six rows of J (dZ/dsigma of the active cells, data order) of cfg3 at the model the tests use (helpers.make_problem("cfg3")),
each from the oracle's compJacTMatVec with datVec = e_k and i e_k: J_k = Re J^T conj(e_k) + i Re J^T conj(i e_k)
(compJacTMatVec returns Re(J^T conj(datVec))).  The rows span the highest and the lowest frequency, both polarisations, an edge
and a centre receiver.  Read by tests/test_gpu_jacobian.py::test_cfg3_rows_equal_the_golden_rows."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import hmcmt_oracle as O            # noqa: E402
from tests.helpers import GOLDEN, make_problem  # noqa: E402


def row_index(data, f, r, d):
    return int(np.flatnonzero((data.freqID == f) & (data.rxID == r) & (data.dtID == d))[0])


def main():
    mesh, data, inv, m = make_problem("cfg3")
    nF, nR = len(data.freqs), data.rxLoc.shape[0]
    picks = [(1, 1, 1), (1, nR // 2 + 1, 2), (1, nR, 1), (nF, 1, 2), (nF, nR // 2 + 1, 1), (nF // 2, nR, 2)]
    rows = np.array([row_index(data, *p) for p in picks])
    sigma = inv.bgModel.copy()
    sigma[inv.activeIdx] += np.exp(m)
    mesh.sigma = sigma
    if not mesh.setup:
        O.setupTensorMesh2D(mesh)
    _, fwd = O.MT2DFwdSolver(mesh, data)
    J = np.empty((len(rows), len(m)), dtype=np.complex128)
    for q, k in enumerate(rows):
        e = np.zeros(len(data.rxID), dtype=np.complex128)
        e[k] = 1.0
        re = O.compJacTMatVec(fwd.exTE, fwd.hxTM, e, mesh, data, inv.activeIdx, fwd.AinvTE, fwd.AinvTM, False)
        im = O.compJacTMatVec(fwd.exTE, fwd.hxTM, 1j * e, mesh, data, inv.activeIdx, fwd.AinvTE, fwd.AinvTM, False)
        J[q] = re + 1j * im
        print(f"row {k} (freq {data.freqID[k]}, rx {data.rxID[k]}, dt {data.dtID[k]}) done", flush=True)
    np.savez(os.path.join(GOLDEN, "cfg3_jacrows.npz"), rows=rows[:3], J=J[:3])
    np.savez(os.path.join(GOLDEN, "cfg3_jacrows2.npz"), rows=rows[3:], J=J[3:])


if __name__ == "__main__":
    main()
