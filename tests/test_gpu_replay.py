"""The kernels AROUND the two solves against a field replay (tests/replay_ref.py): k_rxall / k_rx (impedance, tipper,
residual, vbar, rxCoef), k_src (adjoint sources, receiver-layer Q-terms, the misfit sum), k_misfit and the gradient tail
k_wb_gradcell, k_bcsens_pre, k_bcsens_contract, k_gradfinal.  The reference is evaluated from the context's OWN fields
(HipContext.fields(), .fields(adjoint=True)), so the solve error -- all an end-to-end comparison with the oracle can see at the
1e-10 level -- drops out, and every datum and every active cell is held to a bar of a few rounding errors of its own summands.

  problem  mesh                              survey                                       what it reaches
  P1       12 x 8 earth rows + 3 air         3 frequencies, 4 receivers                   baseline; every receiver at an edge
  P2       the same                          300 receivers (~25 per cell), 1800 data      item branch of k_src (nRx > 256); second
                                                                                          pass and ragged tail of the misfit sums
  P3-256   70 x 10 + 2 air                   1 frequency, 256 receivers                   the LDS table, full; two source blocks
  P3-257   the same                          257 receivers                                one past the table
  P4       136 x 14 + 7 air (nz = 21)        2 frequencies, 300 receivers, a quarter of   two Q-term and two boundary-weight blocks per
                                             the data masked, a receiver without a TE     system; ragged quarters of k_bcsens_contract;
                                             datum at one frequency, one without data,    empty rows of srStart
                                             one fixed earth cell
  P5       P2's survey as Rho_Pha            two data per (system, receiver)              rho / phase forms of item_resid
  P6-128   P3's mesh, ZXY ZYX TZY            128 receivers = 256 functionals              tipper, the table full
  P6-130   the same                          130 receivers = 260 functionals              tipper, item branch
  P6-130T  TZY alone                         130 receivers                                TM systems off: lambda exactly zero

Every receiver set is seeded uniform over the whole mesh width (several receivers per cell: overlapping stencil windows) with
one receiver on the first interior node, one on the last, one in the first cell column and one in the last (clampk).  Each
problem runs with HMCMT_PERSIST=1 and =0: the two launch sites of k_rxall and k_src.  All three meshes lie inside the
persistent kernel's envelope (asserted), so `persist1` means the persistent kernel ran.

The bars are tests/replay_ref.py's; their constants were fixed on the CPU (tests/test_replay_host.py) before any GPU run.
Measured on the MI355X, largest over the 18 cases in units of the bar: data 0.29, misfit 0.014 (k_src) and 0.012
(k_misfit), adjoint residual 0.29, cell terms 0.28, boundary terms 0.36; the whole file takes 3.5 s."""
import os

import numpy as np
import pytest

from hmcmt2d_amd.lib import HipContext, persist_envelope
from tests import replay_ref as RR

pytestmark = pytest.mark.gpu

ROUTES_TOL = 1e-9                       # tests/test_gpu_jvp.py
CASES = [(name, persist) for name in RR.PROBLEMS for persist in ("1", "0")]
IDS = [f"{name}-persist{persist}" for name, persist in CASES]
_runs = {}


def _run(name, persist):
    """One context per case: forward() (k_misfit), grad() (block 0 of k_src), grad() without the boundary terms; the fields
    behind each gradient; the replay of each."""
    key = (name, persist)
    if key in _runs:
        return _runs[key]
    mesh, data, inv, m = RR.problem(name)
    ny, nz = mesh.gridSize
    assert persist_envelope(ny, nz)["column_parts"] >= 1              # inside the persistent kernel's envelope
    old = os.environ.get("HMCMT_PERSIST")
    os.environ["HMCMT_PERSIST"] = persist
    try:
        ctx = HipContext(mesh, data, inv, verify=False)
        try:
            out = dict(name=name, tol=ctx.opts.tol, m=m, inv=inv, data=data)
            out["pred_f"], out["misfit_f"] = ctx.forward(m)
            out["X_f"] = ctx.fields()
            out["pred"], out["misfit"], out["grad"] = ctx.grad(m)
            out["X"], out["Lam"] = ctx.fields(), ctx.fields(adjoint=True)
            ctx.debug_flags(no_boundary_terms=True)
            out["pred_nb"], _, out["grad_nb"] = ctx.grad(m)
            out["X_nb"], out["Lam_nb"] = ctx.fields(), ctx.fields(adjoint=True)
            ctx.debug_flags()
            out["info"], out["stats"] = ctx.persist_info(), ctx.stats()
            if name == "P2":
                u = inv.dataW * (inv.dataW * (out["pred"] - inv.obsData))
                ctx.linearize(m)
                out["jtvp"] = [ctx.jtvp(u), ctx.jtvp(0.5j * u)]
                out["jtvp_blk"] = ctx.jtvp_block(np.stack([u, 0.5j * u]))
        finally:
            ctx.close()
    finally:
        if old is None:
            os.environ.pop("HMCMT_PERSIST", None)
        else:
            os.environ["HMCMT_PERSIST"] = old
    R = RR.Replay(mesh, data, inv, m)
    out["R"] = R
    out["g"] = R.gradient(out["X"], out["Lam"], out["pred"])
    same = all(np.array_equal(out[k][i], out[k + "_nb"][i]) for k in ("X", "Lam") for i in (0, 1)) and \
        np.array_equal(out["pred"], out["pred_nb"])
    out["g_nb"] = out["g"] if same else R.gradient(out["X_nb"], out["Lam_nb"], out["pred_nb"])
    out["same_fields"] = same
    _runs[key] = out
    return out


@pytest.mark.parametrize("name,persist", CASES, ids=IDS)
def test_which_launch_site_ran(name, persist):
    r = _run(name, persist)
    info = r["info"]
    assert r["stats"]["status"] == 0
    assert info["placement_fallbacks"] == 0 and info["timeouts"] == 0, info
    if persist == "1":
        assert info["enabled"] == 1 and info["solves"] >= 5, info       # forward, and forward + adjoint twice
    else:
        assert info["solves"] == 0, info


@pytest.mark.parametrize("name,persist", CASES, ids=IDS)
def test_data_componentwise(name, persist):
    r = _run(name, persist)
    for pred, X in ((r["pred_f"], r["X_f"]), (r["pred"], r["X"]), (r["pred_nb"], r["X_nb"])):      # (forward(): k_rxall without derivatives)
        ref = r["R"].pred(*X)
        err, bar = np.abs(pred - ref), RR.bar_data(ref)
        print(f"replay gpu {name} persist{persist}: data worst {np.max(err / np.abs(ref)):.2e} of |pred| = {np.max(err / bar):.3f} bar")
        assert np.all(err <= bar), (np.max(err / bar), int(np.argmax(err / bar)))


@pytest.mark.parametrize("name,persist", CASES, ids=IDS)
def test_misfit_from_both_kernels(name, persist):
    r = _run(name, persist)
    for label, pred, mis in (("k_src block 0", r["pred"], r["misfit"]), ("k_misfit", r["pred_f"], r["misfit_f"])):
        ref = float(r["R"].misfit(pred))
        err, bar = abs(mis - ref), RR.bar_misfit(ref)
        print(f"replay gpu {name} persist{persist}: misfit ({label}) {err / ref:.2e} relative = {err / bar:.3f} bar")
        assert err <= bar, (label, err / bar)


@pytest.mark.parametrize("name,persist", CASES, ids=IDS)
def test_adjoint_sources_through_the_residual(name, persist):
    r = _run(name, persist)
    nF = len(r["data"].freqs)
    for g, Lam in ((r["g"], r["Lam"]), (r["g_nb"], r["Lam_nb"])):
        worst = max(g["res"].values())
        print(f"replay gpu {name} persist{persist}: adjoint residual worst {worst:.2e} = {worst / (4 * r['tol']):.3f} bar")
        assert worst <= 4 * r["tol"], g["res"]
        for mode, f in g["nodata"]:
            assert not Lam[mode == "TM"][:, f].any(), (mode, f)           # exactly zero
    assert len(r["g"]["res"]) + len(r["g"]["nodata"]) == 2 * nF
    if name == "P6-130T":
        assert r["g"]["nodata"] == [("TM", 0)]


@pytest.mark.parametrize("name,persist", CASES, ids=IDS)
def test_cell_terms_per_cell(name, persist):
    """grad() with the boundary-derivative terms left out against shares (a) + (b)."""
    r = _run(name, persist)
    g = r["g_nb"]
    err, bar = np.abs(r["grad_nb"] - g["a"] - g["b"]), RR.bar_ab(g)
    tot = g["A_a"] + g["A_b"]
    print(f"replay gpu {name} persist{persist}: cell terms worst {np.max(err / tot):.2e} of the summand total = {np.max(err / bar):.3f} bar")
    assert np.all(err <= bar), (np.max(err / bar), int(np.argmax(err / bar)))


@pytest.mark.parametrize("name,persist", CASES, ids=IDS)
def test_boundary_terms_per_cell(name, persist):
    """The full gradient minus the one without boundary terms against share (c)."""
    r = _run(name, persist)
    g, gn = r["g"], r["g_nb"]
    ref, bar = g["c"], RR.bar_c(g)
    if not r["same_fields"]:
        # the second evaluation solved again: its cell terms are those of its own fields
        ref = ref + (g["a"] + g["b"]) - (gn["a"] + gn["b"])
        bar = bar + RR.bar_ab(g) + RR.bar_ab(gn)
    err = np.abs(r["grad"] - r["grad_nb"] - ref)
    shallow = ~g["deep"]
    assert np.all(RR.bar_c(g)[shallow] <= RR.CAP_C * g["A_c"][shallow])         # the condition on the inputs
    print(f"replay gpu {name} persist{persist}: boundary terms worst {np.max(err / g['A_c']):.2e} of the summand total = "
          f"{np.max(err / bar):.3f} bar (same fields in both evaluations: {r['same_fields']})")
    assert np.all(err <= bar), (np.max(err / bar), int(np.argmax(err / bar)))


@pytest.mark.parametrize("persist", ["1", "0"])
def test_products_launch_the_same_sources_P2(persist):
    """exp(m) . jtvp(W^2 r) = grad: jtvp at nvec = 1 launches k_src from host_jacobian.h (300 receivers: its item branch);
    jtvp_block at nvec = 2 launches k_blk_src (the item functions)."""
    r = _run("P2", persist)
    sc = np.abs(r["grad"]).max()
    e1 = np.abs(np.exp(r["m"]) * r["jtvp"][0] - r["grad"]).max() / sc
    e2 = max(np.abs(r["jtvp_blk"][k] - r["jtvp"][k]).max() / np.abs(r["jtvp"][k]).max() for k in (0, 1))
    print(f"replay gpu P2 persist{persist}: jtvp against grad {e1:.2e}, block rows against the single products {e2:.2e}")
    assert e1 < ROUTES_TOL and e2 < ROUTES_TOL, (e1, e2)
