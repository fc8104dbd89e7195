"""Wall time per sample of the samplers, interleaved in one session on one MI355X -> profiles/chain_time.log.

  (a) runHMCSampler(device_leapfrog=True): the host loop around hmcmt_leapfrog (the parent's product sampler)
  (b) runHMCSampler(device_chain=True)
  (c) runHMCSampler(device_chain=True, keep_samples=False)
  (d) (c) with both accumulators of the commit on: hist={} (every cell, 300 bins) and data_moments=True.  Its figure leaves out the
      one read-back of the counters at the end of the run (timed again on the live chain and reported as d_readback_ms): with a
      handful of samples per run it would otherwise be the figure
  (e) (c) with the autocovariance accumulator on: ess={} (every cell, 63 lags).  Its figure leaves out the two read-outs at the end
      of the run (chain_acov and chain_ess, timed again on the live chain and reported apart as e_acov_readout_ms and
      e_ess_readout_ms), for the same reason.  With a handful of samples per run every commit of (e) has count < maxlag, so most
      lags still fill their head sums H_k (16 bytes per lag) and the steady branch (ring read, fma into S_k: 24 bytes per lag) is
      not in (e)'s figure.  It is timed apart: one more chain with ess={} of maxlag + 1 + STEADY samples, with HIP-event pairs round
      every k_chain_acov launch in place in the commit (hmcmt_debug_chain_acov_time) -> acov_commit_us: the mean per launch of the
      commits with count < maxlag ("filling") and of those behind them ("steady"), each interval including its two event records
  (f) (c) with the covariance accumulator on: cov={"rows": 64 cells} -- under 8 sites at 8 depths, chosen by sitePPDTargets -- at the
      default batch.  Its figure leaves out the two read-outs at the end of the run (chain_cov and chain_corr, timed again on the
      live chain and reported as f_cov_readout_ms and f_corr_readout_ms).  The full matrix is timed apart at cfg3 (--cov-full): per
      batch length 1, 8 and 16 one chain with cov_begin(every cell), HIP-event pairs round every k_chain_cov_commit and
      k_chain_cov_flush launch in place (hmcmt_debug_chain_cov_time) -> cov_full_us: the mean per launch, the flush's achieved bytes
      per second against its design traffic 16 nrow nAC, and beside them a plain device-to-device copy of an array of S's size
at cfg3 and cfg5 with bench.py's settings near the true model (L = 8, dt = 0.03), and beside them the floor: L times the per-step
time bench.py reports for its near_true_state chain in the same session.  Every figure: median of REPS runs of NS samples, with the
minimum and maximum (the spread).  The requirement read off the log: (b) and (c) are not slower than (a) by more than that spread.

    python scripts/gpu_chain_time.py [cfg3 cfg5] [--reps 5] [--samples 6]

One JSON line per configuration is appended to the log; every line carries its own repetitions, samples per run and command line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmcmt2d_amd import sampler, synthetic as S                      # noqa: E402
from hmcmt2d_amd.lib import HipContext                               # noqa: E402
from hmcmt2d_amd.structs import HMCPrior                             # noqa: E402
from tests.helpers import make_problem                               # noqa: E402

L, DT, RHOREF = 8, 0.03, 100.0
MODES = {"a_host_loop_device_leapfrog": dict(device_leapfrog=True),
         "b_device_chain": dict(device_chain=True),
         "c_device_chain_no_samples": dict(device_chain=True, keep_samples=False),
         "d_device_chain_no_samples_hist_data_moments": dict(device_chain=True, keep_samples=False, hist={}, data_moments=True)}
D = "d_device_chain_no_samples_hist_data_moments"
E = "e_device_chain_no_samples_ess"
MAXLAG, STEADY = 63, 24
MODES[E] = dict(device_chain=True, keep_samples=False, ess={})
F = "f_device_chain_no_samples_cov"
MODES[F] = dict(device_chain=True, keep_samples=False, cov={})      # (the rows depend on the mesh: one_run fills them in)


def cov_rows(mesh, data, inv):
    """64 active cells: under 8 of the sites, evenly spaced along the line, at 8 depths evenly spaced in the rows below the air"""
    ys = np.unique(np.asarray(data.rxLoc)[:, 0])
    ys = ys[np.linspace(0, len(ys) - 1, 8).round().astype(int)]
    nair = len(mesh.airLayer)
    zNode = np.concatenate([[0.0], np.cumsum(mesh.zLen)]) - mesh.origin[1]
    zCen = (zNode[:-1] + np.diff(zNode) / 2)[nair:]
    zs = zCen[np.linspace(0, len(zCen) - 1, 8).round().astype(int)]
    return sampler.sitePPDTargets(mesh, inv, ys, zs)


def one_run(name, kw, ns, seed):
    mesh, data, inv, _ = make_problem(name)
    inv.strModel = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])
    prior = HMCPrior(totalsamples=ns, burninsamples=0, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)
    if kw.get("cov") is not None:
        kw = dict(kw, cov={"rows": cov_rows(mesh, data, inv)})
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        warm = HMCPrior(totalsamples=1, burninsamples=0, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)
        import copy
        sampler.runHMCSampler(mesh, data, copy.deepcopy(inv), warm, np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, **kw)   # untimed
        t0 = time.perf_counter()
        _, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx, **kw)
        dt = time.perf_counter() - t0
        back = 0.0
        if kw.get("hist") is not None:                  # the chain is still there: the same read-back once more
            t1 = time.perf_counter()
            ctx.chain_hist()
            back = time.perf_counter() - t1
        if kw.get("ess") is not None:                   # ... and the two read-outs, apart
            t1 = time.perf_counter()
            ctx.chain_acov()
            t2 = time.perf_counter()
            ctx.chain_ess()
            back = (t2 - t1, time.perf_counter() - t2)
        if kw.get("cov") is not None:
            t1 = time.perf_counter()
            ctx.chain_cov()
            t2 = time.perf_counter()
            ctx.chain_corr()
            back = (t2 - t1, time.perf_counter() - t2)
    finally:
        ctx.close()
    if isinstance(back, tuple):
        return 1e3 * (dt - sum(back)) / ns, st.nAccept, tuple(1e3 * b for b in back)
    return 1e3 * (dt - back) / ns, st.nAccept, 1e3 * back


def commit_time(name, seed):
    """mean microseconds per k_chain_acov launch, by HIP events in place, over one chain of MAXLAG + 1 + STEADY samples"""
    mesh, data, inv, _ = make_problem(name)
    inv.strModel = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])
    prior = HMCPrior(totalsamples=MAXLAG + 1 + STEADY, burninsamples=0, dt=DT, timestep=[L, L], sigBounds=[1e-4, 1.0], regParam=1.0)
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        begin = ctx.chain_acov_begin

        def begin_timed(*a, **k):                       # (the sampler begins the accumulator: the events go on right behind it)
            begin(*a, **k)
            ctx.chain_acov_timing(True)

        ctx.chain_acov_begin = begin_timed
        _, st, _ = sampler.runHMCSampler(mesh, data, inv, prior, np.random.default_rng(seed), rhoref=RHOREF, ctx=ctx,
                                         device_chain=True, keep_samples=False, ess={"maxlag": MAXLAG})
        t = ctx.chain_acov_timing()
    finally:
        ctx.close()
    out = {k: {"mean_us": 1e3 * ms / max(n, 1), "launches": n} for k, (ms, n) in t.items()}
    out.update(ntarget=len(st.ess["targets"]), maxlag=MAXLAG, samples=prior.totalsamples, accepted=st.nAccept)
    return out


def d2d_copy_time(name):
    """a plain device-to-device copy of as many bytes as the full matrix S of `name` holds: microseconds per copy, mean of 5 behind
    an untimed one, by events (torch's; taken first in the session, before the library's contexts)"""
    import torch
    n = len(make_problem(name)[2].activeIdx)
    a = torch.zeros(n * n, dtype=torch.float64, device="cuda:0")
    b = torch.empty_like(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    b.copy_(a)                                          # untimed
    reps = 5
    ev[0].record()
    for _ in range(reps):
        b.copy_(a)
    ev[1].record()
    torch.cuda.synchronize()
    us = 1e3 * ev[0].elapsed_time(ev[1]) / reps
    del a, b
    torch.cuda.empty_cache()
    return us


def cov_full_time(name, seed, copy_us):
    """the full matrix: mean microseconds per commit and per flush launch for the batch lengths 1, 8 and 16, by HIP events in place,
    the chain driven as the sampler drives it (no read-out: nrow x nAC doubles would cross to the host); copy_us: d2d_copy_time of
    the same session"""
    mesh, data, inv, _ = make_problem(name)
    start = np.log(S.true_model_sigma(mesh, block=True)[inv.activeIdx])
    n = len(start)
    rng = np.random.default_rng(seed)
    out = {"nAC": n, "nrow": n, "S_bytes": 8 * n * n, "design_bytes_per_flush": 16 * n * n}
    ctx = HipContext(mesh, data, inv, device_id=0)
    try:
        ref = np.log(np.ones(n) / RHOREF)
        ctx.set_prior(ref, inv.Wm, sampler.setMassMatrix(n, 1.0)[0])
        ctx.chain_begin(start, DT, 1.0, np.log(1e-4), 0.0, burnin=0)
        for B, ns in ((1, 8), (8, 32), (16, 64)):
            ctx.chain_cov_begin(None, B)
            ctx.chain_cov_timing(True)
            acc = 0
            for _ in range(ns):
                ctx.chain_momentum(rng.standard_normal(n))
                acc += ctx.chain_step(L, rng.random())[0]["accepted"]
            t = ctx.chain_cov_timing(False)
            flush_us = 1e3 * t["flush"][0] / max(t["flush"][1], 1)
            out[f"batch_{B}"] = {"commit_us": 1e3 * t["commit"][0] / max(t["commit"][1], 1), "commits": t["commit"][1], "flush_us": flush_us,
                                 "flushes": t["flush"][1], "flush_design_GBps": 16 * n * n / (flush_us * 1e-6) / 1e9 if flush_us else None,
                                 "flush_us_per_sample": flush_us / B, "accepted": acc}
        ctx.chain_end()
    finally:
        ctx.close()
    out["d2d_copy_of_S"] = {"us": copy_us, "GBps_read_plus_write": 16 * n * n / (copy_us * 1e-6) / 1e9}
    out["flush_batch_8_over_copy"] = out["batch_8"]["flush_design_GBps"] / out["d2d_copy_of_S"]["GBps_read_plus_write"]
    return out


def bench_floor(name):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "96", "--warmup", "16", "--config", name, "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900).stdout
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    near = res.get("extras", res).get("near_true_state", {})
    sps = near.get("steps_per_s", res.get("value"))
    return 1e3 * L / sps, sps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["cfg3", "cfg5"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=6)
    ap.add_argument("--no-floor", action="store_true")
    ap.add_argument("--cov-full", nargs="*", default=["cfg3"], help="configurations whose full covariance matrix is timed (default cfg3)")
    a = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = open(os.path.join(ROOT, "profiles", "chain_time.log"), "a")
    copy_us = {name: d2d_copy_time(name) for name in a.configs if name in a.cov_full}
    for name in a.configs:
        ms = {k: [] for k in MODES}
        acc, back, eback, fback = {}, [], [], []
        for rep in range(a.reps):                       # interleaved: a, b, c, d, e, f, a, b, ...
            for k, kw in MODES.items():
                t, nacc, rb = one_run(name, kw, a.samples, 100 + rep)
                ms[k].append(t); acc[k] = nacc
                if k == D:
                    back.append(rb)
                if k == E:
                    eback.append(rb)
                if k == F:
                    fback.append(rb)
                print(f"{name} rep {rep} {k}: {t:.3f} ms per sample", file=sys.stderr, flush=True)
        line = {"config": name, "argv": sys.argv[1:], "L": L, "dt": DT, "samples_per_run": a.samples, "reps": a.reps, "ms_per_sample": {}}
        for k, v in ms.items():
            line["ms_per_sample"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "accepted_last_run": acc[k]}
        spread = max(max(v) - min(v) for v in ms.values())
        med = {k: statistics.median(v) for k, v in ms.items()}
        line["spread_ms"] = spread
        line["b_minus_a_ms"] = med["b_device_chain"] - med["a_host_loop_device_leapfrog"]
        line["c_minus_a_ms"] = med["c_device_chain_no_samples"] - med["a_host_loop_device_leapfrog"]
        line["b_and_c_within_spread_of_a"] = bool(line["b_minus_a_ms"] <= spread and line["c_minus_a_ms"] <= spread)
        line["d_minus_c_ms"] = med[D] - med["c_device_chain_no_samples"]
        line["d_within_spread_of_c"] = bool(abs(line["d_minus_c_ms"]) <= spread)
        line["d_readback_ms"] = statistics.median(back)
        line["e_minus_c_ms"] = med[E] - med["c_device_chain_no_samples"]
        line["e_within_spread_of_c"] = bool(abs(line["e_minus_c_ms"]) <= spread)
        line["e_acov_readout_ms"] = statistics.median(b[0] for b in eback)
        line["e_ess_readout_ms"] = statistics.median(b[1] for b in eback)
        line["acov_commit_us"] = commit_time(name, 100)
        line["f_minus_c_ms"] = med[F] - med["c_device_chain_no_samples"]
        line["f_within_spread_of_c"] = bool(abs(line["f_minus_c_ms"]) <= spread)
        line["f_cov_readout_ms"] = statistics.median(b[0] for b in fback)
        line["f_corr_readout_ms"] = statistics.median(b[1] for b in fback)
        if name in a.cov_full:
            line["cov_full_us"] = cov_full_time(name, 100, copy_us[name])
            line["cov_full_batch_8_share_of_c"] = 1e-3 * (line["cov_full_us"]["batch_8"]["commit_us"] + line["cov_full_us"]["batch_8"]["flush_us_per_sample"]) / med["c_device_chain_no_samples"]
        if not a.no_floor:
            floor, sps = bench_floor(name)
            line["floor_ms_per_sample_L_times_bench_step"] = floor
            line["bench_near_true_steps_per_s"] = sps
            line["c_above_floor"] = med["c_device_chain_no_samples"] / floor - 1.0
        print(json.dumps(line)); log.write(json.dumps(line) + "\n"); log.flush()


if __name__ == "__main__":
    main()
