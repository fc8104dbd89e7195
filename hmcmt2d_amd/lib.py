"""ctypes binding of libhmcmt_hip.so (include/hmcmt.h).

There is no fallback: if the shared library is missing, cannot be loaded, or no HIP device is
present, the calls raise.  `build_library()` compiles the in-tree source for gfx950 with hipcc.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

from .marshal import CreateArgs, CREATE_ARGTYPES, c_double_p, c_int64_p

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("HMCMT_LIB_PATH") or os.path.join(HERE, "libhmcmt_hip.so")   # (override: A/B runs of two builds)
CSRC = os.path.join(HERE, "csrc")
SOURCES = [os.path.join(CSRC, "hmcmt_hip.hip"), os.path.join(CSRC, "mumps_shim.hip"), os.path.join(CSRC, "comm.hip")]
HEADERS = [os.path.join(CSRC, h) for h in ("hmcmt_math.h", "hmcmt_items.h", "hmcmt_host.h", "kernels_cocg.h", "kernels_fdm.h",
                                            "kernels_fused.h", "kernels_persist.h", "kernels_persist4.h", "kernels_path.h", "kernels_mass.h", "kernels_chain.h", "kernels_nuts.h", "kernels_map.h", "kernels_jac.h", "kernels_jvp.h", "host_jacobian.h", "host_chain.h", "host_map.h", "hmcmt_knobs.h")] + \
          [os.path.join(HERE, "..", "include", h) for h in ("hmcmt.h", "hmcmt_debug.h", "hmcmt_mumps.h")]

HMCMT_NCAT = 8
CATEGORIES = ["fdm_transform", "tridiagonal", "spmv", "vector_ops", "assembly_bc", "receivers", "gradient",
              "post_smoother"]
PRECOND = {"jacobi": 0, "fdm": 1, "fdmj": 2}
# initial guess of both solves: cold start, the previous evaluation's fields, or those extrapolated along the model path
def _warm_start_code(v):
    if isinstance(v, bool):
        return 2 if v else 0
    return {"cold": 0, "previous": 1, "extrapolate": 2, 0: 0, 1: 1, 2: 2}[v]
# include/hmcmt.h: hmcmt_set_mass kinds and hmcmt_mass_apply operations
HMCMT_MASS_DIAGONAL, HMCMT_MASS_WM, HMCMT_MASS_LOWRANK = 0, 1, 2
HMCMT_MASS_RANK_MAX = 32   # directions of hmcmt_set_mass_lowrank
HMCMT_MASS_OP_INV, HMCMT_MASS_OP_SQRT = 0, 1
ERRORS = {-1: "EINVAL", -2: "ENODEV", -3: "EHIP", -10: "ENOCONV", -11: "EBREAKDOWN", -13: "ENOMEM"}


class HmcmtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libhmcmt_hip: {ERRORS.get(code, code)}: {msg}")
        self.code = code


class Options(C.Structure):
    _fields_ = [("precond", C.c_int32), ("maxit", C.c_int32), ("tol", C.c_double),
                ("check_every", C.c_int32), ("verify", C.c_int32), ("warm_start", C.c_int32),
                ("fdm_precision", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("iters_fwd_max", C.c_int32), ("iters_adj_max", C.c_int32),
                ("iters_fwd_sum", C.c_int32), ("iters_adj_sum", C.c_int32),
                ("err_est_max", C.c_double), ("true_res_max", C.c_double),
                ("status", C.c_int32), ("nsystems", C.c_int32), ("fallback_solves", C.c_int32), ("smoother_sweeps", C.c_int32)]


class ChainRecord(C.Structure):
    """hmcmt_chain_record (include/hmcmt.h): what hmcmt_chain_step reports of one sample."""
    _fields_ = [("accepted", C.c_int32), ("nfevals", C.c_int32), ("K0", C.c_double), ("K1", C.c_double),
                ("D1", C.c_double), ("M1", C.c_double), ("D", C.c_double), ("M", C.c_double), ("hdif", C.c_double),
                ("nsamples", C.c_int64), ("nmoments", C.c_int64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class NutsRecord(C.Structure):
    """hmcmt_nuts_record (include/hmcmt.h): what hmcmt_chain_nuts_sample reports of one sample."""
    _fields_ = [("rec", ChainRecord), ("depth", C.c_int32), ("nleaves", C.c_int32), ("stop", C.c_int32), ("dirs", C.c_uint32),
                ("selected", C.c_int64), ("alpha", C.c_double)]

    def as_dict(self):
        d = self.rec.as_dict()
        d.update({f: getattr(self, f) for f, _ in self._fields_[1:]})
        return d


class DebugNutsArgs(C.Structure):
    """hmcmt_debug_nuts_args (include/hmcmt_debug.h): the device vectors of one leaf's pass."""
    _fields_ = [("n", C.c_int64), ("backward", C.c_int32), ("other_backward", C.c_int32), ("first", C.c_int32), ("merged", C.c_int32),
                ("ndue", C.c_int32), ("reserved_", C.c_int32), ("p", C.c_void_p), ("x", C.c_void_p), ("inv_m", C.c_void_p),
                ("rho_s", C.c_void_p), ("ck_write", C.c_void_p * 3), ("ck_due", (C.c_void_p * 3) * 9), ("rho", C.c_void_p),
                ("rho_next", C.c_void_p), ("p_other", C.c_void_p), ("x_other", C.c_void_p)]


class AdaptOptions(C.Structure):
    """hmcmt_adapt_options (include/hmcmt.h): the warm-up hmcmt_chain_adapt_begin starts."""
    _fields_ = [("nwarmup", C.c_int64), ("adapt_mass", C.c_int32), ("init_buffer", C.c_int32), ("term_buffer", C.c_int32),
                ("base_window", C.c_int32), ("delta", C.c_double), ("gamma", C.c_double), ("t0", C.c_double), ("kappa", C.c_double),
                ("dt_min", C.c_double), ("dt_max", C.c_double)]


class AdaptInfo(C.Structure):
    """hmcmt_adapt_info (include/hmcmt.h): where a warm-up stands."""
    _fields_ = [("step", C.c_int64), ("nwarmup", C.c_int64), ("window_count", C.c_int64), ("next_window_end", C.c_int64),
                ("active", C.c_int32), ("windows_done", C.c_int32), ("dt", C.c_double), ("dt_bar", C.c_double), ("mu", C.c_double),
                ("s_bar", C.c_double), ("alpha_last", C.c_double), ("alpha_sum", C.c_double)]


class AdaptLowrankOptions(C.Structure):
    """hmcmt_adapt_lowrank_options (include/hmcmt.h): the low-rank upgrade of a warm-up (hmcmt_chain_adapt_lowrank)."""
    _fields_ = [("rank", C.c_int32), ("max_samples", C.c_int32), ("cutoff", C.c_double), ("gamma", C.c_double)]


class AdaptLowrankInfo(C.Structure):
    """hmcmt_adapt_lowrank_info (include/hmcmt.h): the last closed window of an upgraded warm-up."""
    _fields_ = [("windows", C.c_int32), ("stored", C.c_int32), ("skipped", C.c_int32), ("dims", C.c_int32), ("rank", C.c_int32),
                ("fallback", C.c_int32), ("stride", C.c_int64), ("theta_min", C.c_double), ("theta_max", C.c_double),
                ("defect", C.c_double), ("host_ms", C.c_double)]


class SketchInfo(C.Structure):
    """hmcmt_sketch_info (include/hmcmt.h): the row sketch of the chain's commit as it stands."""
    _fields_ = [("count", C.c_int64), ("ell", C.c_int32), ("fill", C.c_int32), ("shrinks", C.c_int64), ("Delta", C.c_double),
                ("pivot_given", C.c_int32), ("reserved_", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved_"}


class ChainBlobHeader(C.Structure):
    """hmcmt_chain_blob_header (include/hmcmt.h): what hmcmt_chain_blob_info reports of a chain's checkpoint blob."""
    _fields_ = [("version", C.c_uint32), ("nsections", C.c_uint32), ("total_bytes", C.c_uint64), ("nAC", C.c_int64), ("nData", C.c_int64),
                ("mass_kind", C.c_int32), ("seeded", C.c_uint32), ("nsamples", C.c_int64), ("nmoments", C.c_int64),
                ("tags", C.c_uint32 * 16), ("section_bytes", C.c_uint64 * 16)]


class MapOptions(C.Structure):
    """hmcmt_map_options (include/hmcmt.h): the options of a MAP run (hmcmt_map_begin)."""
    _fields_ = [("history", C.c_int32), ("max_backtracks", C.c_int32), ("c1", C.c_double), ("shrink", C.c_double),
                ("curv_eps", C.c_double), ("gtol", C.c_double)]


class MapRecord(C.Structure):
    """hmcmt_map_record (include/hmcmt.h): what hmcmt_map_begin / hmcmt_map_step report of the state they return."""
    _fields_ = [("iter", C.c_int32), ("status", C.c_int32), ("nfevals", C.c_int32), ("backtracks", C.c_int32), ("resets", C.c_int32),
                ("npairs", C.c_int32), ("pair_stored", C.c_int32), ("nbound", C.c_int32), ("alpha", C.c_double), ("gamma", C.c_double),
                ("phi", C.c_double), ("D", C.c_double), ("M", C.c_double), ("pg_inf", C.c_double), ("pg_2", C.c_double),
                ("gTd", C.c_double), ("sTy", C.c_double), ("phi_trial", C.c_double * 16)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_[:-1]}
        d["phi_trial"] = np.array(self.phi_trial[:])
        return d


class DebugMapArgs(C.Structure):
    """hmcmt_debug_map_args (include/hmcmt_debug.h): the host vectors of one direction."""
    _fields_ = [("n", C.c_int64), ("history", C.c_int32), ("head", C.c_int32), ("count", C.c_int32), ("reserved_", C.c_int32),
                ("rows", C.c_void_p), ("sy", C.c_void_p), ("yy", C.c_void_p), ("m", C.c_void_p), ("g", C.c_void_p),
                ("lo", C.c_double), ("hi", C.c_double), ("alpha", C.c_double),
                ("pg", C.c_void_p), ("d", C.c_void_p), ("mt", C.c_void_p), ("sums", C.c_void_p)]


def build_library(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -shared: cross-compiles without a GPU."""
    newest = max(os.path.getmtime(f) for f in SOURCES + HEADERS)
    if not force and os.path.exists(SO_PATH) and os.path.getmtime(SO_PATH) >= newest:
        return SO_PATH
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC",
           "-Wno-unused-value", "-Wno-pass-failed", "-o", SO_PATH] + SOURCES + ["-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO_PATH


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise HmcmtError(-2, f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback)")
    lib = C.CDLL(SO_PATH)
    vp = C.c_void_p
    lib.hmcmt_default_options.argtypes = [C.POINTER(Options)]
    lib.hmcmt_default_options.restype = None
    lib.hmcmt_create.argtypes = [C.POINTER(vp), C.c_int32] + CREATE_ARGTYPES + [C.POINTER(Options)]
    lib.hmcmt_destroy.argtypes = [vp]
    lib.hmcmt_last_error.argtypes = [vp]
    lib.hmcmt_last_error.restype = C.c_char_p
    lib.hmcmt_set_options.argtypes = [vp, C.POINTER(Options)]
    lib.hmcmt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.hmcmt_get_iters.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.hmcmt_grad.argtypes = [vp, c_double_p, c_double_p, c_double_p, c_double_p]
    lib.hmcmt_forward.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    lib.hmcmt_grad_device.argtypes = [vp, vp, vp, vp, vp]
    lib.hmcmt_forward_device.argtypes = [vp, vp, vp, vp]
    lib.hmcmt_grad_device_async.argtypes = [vp, vp, vp, vp, vp]
    lib.hmcmt_wait.argtypes = [vp]
    lib.hmcmt_set_prior.argtypes = [vp, c_double_p, c_int64_p, c_int64_p, c_double_p, c_double_p]
    lib.hmcmt_leapfrog.argtypes = [vp, c_double_p, c_double_p, C.c_double, C.c_int32, C.c_double, C.c_double,
                                   C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                   C.POINTER(C.c_int32)]
    lib.hmcmt_leapfrog_device.argtypes = [vp, vp, vp, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32,
                                          vp, vp, vp, C.POINTER(C.c_int32)]
    lib.hmcmt_get_fields.argtypes = [vp, C.c_int32, c_double_p, c_double_p]
    lib.hmcmt_set_mass.argtypes = [vp, C.c_int32]
    lib.hmcmt_set_mass_lowrank.argtypes = [vp, c_double_p, C.c_int32, c_double_p, c_double_p]
    lib.hmcmt_mass_apply.argtypes = [vp, C.c_int32, vp, vp, C.c_int32]
    lib.hmcmt_mass_info.argtypes = [vp, c_double_p]
    lib.hmcmt_profile.argtypes = [vp, C.c_int32]
    lib.hmcmt_profile_every.argtypes = [vp, C.c_int32]
    lib.hmcmt_profile_read.argtypes = [vp, c_double_p, c_int64_p]
    lib.hmcmt_profile_counters.argtypes = [vp, c_int64_p]
    lib.hmcmt_profile_overhead.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hmcmt_dims.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.hmcmt_debug_transform.argtypes = [vp, C.c_int32, c_double_p, c_double_p]
    lib.hmcmt_comm_id.argtypes = [C.c_char_p]
    lib.hmcmt_comm_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int32, C.c_char_p]
    lib.hmcmt_allgather_samples.argtypes = [vp, vp, vp, C.c_int64, C.c_int32]
    lib.hmcmt_comm_destroy.argtypes = [vp]
    lib.hmcmt_comm_last_error.argtypes = [vp]
    lib.hmcmt_comm_last_error.restype = C.c_char_p
    for name in ("hmcmt_comm_id", "hmcmt_comm_create", "hmcmt_allgather_samples", "hmcmt_comm_destroy"):
        getattr(lib, name).restype = C.c_int
    lib.hmcmt_debug_flags.argtypes = [vp, C.c_int32]
    lib.hmcmt_debug_spmv.argtypes = [vp, c_double_p, c_double_p]
    lib.hmcmt_debug_precond.argtypes = [vp, c_double_p, c_double_p]
    lib.hmcmt_debug_persist_precond.argtypes = [vp, C.c_int32, c_double_p, c_double_p]
    lib.hmcmt_persist_info.argtypes = [vp, c_int64_p, C.c_int32]
    lib.hmcmt_debug_hog.argtypes = [vp, C.c_int32, C.c_int32]
    lib.hmcmt_next_cu_share.argtypes = [C.c_int32, C.c_int32]
    lib.hmcmt_persist_width.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.hmcmt_persist_order.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), c_int64_p]
    lib.hmcmt_persist_pack.argtypes = [c_double_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), c_double_p]
    lib.hmcmt_persist_envelope.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int64, c_int64_p]
    lib.hmcmt_guard.argtypes = [vp, c_double_p]
    lib.hmcmt_jacobian.argtypes = [vp, c_double_p, C.c_int64, C.c_int64, C.c_int32, c_double_p, C.POINTER(Stats)]
    lib.hmcmt_jacobian_device.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int32, vp, C.POINTER(Stats)]
    lib.hmcmt_sensitivity.argtypes = [vp, c_double_p, C.c_int32, c_double_p, C.POINTER(Stats)]
    lib.hmcmt_linearize.argtypes = [vp, c_double_p]
    lib.hmcmt_linearize_device.argtypes = [vp, vp]
    for name in ("hmcmt_jvp", "hmcmt_jtvp", "hmcmt_gn_hessvec"):
        getattr(lib, name).argtypes = [vp, c_double_p, C.c_int32, c_double_p, C.POINTER(Stats)]
        getattr(lib, name + "_device").argtypes = [vp, vp, C.c_int32, vp, C.POINTER(Stats)]
    for name in ("hmcmt_jvp_block", "hmcmt_jtvp_block", "hmcmt_gn_hessvec_block"):
        getattr(lib, name).argtypes = [vp, c_double_p, C.c_int32, C.c_int32, c_double_p, C.POINTER(Stats)]
        getattr(lib, name + "_device").argtypes = [vp, vp, C.c_int32, C.c_int32, vp, C.POINTER(Stats)]
    for name in JVP_SYMBOLS + CHAIN_SYMBOLS + CHAIN_HIST_SYMBOLS + CHAIN_ACOV_SYMBOLS + CHAIN_COV_SYMBOLS + CHAIN_ADAPT_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib.hmcmt_chain_set_dt.argtypes = [vp, C.c_double]
    lib.hmcmt_chain_set_mass_diag.argtypes = [vp, c_double_p]
    lib.hmcmt_chain_mass_diag.argtypes = [vp, vp, C.c_int32]
    lib.hmcmt_default_adapt_options.argtypes = [C.POINTER(AdaptOptions)]
    lib.hmcmt_default_adapt_options.restype = None
    lib.hmcmt_chain_adapt_begin.argtypes = [vp, C.POINTER(AdaptOptions)]
    lib.hmcmt_chain_adapt_info.argtypes = [vp, C.POINTER(AdaptInfo)]
    lib.hmcmt_chain_adapt_end.argtypes = [vp]
    lib.hmcmt_default_adapt_lowrank_options.argtypes = [C.POINTER(AdaptLowrankOptions)]
    lib.hmcmt_default_adapt_lowrank_options.restype = None
    lib.hmcmt_chain_adapt_lowrank.argtypes = [vp, C.POINTER(AdaptLowrankOptions)]
    lib.hmcmt_chain_adapt_lowrank_info.argtypes = [vp, C.POINTER(AdaptLowrankInfo)]
    lib.hmcmt_chain_set_mass_lowrank.argtypes = [vp, c_double_p, C.c_int32, c_double_p, c_double_p]
    lib.hmcmt_chain_mass_lowrank.argtypes = [vp, C.POINTER(C.c_int32), vp, vp, vp, C.c_int32]
    lib.hmcmt_debug_adapt_lowrank.argtypes = [vp, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int32, c_double_p]
    lib.hmcmt_debug_adapt_lowrank_rows.argtypes = [vp, C.POINTER(C.c_int32), c_double_p, c_double_p]
    lib.hmcmt_debug_adapt_lowrank_time.argtypes = [vp, c_double_p]
    for name in ("hmcmt_chain_adapt_lowrank", "hmcmt_chain_adapt_lowrank_info", "hmcmt_chain_set_mass_lowrank", "hmcmt_chain_mass_lowrank",
                 "hmcmt_debug_adapt_lowrank", "hmcmt_debug_adapt_lowrank_rows", "hmcmt_debug_adapt_lowrank_time"):
        getattr(lib, name).restype = C.c_int
    lib.hmcmt_chain_begin.argtypes = [vp, c_double_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.hmcmt_chain_momentum.argtypes = [vp, c_double_p, C.POINTER(C.c_double)]
    lib.hmcmt_chain_step.argtypes = [vp, C.c_int32, C.c_double, C.POINTER(ChainRecord), c_double_p, c_double_p]
    lib.hmcmt_chain_state.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    lib.hmcmt_chain_moments.argtypes = [vp, C.POINTER(C.c_int64), vp, vp, C.c_int32]
    lib.hmcmt_chain_end.argtypes = [vp]
    lib.hmcmt_chain_set_energy.argtypes = [vp, C.c_double, C.c_double]
    lib.hmcmt_chain_hist_begin.argtypes = [vp, C.c_int64, c_int64_p, C.c_int32, C.c_double, C.c_double]
    lib.hmcmt_chain_hist.argtypes = [vp, C.POINTER(C.c_int64), vp, C.c_int32]
    lib.hmcmt_chain_hist_quantiles.argtypes = [vp, C.c_int32, c_double_p, vp, C.c_int32]
    lib.hmcmt_chain_data_moments_begin.argtypes = [vp]
    lib.hmcmt_chain_data_moments.argtypes = [vp, C.POINTER(C.c_int64), vp, vp, C.c_int32]
    lib.hmcmt_chain_acov_begin.argtypes = [vp, C.c_int64, c_int64_p, C.c_int32]
    lib.hmcmt_chain_acov.argtypes = [vp, C.POINTER(C.c_int64), vp, vp, C.c_int32]
    lib.hmcmt_chain_ess.argtypes = [vp, vp, vp, vp, C.c_int32]
    lib.hmcmt_debug_chain_acov_time.argtypes = [vp, C.c_int32, c_double_p, c_int64_p]
    lib.hmcmt_debug_chain_acov_time.restype = C.c_int
    lib.hmcmt_chain_cov_begin.argtypes = [vp, C.c_int64, c_int64_p, C.c_int32]
    lib.hmcmt_chain_cov.argtypes = [vp, C.POINTER(C.c_int64), vp, vp, vp, C.c_int32]
    lib.hmcmt_chain_corr.argtypes = [vp, vp, C.c_int32]
    lib.hmcmt_debug_chain_cov_time.argtypes = [vp, C.c_int32, c_double_p, c_int64_p]
    lib.hmcmt_debug_chain_cov_time.restype = C.c_int
    lib.hmcmt_chain_sketch_begin.argtypes = [vp, C.c_int32, c_double_p]
    lib.hmcmt_chain_sketch.argtypes = [vp, C.POINTER(SketchInfo), vp, vp, vp, C.c_int32]
    lib.hmcmt_chain_pca.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), vp, vp, C.POINTER(C.c_double), C.c_int32]
    lib.hmcmt_debug_chain_sketch.argtypes = [vp, C.c_int32, C.c_int64, c_double_p, c_double_p, C.POINTER(SketchInfo), vp, vp, vp, vp, C.c_int32,
                                             vp, vp]
    lib.hmcmt_debug_chain_sketch_sums.argtypes = [vp, vp, vp, vp, C.c_int32]
    lib.hmcmt_debug_chain_sketch_sums.restype = C.c_int
    lib.hmcmt_debug_chain_sketch_time.argtypes = [vp, C.c_int32, c_double_p, c_int64_p, C.POINTER(C.c_double)]
    for name in ("hmcmt_chain_sketch_begin", "hmcmt_chain_sketch", "hmcmt_chain_pca", "hmcmt_debug_chain_sketch", "hmcmt_debug_chain_sketch_time"):
        getattr(lib, name).restype = C.c_int
    lib.hmcmt_rng_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    lib.hmcmt_rng_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int64, C.c_int64, c_double_p]
    lib.hmcmt_chain_seed.argtypes = [vp, C.c_uint64, C.c_uint32]
    lib.hmcmt_chain_rng_state.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.hmcmt_chain_rng_seek.argtypes = [vp, C.c_uint64]
    lib.hmcmt_chain_normals.argtypes = [vp, C.c_uint64, vp, C.c_int32]
    lib.hmcmt_chain_sample.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(ChainRecord), c_double_p, c_double_p]
    lib.hmcmt_chain_run.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(ChainRecord), c_double_p, c_double_p, c_int64_p]
    lib.hmcmt_chain_nuts_sample.argtypes = [vp, C.c_int32, C.POINTER(NutsRecord), c_double_p, c_double_p]
    lib.hmcmt_chain_nuts_run.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(NutsRecord), c_double_p, c_double_p, c_int64_p]
    lib.hmcmt_rng_nuts.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    lib.hmcmt_debug_nuts_leaf.argtypes = [vp, C.POINTER(DebugNutsArgs), c_double_p]
    lib.hmcmt_debug_nuts_leaf.restype = C.c_int
    lib.hmcmt_debug_nuts_iters.argtypes = [vp, c_int64_p, C.c_int32]
    lib.hmcmt_debug_nuts_iters.restype = C.c_int
    lib.hmcmt_chain_save_size.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.hmcmt_chain_save.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.hmcmt_chain_restore.argtypes = [vp, vp, C.c_uint64]
    lib.hmcmt_chain_blob_info.argtypes = [vp, C.c_uint64, C.POINTER(ChainBlobHeader)]
    for name in CHAIN_RNG_SYMBOLS + CHAIN_NUTS_SYMBOLS + CHAIN_SAVE_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib.hmcmt_map_default_options.argtypes = [C.POINTER(MapOptions)]
    lib.hmcmt_map_default_options.restype = None
    lib.hmcmt_map_begin.argtypes = [vp, c_double_p, C.c_double, C.c_double, C.c_double, C.POINTER(MapOptions), C.POINTER(MapRecord)]
    lib.hmcmt_map_step.argtypes = [vp, C.POINTER(MapRecord)]
    lib.hmcmt_map_run.argtypes = [vp, C.c_int32, C.POINTER(MapRecord), C.POINTER(C.c_int32)]
    lib.hmcmt_map_state.argtypes = [vp, vp, vp, vp, C.c_int32]
    lib.hmcmt_map_end.argtypes = [vp]
    lib.hmcmt_debug_map_direction.argtypes = [vp, C.POINTER(DebugMapArgs)]
    lib.hmcmt_debug_map_rows.argtypes = [vp, C.POINTER(C.c_int32), c_double_p, c_double_p, c_double_p]
    for name in MAP_SYMBOLS[1:] + ["hmcmt_debug_map_direction", "hmcmt_debug_map_rows"]:
        getattr(lib, name).restype = C.c_int
    lib.hmcmt_debug_fdm_fwd.argtypes = [vp, c_double_p, c_double_p]
    lib.hmcmt_debug_back_post.argtypes = [vp, c_double_p, c_double_p, c_double_p, c_double_p]
    lib.hmcmt_debug_extrap.argtypes = [vp, C.c_int32, c_double_p]
    lib.hmcmt_debug_guess_capture.argtypes = [vp, C.c_int32]
    lib.hmcmt_debug_guess.argtypes = [vp, C.c_int32, c_double_p]
    for name in ("hmcmt_debug_extrap", "hmcmt_debug_guess_capture", "hmcmt_debug_guess"):
        getattr(lib, name).restype = C.c_int
    for name in ("hmcmt_create", "hmcmt_destroy", "hmcmt_set_options", "hmcmt_get_stats", "hmcmt_get_iters",
                 "hmcmt_grad", "hmcmt_forward", "hmcmt_grad_device", "hmcmt_forward_device", "hmcmt_grad_device_async",
                 "hmcmt_wait", "hmcmt_set_prior", "hmcmt_set_mass", "hmcmt_set_mass_lowrank", "hmcmt_mass_apply", "hmcmt_mass_info", "hmcmt_leapfrog", "hmcmt_leapfrog_device", "hmcmt_get_fields", "hmcmt_profile", "hmcmt_profile_every", "hmcmt_profile_read", "hmcmt_profile_counters", "hmcmt_profile_overhead",
                 "hmcmt_dims", "hmcmt_debug_transform", "hmcmt_debug_flags", "hmcmt_debug_spmv", "hmcmt_debug_precond",
                 "hmcmt_debug_fdm_fwd", "hmcmt_debug_back_post", "hmcmt_debug_persist_precond", "hmcmt_persist_info", "hmcmt_guard", "hmcmt_debug_hog", "hmcmt_next_cu_share", "hmcmt_persist_envelope", "hmcmt_persist_width", "hmcmt_persist_order", "hmcmt_persist_pack",
                 "hmcmt_jacobian", "hmcmt_jacobian_device", "hmcmt_sensitivity"):
        getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


# matrix-free Jacobian products at a linearisation point
JVP_SYMBOLS = ["hmcmt_linearize", "hmcmt_linearize_device", "hmcmt_jvp", "hmcmt_jvp_device", "hmcmt_jtvp", "hmcmt_jtvp_device",
               "hmcmt_gn_hessvec", "hmcmt_gn_hessvec_device",
               "hmcmt_jvp_block", "hmcmt_jvp_block_device", "hmcmt_jtvp_block", "hmcmt_jtvp_block_device",
               "hmcmt_gn_hessvec_block", "hmcmt_gn_hessvec_block_device"]
BLOCK_MAX = 32      # include/hmcmt.h: HMCMT_BLOCK_MAX
# the device-resident HMC chain
CHAIN_SYMBOLS = ["hmcmt_chain_begin", "hmcmt_chain_momentum", "hmcmt_chain_step", "hmcmt_chain_state", "hmcmt_chain_moments",
                 "hmcmt_chain_end", "hmcmt_chain_set_energy"]
# the optional accumulators of the chain's commit: histograms of the model, moments of the predicted data
CHAIN_HIST_SYMBOLS = ["hmcmt_chain_hist_begin", "hmcmt_chain_hist", "hmcmt_chain_hist_quantiles",
                      "hmcmt_chain_data_moments_begin", "hmcmt_chain_data_moments"]
HIST_MAXBINS = 4096   # include/hmcmt.h: nbins of hmcmt_chain_hist_begin
# ... and the third one: lagged autocovariances, integrated autocorrelation time and effective sample size
CHAIN_ACOV_SYMBOLS = ["hmcmt_chain_acov_begin", "hmcmt_chain_acov", "hmcmt_chain_ess"]
ACOV_MAXLAG = 1023    # include/hmcmt.h: maxlag of hmcmt_chain_acov_begin
# ... and the fourth one: posterior covariance and correlation between cells
CHAIN_COV_SYMBOLS = ["hmcmt_chain_cov_begin", "hmcmt_chain_cov", "hmcmt_chain_corr"]
COV_BATCH_MAX = 16    # include/hmcmt.h: HMCMT_COV_BATCH_MAX
# ... and the fifth one: a frequent-directions row sketch of the committed models and its principal components
CHAIN_SKETCH_SYMBOLS = ["hmcmt_chain_sketch_begin", "hmcmt_chain_sketch", "hmcmt_chain_pca"]
SKETCH_ELL_MAX = 64   # include/hmcmt.h: HMCMT_SKETCH_ELL_MAX
MASS_RANK_MAX = 32    # include/hmcmt.h: HMCMT_MASS_RANK_MAX
# ... and the warm-up: the chain's step size and diagonal mass between two steps, and their adaptation
CHAIN_ADAPT_SYMBOLS = ["hmcmt_chain_set_dt", "hmcmt_chain_set_mass_diag", "hmcmt_chain_mass_diag", "hmcmt_default_adapt_options",
                       "hmcmt_chain_adapt_begin", "hmcmt_chain_adapt_info", "hmcmt_chain_adapt_end"]
# ... and its low-rank upgrade: directions and factors from the window's draws and gradients, the setter and the read-out of a live chain
CHAIN_ADAPT_LOWRANK_SYMBOLS = ["hmcmt_default_adapt_lowrank_options", "hmcmt_chain_adapt_lowrank", "hmcmt_chain_adapt_lowrank_info",
                               "hmcmt_chain_set_mass_lowrank", "hmcmt_chain_mass_lowrank"]
# ... and the chain's own random numbers: Philox4x32-10 by counter, one call and one wait per sample, one call per run
CHAIN_RNG_SYMBOLS = ["hmcmt_rng_draw", "hmcmt_rng_normals", "hmcmt_chain_seed", "hmcmt_chain_rng_state", "hmcmt_chain_rng_seek",
                     "hmcmt_chain_normals", "hmcmt_chain_sample", "hmcmt_chain_run"]
# ... and the No-U-turn sampler on a seeded chain: the trajectory length chosen per sample
CHAIN_NUTS_SYMBOLS = ["hmcmt_chain_nuts_sample", "hmcmt_chain_nuts_run", "hmcmt_rng_nuts"]
NUTS_DEPTH_MAX = 10   # include/hmcmt.h: HMCMT_NUTS_DEPTH_MAX
# ... and the chain's checkpoint: one blob out, one blob in, a blob's header without a device
CHAIN_SAVE_SYMBOLS = ["hmcmt_chain_save_size", "hmcmt_chain_save", "hmcmt_chain_restore", "hmcmt_chain_blob_info"]
# the MAP model on the device: projected L-BFGS over the library's gradient
MAP_SYMBOLS = ["hmcmt_map_default_options", "hmcmt_map_begin", "hmcmt_map_step", "hmcmt_map_run", "hmcmt_map_state", "hmcmt_map_end"]
MAP_HISTORY_MAX = 32          # include/hmcmt.h: HMCMT_MAP_HISTORY_MAX
MAP_RUNNING, MAP_CONVERGED, MAP_STALLED = 0, 1, 2
MAP_STATUS = {MAP_RUNNING: "RUNNING", MAP_CONVERGED: "CONVERGED", MAP_STALLED: "STALLED"}
MAP_OPTION_KEYS = ("history", "max_backtracks", "c1", "shrink", "curv_eps", "gtol")
MAP_HOOK_NMAX, MAP_SUMS = 0x40000000, 136   # include/hmcmt_debug.h: HMCMT_MAP_HOOK_NMAX, HMCMT_MAP_SUMS
NUTS_CK_MAX, NUTS_SUMS = 9, 21   # include/hmcmt_debug.h: HMCMT_NUTS_CK_MAX, HMCMT_NUTS_SUMS
ADAPT_LOWRANK_KEYS = ("rank", "max_samples", "cutoff", "gamma")
ADAPT_LOWRANK_NMIN, ADAPT_LOWRANK_NMAX = 4, 128   # include/hmcmt.h: max_samples of hmcmt_adapt_lowrank_options
ADAPT_OPTION_KEYS = ("adapt_mass", "init_buffer", "term_buffer", "base_window", "delta", "gamma", "t0", "kappa", "dt_min", "dt_max")
# include/hmcmt.h: the drop-in boundary
PRODUCT_SYMBOLS = JVP_SYMBOLS + CHAIN_SYMBOLS + CHAIN_HIST_SYMBOLS + CHAIN_ACOV_SYMBOLS + CHAIN_COV_SYMBOLS + CHAIN_SKETCH_SYMBOLS + CHAIN_ADAPT_SYMBOLS + CHAIN_ADAPT_LOWRANK_SYMBOLS + CHAIN_RNG_SYMBOLS + CHAIN_NUTS_SYMBOLS + CHAIN_SAVE_SYMBOLS + MAP_SYMBOLS + ["hmcmt_default_options", "hmcmt_create", "hmcmt_destroy", "hmcmt_last_error",
                   "hmcmt_set_options", "hmcmt_get_stats", "hmcmt_get_iters", "hmcmt_grad", "hmcmt_forward",
                   "hmcmt_grad_device", "hmcmt_forward_device", "hmcmt_grad_device_async", "hmcmt_wait",
                   "hmcmt_set_prior", "hmcmt_set_mass", "hmcmt_set_mass_lowrank", "hmcmt_mass_apply", "hmcmt_leapfrog", "hmcmt_leapfrog_device", "hmcmt_get_fields",
                   "hmcmt_guard", "hmcmt_next_cu_share", "hmcmt_jacobian", "hmcmt_jacobian_device", "hmcmt_sensitivity",
                   "hmcmt_comm_id", "hmcmt_comm_create", "hmcmt_allgather_samples", "hmcmt_comm_destroy", "hmcmt_comm_last_error"]
# include/hmcmt_debug.h: instrumentation, introspection of the persistent kernel, test hooks
DEBUG_SYMBOLS = ["hmcmt_profile", "hmcmt_profile_every", "hmcmt_profile_read", "hmcmt_profile_counters", "hmcmt_profile_overhead", "hmcmt_dims",
                 "hmcmt_debug_transform", "hmcmt_debug_flags", "hmcmt_debug_spmv", "hmcmt_debug_precond", "hmcmt_debug_fdm_fwd",
                 "hmcmt_debug_back_post", "hmcmt_debug_persist_precond", "hmcmt_persist_info", "hmcmt_debug_hog", "hmcmt_persist_envelope",
                 "hmcmt_persist_width", "hmcmt_persist_order", "hmcmt_persist_pack", "hmcmt_mass_info", "hmcmt_debug_chain_acov_time",
                 "hmcmt_debug_chain_cov_time", "hmcmt_debug_extrap", "hmcmt_debug_guess_capture", "hmcmt_debug_guess", "hmcmt_debug_nuts_leaf",
                 "hmcmt_debug_nuts_iters", "hmcmt_debug_adapt_lowrank", "hmcmt_debug_adapt_lowrank_rows",
                 "hmcmt_debug_adapt_lowrank_time", "hmcmt_debug_chain_sketch", "hmcmt_debug_chain_sketch_sums",
                 "hmcmt_debug_chain_sketch_time", "hmcmt_debug_map_direction", "hmcmt_debug_map_rows"]
EXPORTED_SYMBOLS = PRODUCT_SYMBOLS + DEBUG_SYMBOLS


def map_options(**kw):
    """hmcmt_map_options from the library's defaults (hmcmt_map_default_options: no device needed) and the given keys, checked against
    the ranges of include/hmcmt.h before any call that touches the device: ValueError names the first one out of range."""
    unknown = sorted(set(kw) - set(MAP_OPTION_KEYS))
    if unknown:
        raise ValueError(f"unknown MAP option(s) {unknown}; the options are {MAP_OPTION_KEYS}")
    o = MapOptions()
    load_library().hmcmt_map_default_options(C.byref(o))
    for k, v in kw.items():
        if k in ("history", "max_backtracks"):
            if int(v) != v:
                raise ValueError(f"MAP option {k} must be an integer")
            v = int(v)
        else:
            v = float(v)
        setattr(o, k, v)
    if not 1 <= o.history <= MAP_HISTORY_MAX:
        raise ValueError(f"MAP option history must be within 1 .. {MAP_HISTORY_MAX}")
    if not 0 <= o.max_backtracks <= 15:
        raise ValueError("MAP option max_backtracks must be within 0 .. 15")
    if not 0 < o.c1 < 1 or not 0 < o.shrink < 1:
        raise ValueError("MAP options c1 and shrink must lie strictly between 0 and 1")
    if not (np.isfinite(o.curv_eps) and o.curv_eps >= 0 and np.isfinite(o.gtol) and o.gtol >= 0):
        raise ValueError("MAP options curv_eps and gtol must be finite and not negative")
    return o


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _rng_ints(seed, stream, t=0):
    seed, stream, t = int(seed), int(stream), int(t)
    if not (0 <= seed < 2 ** 64 and 0 <= stream < 2 ** 32 and 0 <= t < 2 ** 64):
        raise ValueError(f"seed and t are uint64 and stream is uint32; got seed {seed}, stream {stream}, t {t}")
    return seed, stream, t


def rng_draw(seed, stream, t, Lmin, Lmax):
    """(L, u) of draw t of the chain (seed, stream): hmcmt_rng_draw, pure arithmetic on the host, no GPU needed."""
    lib = load_library()
    L, u = C.c_int32(), C.c_double()
    rc = lib.hmcmt_rng_draw(*_rng_ints(seed, stream, t), int(Lmin), int(Lmax), C.byref(L), C.byref(u))
    if rc != 0:
        raise HmcmtError(rc, "hmcmt_rng_draw: need 1 <= Lmin <= Lmax")
    return int(L.value), float(u.value)


def rng_nuts(seed, stream, t, kind, index):
    """(forward, u) of a NUTS sample's draws beside the momentum: kind 0, doubling `index` -- its direction and the uniform of its
    merge; kind 1, the sample's index-th leaf -- the uniform of its selection (forward is 0).  hmcmt_rng_nuts, on the host."""
    lib = load_library()
    f, u = C.c_int32(), C.c_double()
    index = int(index)
    if not 0 <= index < 2 ** 32:
        raise ValueError(f"index is uint32; got {index}")
    rc = lib.hmcmt_rng_nuts(*_rng_ints(seed, stream, t), int(kind), index, C.byref(f), C.byref(u))
    if rc != 0:
        raise HmcmtError(rc, "hmcmt_rng_nuts: need kind 0 (index < 32) or 1 (index < 2^30)")
    return int(f.value), float(u.value)


def rng_normals(seed, stream, t, n, a0=0):
    """The unclipped standard normals of the cells a0 .. a0 + n - 1 in draw t of the chain (seed, stream): hmcmt_rng_normals, the
    device's numbers to libm accuracy, computed on the host, no GPU needed."""
    lib = load_library()
    z = np.empty(max(int(n), 0))                             # (a negative n is the library's to refuse)
    rc = lib.hmcmt_rng_normals(*_rng_ints(seed, stream, t), int(a0), int(n), _dp(z))
    if rc != 0:
        raise HmcmtError(rc, "hmcmt_rng_normals: need a0 >= 0, n >= 0 and a0 + n <= 2^31")
    return z


def chain_blob_info(blob):
    """The header of a chain's checkpoint blob (HipContext.chain_save) as a dict -- version, total_bytes, nAC, nData, mass_kind, seeded,
    nsamples, nmoments, sections: [(tag, bytes)] in table order, the tags as four-character strings.  hmcmt_chain_blob_info: the
    container is validated completely (magic, version, lengths, section table, checksum) on the host, no GPU needed; HmcmtError
    (EINVAL) for anything that is no intact version-1 blob."""
    lib = load_library()
    blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, dtype=np.uint8)
    h = ChainBlobHeader()
    rc = lib.hmcmt_chain_blob_info(blob.ctypes.data, blob.size, C.byref(h))
    if rc != 0:
        raise HmcmtError(rc, "hmcmt_chain_blob_info: not an intact chain blob of version 1")
    out = {f: int(getattr(h, f)) for f in ("version", "total_bytes", "nAC", "nData", "mass_kind", "seeded", "nsamples", "nmoments")}
    out["sections"] = [(int(h.tags[k]).to_bytes(4, "little").decode("ascii"), int(h.section_bytes[k])) for k in range(h.nsections)]
    return out


def adapt_lowrank_options(options):
    """hmcmt_adapt_lowrank_options from a dict (or True / None: the defaults); ValueError for an unknown key or a value out of range --
    checked here so that a wrong request is refused before a context exists (the library checks the same)."""
    options = {} if options is None or options is True else dict(options)
    unknown = sorted(set(options) - set(ADAPT_LOWRANK_KEYS))
    if unknown:
        raise ValueError(f"adapt lowrank: unknown option(s) {unknown}; known: {list(ADAPT_LOWRANK_KEYS)}")
    o = AdaptLowrankOptions(rank=8, max_samples=64, cutoff=2.0, gamma=1e-5)
    for k, v in options.items():
        setattr(o, k, type(getattr(o, k))(v))
    if not 1 <= o.rank <= HMCMT_MASS_RANK_MAX:
        raise ValueError(f"adapt lowrank: rank {o.rank} is outside 1 .. {HMCMT_MASS_RANK_MAX}")
    if not ADAPT_LOWRANK_NMIN <= o.max_samples <= ADAPT_LOWRANK_NMAX:
        raise ValueError(f"adapt lowrank: max_samples {o.max_samples} is outside {ADAPT_LOWRANK_NMIN} .. {ADAPT_LOWRANK_NMAX}")
    if not (np.isfinite(o.cutoff) and o.cutoff > 1.0):
        raise ValueError(f"adapt lowrank: cutoff {o.cutoff} must be finite and > 1")
    if not (np.isfinite(o.gamma) and o.gamma > 0.0):
        raise ValueError(f"adapt lowrank: gamma {o.gamma} must be finite and > 0")
    return o


def lowrank_mass_arrays(nAC, invM, U, lam):
    """The arguments of HipContext.set_mass_lowrank as contiguous float64 arrays; ValueError for a wrong shape (the values are the
    library's to judge, a rank outside 1 .. HMCMT_MASS_RANK_MAX included)."""
    U = np.ascontiguousarray(U, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    if U.ndim != 2 or U.shape[1] != nAC:
        raise ValueError(f"U must be [rank, nAC = {nAC}], C-ordered; got shape {U.shape}")
    if lam.shape != (U.shape[0],):
        raise ValueError(f"lam must have one entry per row of U ({U.shape[0]}); got shape {lam.shape}")
    if invM is not None:
        invM = np.ascontiguousarray(invM, dtype=np.float64)
        if invM.shape != (nAC,):
            raise ValueError(f"invM must have nAC = {nAC} entries; got shape {invM.shape}")
    return invM, U, lam


class SampleComm:
    """hmcmt_comm: the RCCL communicator of this process (one process per GPU) for the all-gather of sample blocks."""
    ID_BYTES = 128

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = C.create_string_buffer(SampleComm.ID_BYTES)
        rc = lib.hmcmt_comm_id(buf)
        if rc != 0:
            raise HmcmtError(rc, (lib.hmcmt_comm_last_error(None) or b"").decode())
        return buf.raw

    def __init__(self, device_id, nranks, rank, uid):
        self.lib = load_library()
        if len(uid) != self.ID_BYTES:
            raise ValueError("the RCCL unique id has 128 bytes")
        h = C.c_void_p()
        rc = self.lib.hmcmt_comm_create(C.byref(h), int(device_id), int(nranks), int(rank), uid)
        if rc != 0:
            raise HmcmtError(rc, (self.lib.hmcmt_comm_last_error(None) or b"").decode())
        self.h, self.nranks, self.rank = h, int(nranks), int(rank)

    def allgather(self, block):
        """host float64 block of this rank -> [nranks, len(block)] with every rank's block"""
        send = np.ascontiguousarray(block, dtype=np.float64).reshape(-1)
        recv = np.empty(self.nranks * send.size)
        rc = self.lib.hmcmt_allgather_samples(self.h, send.ctypes.data, recv.ctypes.data, send.size, 0)
        if rc != 0:
            raise HmcmtError(rc, (self.lib.hmcmt_comm_last_error(self.h) or b"").decode())
        return recv.reshape(self.nranks, send.size)

    def allgather_device(self, d_send, d_recv, count):
        rc = self.lib.hmcmt_allgather_samples(self.h, d_send, d_recv, int(count), 1)
        if rc != 0:
            raise HmcmtError(rc, (self.lib.hmcmt_comm_last_error(self.h) or b"").decode())

    def close(self):
        if self.h:
            self.lib.hmcmt_comm_destroy(self.h)
            self.h = None


def persist_envelope(ny, nz, cus_per_xcd=32, nsystems=32):
    """Would a mesh of ny x nz cells (nz incl. the air layers) run the one-launch-per-solve kernel, and in which shape
    (hmcmt_persist_envelope: pure arithmetic, no GPU needed)?  column_parts == 0: outside its envelope."""
    lib = load_library()
    out = (C.c_int64 * 6)()
    rc = lib.hmcmt_persist_envelope(int(ny), int(nz), int(cus_per_xcd), int(nsystems), out)
    if rc != 0:
        raise HmcmtError(rc, "hmcmt_persist_envelope: ny >= 2, nz >= 3, cus_per_xcd >= 1, nsystems >= 1")
    return dict(zip(("column_parts", "threads_half", "workgroups_per_system", "slab_modes", "lds_bytes", "slots_per_xcd"), (int(x) for x in out)))


def persist_pack(cost, queues):
    """(order, makespan, makespan of the index order): the packing behind HipContext.persist_order on the caller's costs
    (hmcmt_persist_pack: pure arithmetic, no GPU needed) -- systems onto `queues` queues that take turns, position
    queue + queues * round -> system."""
    lib = load_library()
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    order = (C.c_int32 * len(cost))()
    m1, m0 = C.c_double(0.0), C.c_double(0.0)
    rc = lib.hmcmt_persist_pack(_dp(cost), len(cost), int(queues), order, C.byref(m1))
    if rc == 0:
        rc = lib.hmcmt_persist_pack(_dp(cost), len(cost), int(queues), None, C.byref(m0))
    if rc != 0:
        raise HmcmtError(rc, "hmcmt_persist_pack: costs >= 0, at least one system and one queue")
    return np.array(list(order)), float(m1.value), float(m0.value)


class HipContext:
    """One GPU context: the drop-in for the reference's per-call solver state."""
    live = 0          # contexts created and not yet closed in this process (a second one on a device switches BOTH to the
                      # launch-per-phase loop: tests/conftest.py fails a test that leaves one behind)

    def __init__(self, mtMesh, mtData, invParam, device_id=0, precond="fdmj", tol=None, maxit=None,
                 verify=False, check_every=None, warm_start=True, fdm_precision="mixed", cu_share=None):
        """cu_share = (index, count): the context is confined to that share (count 1, 2 or 4) of the CUs of every XCD
        (hmcmt_next_cu_share): `count` contexts -- chains -- on one device then run their persistent solve kernels side by side."""
        self.lib = load_library()
        self.args = CreateArgs(mtMesh, mtData, invParam)
        opts = Options()
        self.lib.hmcmt_default_options(C.byref(opts))
        opts.precond = PRECOND[precond]
        if precond == "jacobi" and maxit is None:
            maxit = 20000
        if tol is not None:
            opts.tol = tol
        if maxit is not None:
            opts.maxit = maxit
        if check_every is not None:
            opts.check_every = check_every
        opts.verify = int(verify)
        opts.warm_start = _warm_start_code(warm_start)
        opts.fdm_precision = {"mixed": 0, "fp64": 1}[fdm_precision]
        self.opts = opts
        h = C.c_void_p()
        if cu_share is not None:
            rc = self.lib.hmcmt_next_cu_share(int(cu_share[0]), int(cu_share[1]))       # (this thread's next create)
            if rc != 0:
                raise HmcmtError(rc, f"cu_share {cu_share}: (index, count) with count 1, 2 or 4")
        rc = self.lib.hmcmt_create(C.byref(h), device_id, *self.args.as_tuple(), C.byref(opts))
        if rc != 0:
            raise HmcmtError(rc, (self.lib.hmcmt_last_error(None) or b"").decode())
        self.h = h
        HipContext.live += 1
        d = (C.c_int32 * 7)()
        self.lib.hmcmt_dims(self.h, d)
        self.NYP, self.NZP, self.S, self.ny, self.nz, self.zid, self.nblk = list(d)
        self.nAC, self.nData, self.nFreq = self.args.nAC, self.args.nData, self.args.nFreq

    # -- helpers ------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise HmcmtError(rc, (self.lib.hmcmt_last_error(self.h) or b"").decode())

    def set_options(self, **kw):
        before = {k: getattr(self.opts, k) for k in kw}
        try:
            self._set_options(**kw)
        except HmcmtError:
            for k, v in before.items():              # (the library kept its options: so does the mirror)
                setattr(self.opts, k, v)
            raise

    def _set_options(self, **kw):
        for k, v in kw.items():
            if k == "precond":
                v = PRECOND[v]
            if k == "fdm_precision":
                v = {"mixed": 0, "fp64": 1}[v]
            if k == "warm_start":
                v = _warm_start_code(v)
            setattr(self.opts, k, v)
        self._check(self.lib.hmcmt_set_options(self.h, C.byref(self.opts)))

    def stats(self):
        s = Stats()
        self._check(self.lib.hmcmt_get_stats(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in Stats._fields_}

    def iters(self):
        it = (C.c_int32 * (2 * self.S))()
        self._check(self.lib.hmcmt_get_iters(self.h, it))
        return np.array(list(it)).reshape(2, self.S)

    # -- hot path -----------------------------------------------------------------------------
    def grad(self, m):
        """compDataGradient: m -> (predData, dataMisfit, dataGrad)."""
        m = np.ascontiguousarray(m, dtype=np.float64)
        if m.shape != (self.nAC,):
            raise ValueError("model vector has the wrong length")
        pred = np.empty(self.nData, dtype=np.complex128)
        grad = np.empty(self.nAC)
        mis = C.c_double()
        self._check(self.lib.hmcmt_grad(self.h, _dp(m), _dp(pred), C.byref(mis), _dp(grad)))
        return (pred.real.copy() if self.args.real_data else pred), mis.value, grad

    def forward(self, m):
        """MT2DFwdSolver + compDataMisfit: m -> (predData, dataMisfit)."""
        m = np.ascontiguousarray(m, dtype=np.float64)
        if m.shape != (self.nAC,):
            raise ValueError("model vector has the wrong length")
        pred = np.empty(self.nData, dtype=np.complex128)
        mis = C.c_double()
        self._check(self.lib.hmcmt_forward(self.h, _dp(m), _dp(pred), C.byref(mis)))
        return (pred.real.copy() if self.args.real_data else pred), mis.value

    def grad_device(self, d_m, d_pred, d_misfit, d_grad):
        """Raw device pointers (ints), e.g. torch tensors' data_ptr()."""
        self._check(self.lib.hmcmt_grad_device(self.h, d_m, d_pred, d_misfit, d_grad))

    def grad_device_async(self, d_m, d_pred, d_misfit, d_grad):
        """Enqueue only (hmcmt_grad_device_async); finish with wait()."""
        self._check(self.lib.hmcmt_grad_device_async(self.h, d_m, d_pred, d_misfit, d_grad))

    def wait(self):
        self._check(self.lib.hmcmt_wait(self.h))

    def forward_device(self, d_m, d_pred, d_misfit):
        self._check(self.lib.hmcmt_forward_device(self.h, d_m, d_pred, d_misfit))

    def fields(self, adjoint=False):
        nn = (self.ny + 1) * (self.nz + 1)
        e = np.empty(nn * self.nFreq, dtype=np.complex128)
        h = np.empty(nn * self.nFreq, dtype=np.complex128)
        self._check(self.lib.hmcmt_get_fields(self.h, int(adjoint), _dp(e), _dp(h)))
        return e.reshape(self.nFreq, nn).T.copy(), h.reshape(self.nFreq, nn).T.copy()

    # -- explicit Jacobian (hmcmt_jacobian / hmcmt_sensitivity) ---------------------------------
    JAC_WRT = {"sigma": 0, "lnsigma": 1}

    def _model(self, m):
        m = np.ascontiguousarray(m, dtype=np.float64)
        if m.shape != (self.nAC,):
            raise ValueError("model vector has the wrong length")
        return m

    def _wrt(self, wrt):
        if wrt not in self.JAC_WRT:
            raise ValueError(f"wrt must be one of {sorted(self.JAC_WRT)}")
        return self.JAC_WRT[wrt]

    def jacobian(self, m, rows=None, wrt="sigma"):
        """Rows of the data Jacobian J (data order) at model m: (nrows, nAC), complex for DataType Impedance, real for
        Rho_Pha.  rows: None (all), a (start, stop) pair or a range with step 1.  wrt "sigma" (compJacMat's J) or "lnsigma"."""
        m = self._model(m)
        r0, r1 = (0, self.nData) if rows is None else ((rows.start, rows.stop) if isinstance(rows, range) else tuple(rows))
        if isinstance(rows, range) and rows.step != 1:
            raise ValueError("rows: a contiguous range")
        if not 0 <= r0 <= r1 <= self.nData:
            raise ValueError(f"rows ({r0}, {r1}): need 0 <= start <= stop <= nData = {self.nData}")
        n = r1 - r0
        width = 1 if self.args.real_data else 2
        J = np.empty((n, self.nAC * width))
        st = Stats()
        self._check(self.lib.hmcmt_jacobian(self.h, _dp(m), r0, n, self._wrt(wrt), _dp(J), C.byref(st)))
        self.jac_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return J if width == 1 else J.view(np.complex128)

    def jacobian_device(self, d_m, row0, nrows, d_J, wrt="sigma"):
        """Raw device pointers (ints): rows row0 .. row0+nrows-1 into d_J ([nrows][nAC], complex interleaved or real)."""
        st = Stats()
        self._check(self.lib.hmcmt_jacobian_device(self.h, d_m, int(row0), int(nrows), self._wrt(wrt), d_J, C.byref(st)))
        self.jac_stats = {f: getattr(st, f) for f, _ in Stats._fields_}

    def sensitivity(self, m, wrt="sigma"):
        """sens[a] = sqrt(sum_k |dataW_k J_ka|^2) over all data (J not materialised)."""
        m = self._model(m)
        out = np.empty(self.nAC)
        st = Stats()
        self._check(self.lib.hmcmt_sensitivity(self.h, _dp(m), self._wrt(wrt), _dp(out), C.byref(st)))
        self.jac_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return out

    # -- matrix-free Jacobian products at a linearisation point ---------------------------------
    def linearize(self, m):
        """Sets the linearisation point of jvp / jtvp / gn_hessvec: a cold forward evaluation at m plus the receiver functionals
        and boundary sensitivities.  Valid until the next evaluating call or set_options."""
        self._check(self.lib.hmcmt_linearize(self.h, _dp(self._model(m))))

    def linearize_device(self, d_m):
        self._check(self.lib.hmcmt_linearize_device(self.h, d_m))

    def _product(self, fn, x, wrt):
        st = Stats()
        out = np.empty(self.nAC if fn != "hmcmt_jvp" else 2 * self.nData)
        self._check(getattr(self.lib, fn)(self.h, _dp(x), self._wrt(wrt), _dp(out), C.byref(st)))
        self.jvp_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return out

    def _data_vector(self, u):
        u = np.ascontiguousarray(u, dtype=np.complex128)
        if u.shape != (self.nData,):
            raise ValueError("data vector has the wrong length")
        return u.view(np.float64)

    def jvp(self, v, wrt="sigma"):
        """J v at the linearisation point (compJacMat(m) @ v, no J): data layout of pred -- complex, real for real data."""
        out = self._product("hmcmt_jvp", self._model(v), wrt).view(np.complex128)
        return out.real.copy() if self.args.real_data else out

    def jtvp(self, u, wrt="sigma"):
        """Re(J^T conj(u)) = real(compJacTMatVec(.., datVec = u, ..)) at the linearisation point: [nAC]."""
        return self._product("hmcmt_jtvp", self._data_vector(u), wrt)

    def gn_hessvec(self, v, wrt="sigma"):
        """Gauss-Newton Hessian product Re(J^H W^2 J) v, W = dataW (no prior term): two solves, no stored matrix."""
        return self._product("hmcmt_gn_hessvec", self._model(v), wrt)

    def _product_device(self, fn, d_in, d_out, wrt):
        st = Stats()
        self._check(getattr(self.lib, fn)(self.h, d_in, self._wrt(wrt), d_out, C.byref(st)))
        self.jvp_stats = {f: getattr(st, f) for f, _ in Stats._fields_}

    def jvp_device(self, d_v, d_Jv, wrt="sigma"):
        """Raw device pointers (ints): v[nAC] -> Jv interleaved complex [nData]."""
        self._product_device("hmcmt_jvp_device", d_v, d_Jv, wrt)

    def jtvp_device(self, d_u, d_JTu, wrt="sigma"):
        """Raw device pointers: u interleaved complex [nData] -> [nAC]."""
        self._product_device("hmcmt_jtvp_device", d_u, d_JTu, wrt)

    def gn_hessvec_device(self, d_v, d_Hv, wrt="sigma"):
        self._product_device("hmcmt_gn_hessvec_device", d_v, d_Hv, wrt)

    # -- block products: several directions per solve -------------------------------------------
    @staticmethod
    def block_input(X, width, single, complex_in=False):
        """A block of directions as a C-ordered (nvec, width) array of float64 (complex128 for data vectors); needs no device.
        A 1-D input is refused: the single-direction method is the one for it."""
        if isinstance(X, np.ndarray) and X.dtype.kind not in "fiuc":
            raise TypeError(f"block of directions: a numeric array, not dtype {X.dtype}")
        X = np.asarray(X)
        if X.dtype.kind not in "fiuc" or (X.dtype.kind == "c" and not complex_in):
            raise TypeError(f"block of directions: {'real or complex' if complex_in else 'real'} numbers, not dtype {X.dtype}")
        if X.ndim == 1:
            raise ValueError(f"block of directions: a 2-D array (nvec, {width}); for one direction use {single}")
        if X.ndim != 2 or X.shape[1] != width:
            raise ValueError(f"block of directions: shape (nvec, {width}), not {X.shape}")
        if not 1 <= X.shape[0] <= BLOCK_MAX:
            raise ValueError(f"block of directions: nvec = {X.shape[0]}, need 1 .. {BLOCK_MAX}")
        return np.ascontiguousarray(X, dtype=np.complex128 if complex_in else np.float64)

    def _product_block(self, fn, X, wrt, nout):
        st = Stats()
        nvec = X.shape[0]
        out = np.empty((nvec, nout))
        self._check(getattr(self.lib, fn)(self.h, _dp(X.view(np.float64)), nvec, self._wrt(wrt), _dp(out), C.byref(st)))
        self.block_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return out

    def jvp_block(self, V, wrt="sigma"):
        """J V at the linearisation point for the rows of V (nvec, nAC), ONE forward-type solve for all of them: (nvec, nData),
        complex, real for real data.  Row j is jvp(V[j])."""
        out = self._product_block("hmcmt_jvp_block", self.block_input(V, self.nAC, "jvp"), wrt, 2 * self.nData).view(np.complex128)
        return out.real.copy() if self.args.real_data else out

    def jtvp_block(self, U, wrt="sigma"):
        """Re(J^T conj(U_j)) for the rows of U (nvec, nData), ONE adjoint-type solve: (nvec, nAC)."""
        return self._product_block("hmcmt_jtvp_block", self.block_input(U, self.nData, "jtvp", complex_in=True), wrt, self.nAC)

    def gn_hessvec_block(self, V, wrt="sigma"):
        """Re(J^H W^2 J) V for the rows of V (nvec, nAC): one solve of each type, the intermediate kept on the device."""
        return self._product_block("hmcmt_gn_hessvec_block", self.block_input(V, self.nAC, "gn_hessvec"), wrt, self.nAC)

    def _product_block_device(self, fn, d_in, nvec, d_out, wrt):
        st = Stats()
        self._check(getattr(self.lib, fn)(self.h, d_in, int(nvec), self._wrt(wrt), d_out, C.byref(st)))
        self.block_stats = {f: getattr(st, f) for f, _ in Stats._fields_}

    def jvp_block_device(self, d_V, nvec, d_JV, wrt="sigma"):
        """Raw device pointers (ints): V [nvec][nAC] -> JV interleaved complex [nvec][nData]."""
        self._product_block_device("hmcmt_jvp_block_device", d_V, nvec, d_JV, wrt)

    def jtvp_block_device(self, d_U, nvec, d_JTU, wrt="sigma"):
        """Raw device pointers: U interleaved complex [nvec][nData] -> [nvec][nAC]."""
        self._product_block_device("hmcmt_jtvp_block_device", d_U, nvec, d_JTU, wrt)

    def gn_hessvec_block_device(self, d_V, nvec, d_HV, wrt="sigma"):
        self._product_block_device("hmcmt_gn_hessvec_block_device", d_V, nvec, d_HV, wrt)

    # -- prior / leapfrog ---------------------------------------------------------------------
    def set_prior(self, mref, Wm, invM):
        Wm = Wm.tocsr()
        self._prior = (np.ascontiguousarray(mref, dtype=np.float64),
                       np.ascontiguousarray(Wm.indptr, dtype=np.int64),
                       np.ascontiguousarray(Wm.indices, dtype=np.int64),
                       np.ascontiguousarray(Wm.data, dtype=np.float64),
                       np.ascontiguousarray(invM, dtype=np.float64))
        a = self._prior
        self._check(self.lib.hmcmt_set_prior(self.h, _dp(a[0]), a[1].ctypes.data_as(c_int64_p),
                                             a[2].ctypes.data_as(c_int64_p), _dp(a[3]), _dp(a[4])))

    def set_mass(self, kind):
        """hmcmt_set_mass: HMCMT_MASS_DIAGONAL (the invM of set_prior) or HMCMT_MASS_WM (M = Wm of set_prior, factored here);
        after set_prior, which returns to the diagonal kind."""
        self._check(self.lib.hmcmt_set_mass(self.h, int(kind)))

    def set_mass_lowrank(self, invM, U, lam):
        """hmcmt_set_mass_lowrank: M^-1 = S (I + U' (diag(lam) - I) U) S with S = diag(sqrt(invM)).  invM [nAC] or None (the
        diagonal in force), U [rank, nAC] C-ordered with orthonormal rows, lam [rank] > 0; 1 <= rank <= HMCMT_MASS_RANK_MAX.
        Ends a running chain, as set_mass does."""
        invM, U, lam = lowrank_mass_arrays(self.nAC, invM, U, lam)
        self._check(self.lib.hmcmt_set_mass_lowrank(self.h, None if invM is None else _dp(invM), int(U.shape[0]), _dp(U), _dp(lam)))

    def mass_apply(self, op, x):
        """hmcmt_mass_apply on a host vector: M^-1 x (HMCMT_MASS_OP_INV) or L x (HMCMT_MASS_OP_SQRT; F x under
        HMCMT_MASS_LOWRANK)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.nAC,):
            raise ValueError("vector has the wrong length")
        y = np.empty(self.nAC)
        self._check(self.lib.hmcmt_mass_apply(self.h, int(op), x.ctypes.data, y.ctypes.data, 0))
        return y

    def mass_apply_device(self, op, d_x, d_y):
        """hmcmt_mass_apply on device pointers (ints); complete on return."""
        self._check(self.lib.hmcmt_mass_apply(self.h, int(op), d_x, d_y, 1))

    def mass_info(self):
        """{kind, factor_s, bandwidth, separable, pcg_iters, box_rows, box_cols} (hmcmt_mass_info)."""
        o = np.zeros(7)
        self._check(self.lib.hmcmt_mass_info(self.h, _dp(o)))
        return {"kind": int(o[0]), "factor_s": float(o[1]), "bandwidth": int(o[2]), "separable": bool(o[3]),
                "pcg_iters": int(o[4]), "box_rows": int(o[5]), "box_cols": int(o[6])}

    def leapfrog(self, m0, p0, dt, L, regParam, lnSigMin, lnSigMax):
        m0 = np.ascontiguousarray(m0, dtype=np.float64)
        p0 = np.ascontiguousarray(p0, dtype=np.float64)
        m1 = np.empty(self.nAC); p1 = np.empty(self.nAC)
        pred = np.empty(self.nData, dtype=np.complex128)
        mis = C.c_double(); mnorm = C.c_double(); nf = C.c_int32()
        self._check(self.lib.hmcmt_leapfrog(self.h, _dp(m0), _dp(p0), dt, L, regParam, lnSigMin, lnSigMax,
                                            _dp(m1), _dp(p1), _dp(pred), C.byref(mis), C.byref(mnorm),
                                            C.byref(nf)))
        return m1, p1, (pred.real.copy() if self.args.real_data else pred), mis.value, mnorm.value, nf.value

    def leapfrog_device(self, d_m, d_p, dt, L, regParam, lnSigMin, lnSigMax, start_grad=0, d_pred=None, d_misfit=None,
                        d_mnorm=None):
        """hmcmt_leapfrog_device: raw device pointers (ints); d_m, d_p are updated in place; finish with wait().
        start_grad: 0 evaluate / 1 start = end model of the previous trajectory / 2 start = its start model."""
        nf = C.c_int32()
        self._check(self.lib.hmcmt_leapfrog_device(self.h, d_m, d_p, dt, L, regParam, lnSigMin, lnSigMax, start_grad,
                                                   d_pred, d_misfit, d_mnorm, C.byref(nf)))
        return nf.value

    # -- the HMC chain on the device (hmcmt_chain_*) ---------------------------------------------
    def chain_begin(self, m_start, dt, regParam, lnSigMin, lnSigMax, burnin=0):
        """Starts a chain at m_start (after set_prior / set_mass): one forward evaluation there.  Returns (D0, M0): data misfit and
        0.5*regParam*(m-mref)'Wm(m-mref) at the start; the predicted data: chain_state()."""
        D0, M0 = C.c_double(), C.c_double()
        self._check(self.lib.hmcmt_chain_begin(self.h, _dp(self._model(m_start)), float(dt), float(regParam), float(lnSigMin),
                                               float(lnSigMax), int(burnin), C.byref(D0), C.byref(M0)))
        return D0.value, M0.value

    def chain_momentum(self, z):
        """p = sqrtM * clip(z, +-2.5) on the device from standard normals z[nAC]; returns the kinetic energy 0.5 p'M^-1 p."""
        K = C.c_double()
        self._check(self.lib.hmcmt_chain_momentum(self.h, _dp(self._model(z)), C.byref(K)))
        return K.value

    def chain_step(self, L, u, outputs=True):
        """One sample: trajectory of L steps, accept test with the uniform u, commit.  Returns (record dict, model, predData): the
        chain's current model and predicted data after the decision, or None for both with outputs=False (nothing O(nAC) comes back)."""
        rec = ChainRecord()
        m = np.empty(self.nAC) if outputs else None
        pred = np.empty(self.nData, dtype=np.complex128) if outputs else None
        self._check(self.lib.hmcmt_chain_step(self.h, int(L), float(u), C.byref(rec), _dp(m) if outputs else None,
                                              _dp(pred) if outputs else None))
        if outputs and self.args.real_data:
            pred = pred.real.copy()
        return rec.as_dict(), m, pred

    def chain_state(self):
        """(current model, momentum buffer, current predicted data) of the chain."""
        m, p = np.empty(self.nAC), np.empty(self.nAC)
        pred = np.empty(self.nData, dtype=np.complex128)
        self._check(self.lib.hmcmt_chain_state(self.h, _dp(m), _dp(p), _dp(pred)))
        return m, p, (pred.real.copy() if self.args.real_data else pred)

    def chain_moments(self):
        """(count, mean[nAC], m2[nAC]) of the samples behind the burn-in: m2 = sum of squared deviations from the mean (Welford)."""
        n = C.c_int64()
        mean, m2 = np.empty(self.nAC), np.empty(self.nAC)
        self._check(self.lib.hmcmt_chain_moments(self.h, C.byref(n), mean.ctypes.data, m2.ctypes.data, 0))
        return int(n.value), mean, m2

    def chain_moments_device(self, d_mean, d_m2):
        """The same into device pointers (ints); returns count."""
        n = C.c_int64()
        self._check(self.lib.hmcmt_chain_moments(self.h, C.byref(n), d_mean, d_m2, 1))
        return int(n.value)

    def chain_set_energy(self, D, M):
        """Replaces the data misfit and prior term the chain holds for its current model (what the next accept test starts from)."""
        self._check(self.lib.hmcmt_chain_set_energy(self.h, float(D), float(M)))

    def chain_end(self):
        self._check(self.lib.hmcmt_chain_end(self.h))

    # -- the MAP model on the device (hmcmt_map_*) -----------------------------------------------
    def map_begin(self, m_start, regParam, lnSigMin, lnSigMax, **options):
        """Starts a MAP run at clip(m_start) (after set_prior): one gradient evaluation there.  options: history, max_backtracks, c1,
        shrink, curv_eps, gtol (include/hmcmt.h; checked here first).  Returns the record of the start state as a dict."""
        o = map_options(**options)
        for name, v in (("regParam", regParam), ("lnSigMin", lnSigMin), ("lnSigMax", lnSigMax)):
            if not np.isfinite(v):
                raise ValueError(f"{name} must be finite")
        rec = MapRecord()
        self._check(self.lib.hmcmt_map_begin(self.h, _dp(self._model(m_start)), float(regParam), float(lnSigMin), float(lnSigMax),
                                             C.byref(o), C.byref(rec)))
        self._map_history = o.history
        return rec.as_dict()

    def map_step(self):
        """One iteration (direction, line search, pair, commit); the record as a dict.  HmcmtError EINVAL once the run has ended."""
        rec = MapRecord()
        self._check(self.lib.hmcmt_map_step(self.h, C.byref(rec)))
        return rec.as_dict()

    def map_run(self, maxiter):
        """Iterates until the status leaves RUNNING or maxiter steps are made; the records as a list of dicts."""
        recs = (MapRecord * max(int(maxiter), 1))()
        n = C.c_int32(0)
        self._check(self.lib.hmcmt_map_run(self.h, int(maxiter), recs, C.byref(n)))
        return [recs[k].as_dict() for k in range(n.value)]

    def map_state(self):
        """(model, full gradient, predicted data) of the run's current state."""
        m, g = np.empty(self.nAC), np.empty(self.nAC)
        pred = np.empty(self.nData, dtype=np.complex128)
        self._check(self.lib.hmcmt_map_state(self.h, m.ctypes.data, g.ctypes.data, pred.ctypes.data, 0))
        return m, g, (pred.real.copy() if self.args.real_data else pred)

    def map_state_device(self, d_m=None, d_grad=None, d_pred=None):
        """The same into device pointers (ints; each may be None)."""
        self._check(self.lib.hmcmt_map_state(self.h, d_m, d_grad, d_pred, 1))

    def map_end(self):
        self._check(self.lib.hmcmt_map_end(self.h))

    def debug_map_direction(self, rows, head, count, sy, yy, m, g, lo, hi, alpha=1.0):
        """Test hook (hmcmt_debug_map_direction): the direction's three kernels on host vectors of any length n.  rows [2 history, n]
        (None with count = 0: history 1), sy, yy [history, history] by slot.  Returns dict(pg, d, mt, coef [72], proj [2 count])."""
        m = np.ascontiguousarray(m, dtype=np.float64); g = np.ascontiguousarray(g, dtype=np.float64)
        n = m.shape[0]
        a = DebugMapArgs()
        keep = [m, g]
        if rows is None:
            H = 1
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float64); sy = np.ascontiguousarray(sy, dtype=np.float64)
            yy = np.ascontiguousarray(yy, dtype=np.float64)
            H = rows.shape[0] // 2
            if rows.shape != (2 * H, n) or sy.shape != (H, H) or yy.shape != (H, H):
                raise ValueError("rows must be [2 history, n], sy and yy [history, history]")
            keep += [rows, sy, yy]
            a.rows, a.sy, a.yy = rows.ctypes.data, sy.ctypes.data, yy.ctypes.data
        pg, d, mt, sums = np.empty(n), np.empty(n), np.empty(n), np.empty(MAP_SUMS)
        a.n, a.history, a.head, a.count = n, H, int(head), int(count)
        a.m, a.g, a.lo, a.hi, a.alpha = m.ctypes.data, g.ctypes.data, float(lo), float(hi), float(alpha)
        a.pg, a.d, a.mt, a.sums = pg.ctypes.data, d.ctypes.data, mt.ctypes.data, sums.ctypes.data
        self._check(self.lib.hmcmt_debug_map_direction(self.h, C.byref(a)))
        return {"pg": pg, "d": d, "mt": mt, "coef": sums[:72].copy(), "proj": sums[72:72 + 2 * int(count)].copy()}

    def debug_map_rows(self):
        """Test hook (hmcmt_debug_map_rows): dict(history, head, count, iter, rows [2 history, nAC], sy, yy [history, history]) of the run."""
        H = getattr(self, "_map_history", MAP_HISTORY_MAX)
        info = (C.c_int32 * 4)()
        rows, sy, yy = np.empty((2 * H, self.nAC)), np.empty((H, H)), np.empty((H, H))
        self._check(self.lib.hmcmt_debug_map_rows(self.h, info, _dp(rows), _dp(sy), _dp(yy)))
        return {"history": info[0], "head": info[1], "count": info[2], "iter": info[3], "rows": rows, "sy": sy, "yy": yy}

    # -- checkpoint and resume (hmcmt_chain_save / hmcmt_chain_restore) ---------------------------
    def chain_save_size(self):
        """Bytes of the blob chain_save returns for the chain as it stands."""
        n = C.c_uint64()
        self._check(self.lib.hmcmt_chain_save_size(self.h, C.byref(n)))
        return int(n.value)

    def chain_save(self):
        """The chain as one blob (uint8 array): state, moments, generator, the mass in force, every accumulator that is on, an
        adaptation that was begun -- include/hmcmt.h has the format.  A read-out: the chain goes on as if it had not been called."""
        blob = np.empty(self.chain_save_size(), dtype=np.uint8)
        n = C.c_uint64()
        self._check(self.lib.hmcmt_chain_save(self.h, blob.ctypes.data, blob.size, C.byref(n)))
        assert n.value == blob.size
        return blob

    def chain_restore(self, blob):
        """A chain from a blob of chain_save, in place of chain_begin and every accumulator's and adaptation's begin call (after
        set_prior, and set_mass for a blob saved under HMCMT_MASS_WM).  No evaluation runs; the first sample behind it evaluates its
        start gradient.  A blob that is refused (HmcmtError EINVAL) leaves a running chain untouched."""
        blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else blob, dtype=np.uint8)
        self._check(self.lib.hmcmt_chain_restore(self.h, blob.ctypes.data, blob.size))
        # the shapes the read-outs of this binding allocate by: what the begin calls would have noted (the blob has passed the library)
        table = chain_blob_info(blob)["sections"]
        at = 64 + 24 * len(table)
        for tag, nbytes in table:
            head = blob[at:at + 24].view(np.int64)
            if tag == "HIST":
                self._hist_shape = (int(head[0]), int(head[1]))
            elif tag == "ACOV":
                self._acov_shape = (int(head[2]) + 1, int(head[0]))
            elif tag == "COV ":
                self._cov_shape = (int(head[0]), self.nAC)
            elif tag == "SKCH":
                self._sketch_ell = int(head[0])
            at += nbytes

    # -- the chain's own random numbers (hmcmt_chain_seed, hmcmt_chain_sample, hmcmt_chain_run) ----
    def chain_seed(self, seed, stream=0):
        """The chain draws its own numbers from here on: Philox4x32-10 keyed by seed, counter (cell, stream, t), t = 0."""
        seed, stream, _ = _rng_ints(seed, stream)
        self._check(self.lib.hmcmt_chain_seed(self.h, seed, stream))

    def chain_rng_state(self):
        """(seed, stream, t): all a checkpoint of the chain's generator needs; t is the index of the next draw."""
        seed, stream, t = C.c_uint64(), C.c_uint32(), C.c_uint64()
        self._check(self.lib.hmcmt_chain_rng_state(self.h, C.byref(seed), C.byref(stream), C.byref(t)))
        return int(seed.value), int(stream.value), int(t.value)

    def chain_rng_seek(self, t):
        self._check(self.lib.hmcmt_chain_rng_seek(self.h, _rng_ints(0, 0, t)[2]))

    def chain_normals(self, t, d_z=None):
        """The device's clipped normals of draw t, [nAC]; with d_z (a device pointer as int) they stay on the device."""
        t = _rng_ints(0, 0, t)[2]
        if d_z is not None:
            self._check(self.lib.hmcmt_chain_normals(self.h, t, d_z, 1))
            return None
        z = np.empty(self.nAC)
        self._check(self.lib.hmcmt_chain_normals(self.h, t, z.ctypes.data, 0))
        return z

    def chain_sample(self, Lmin, Lmax, outputs=True):
        """One sample of a seeded chain: momentum, L in Lmin .. Lmax and u are draw t's; returns what chain_step returns."""
        rec = ChainRecord()
        m = np.empty(self.nAC) if outputs else None
        pred = np.empty(self.nData, dtype=np.complex128) if outputs else None
        self._check(self.lib.hmcmt_chain_sample(self.h, int(Lmin), int(Lmax), C.byref(rec), _dp(m) if outputs else None,
                                                _dp(pred) if outputs else None))
        if outputs and self.args.real_data:
            pred = pred.real.copy()
        return rec.as_dict(), m, pred

    def chain_run(self, nsamples, Lmin, Lmax, outputs=True, check=True):
        """nsamples samples of a seeded chain in one call.  Returns (records, models [nsamples, nAC], preds [nsamples, nData]) -- None
        for both arrays with outputs=False.  A failing sample raises; with check=False the call returns (records, models, preds, rc)
        cut to the samples that were completed."""
        nsamples = int(nsamples)
        rows = max(nsamples, 0)                              # (a negative nsamples is the library's to refuse)
        recs = (ChainRecord * max(rows, 1))()
        models = np.empty((rows, self.nAC)) if outputs else None
        preds = np.empty((rows, self.nData), dtype=np.complex128) if outputs else None
        done = C.c_int64()
        rc = self.lib.hmcmt_chain_run(self.h, nsamples, int(Lmin), int(Lmax), recs, _dp(models) if outputs else None,
                                      _dp(preds) if outputs else None, C.byref(done))
        if check:
            self._check(rc)
        k = int(done.value)
        out = [recs[i].as_dict() for i in range(k)]
        if outputs:
            models, preds = models[:k], preds[:k]
            if self.args.real_data:
                preds = preds.real.copy()
        return (out, models, preds) if check else (out, models, preds, rc)

    # -- the No-U-turn sampler on a seeded chain (hmcmt_chain_nuts_sample, hmcmt_chain_nuts_run) ----
    def chain_nuts_sample(self, max_depth, outputs=True):
        """One NUTS sample of a seeded chain: the tree doubles up to max_depth times.  Returns (record, m, pred): the record is
        chain_step's (at the selected state) with depth, nleaves, stop, dirs, selected and alpha added."""
        rec = NutsRecord()
        m = np.empty(self.nAC) if outputs else None
        pred = np.empty(self.nData, dtype=np.complex128) if outputs else None
        self._check(self.lib.hmcmt_chain_nuts_sample(self.h, int(max_depth), C.byref(rec), _dp(m) if outputs else None,
                                                     _dp(pred) if outputs else None))
        if outputs and self.args.real_data:
            pred = pred.real.copy()
        return rec.as_dict(), m, pred

    def chain_nuts_run(self, nsamples, max_depth, outputs=True, check=True):
        """nsamples NUTS samples in one call, in chain_run's conventions."""
        nsamples = int(nsamples)
        rows = max(nsamples, 0)                              # (a negative nsamples is the library's to refuse)
        recs = (NutsRecord * max(rows, 1))()
        models = np.empty((rows, self.nAC)) if outputs else None
        preds = np.empty((rows, self.nData), dtype=np.complex128) if outputs else None
        done = C.c_int64()
        rc = self.lib.hmcmt_chain_nuts_run(self.h, nsamples, int(max_depth), recs, _dp(models) if outputs else None,
                                           _dp(preds) if outputs else None, C.byref(done))
        if check:
            self._check(rc)
        k = int(done.value)
        out = [recs[i].as_dict() for i in range(k)]
        if outputs:
            models, preds = models[:k], preds[:k]
            if self.args.real_data:
                preds = preds.real.copy()
        return (out, models, preds) if check else (out, models, preds, rc)

    def debug_nuts_leaf(self, n, p, rho_s, x=None, inv_m=None, backward=False, first=False, ck_write=None, ck_due=(), merged=None):
        """k_nuts_leaf + k_nuts_final on device vectors given as pointers (ints): hmcmt_debug_nuts_leaf.  ck_write: (p, x, rho_s) to
        store; ck_due: a list of such triples to check; merged: dict(rho=, rho_next=, p_other=, x_other=None, other_backward=).
        Returns the NUTS_SUMS sums."""
        a = DebugNutsArgs()
        a.n, a.backward, a.first, a.ndue = int(n), int(bool(backward)), int(bool(first)), len(ck_due)
        a.p, a.x, a.inv_m, a.rho_s = p, x, inv_m, rho_s
        if ck_write is not None:
            for v in range(3):
                a.ck_write[v] = ck_write[v]
        for c, trip in enumerate(ck_due[:NUTS_CK_MAX]):
            for v in range(3):
                a.ck_due[c][v] = trip[v]
        if merged is not None:
            a.merged = 1
            a.rho, a.rho_next, a.p_other, a.x_other = merged["rho"], merged["rho_next"], merged["p_other"], merged.get("x_other")
            a.other_backward = int(bool(merged.get("other_backward", False)))
        sums = np.zeros(NUTS_SUMS)
        self._check(self.lib.hmcmt_debug_nuts_leaf(self.h, C.byref(a), _dp(sums)))
        return sums

    def debug_nuts_iters(self, reset=False):
        """{after_change: (iterations, solves), other: (iterations, solves)} of the NUTS leaves since the last reset (measurement)."""
        o = np.zeros(4, dtype=np.int64)
        self._check(self.lib.hmcmt_debug_nuts_iters(self.h, o.ctypes.data_as(c_int64_p), int(bool(reset))))
        return {"after_change": (int(o[0]), int(o[1])), "other": (int(o[2]), int(o[3]))}

    # -- marginal posteriors from the chain's commit (hmcmt_chain_hist_*, hmcmt_chain_data_moments*) --
    def chain_hist_begin(self, targets, nbins, lo, hi):
        """Starts per-cell histograms of ln sigma over [lo, hi) in nbins bins (values outside are clamped into the edge bins) for the
        active-cell indices `targets` (0-based, repeats allowed): every later commit behind the burn-in counts.  Replaces a
        histogram that is running."""
        t = np.ascontiguousarray(targets, dtype=np.int64).reshape(-1)
        self._check(self.lib.hmcmt_chain_hist_begin(self.h, len(t), t.ctypes.data_as(c_int64_p), int(nbins), float(lo), float(hi)))
        self._hist_shape = (len(t), int(nbins))

    def chain_hist(self):
        """(count, counts[ntarget, nbins] uint32): commits in the histogram and its rows."""
        n = C.c_int64()
        counts = np.empty(self._hist_shape_or_raise(), dtype=np.uint32)
        self._check(self.lib.hmcmt_chain_hist(self.h, C.byref(n), counts.ctypes.data, 0))
        return int(n.value), counts

    def chain_hist_device(self, d_counts):
        """The same into a device pointer (int) to ntarget * nbins uint32, target-major; returns count."""
        n = C.c_int64()
        self._check(self.lib.hmcmt_chain_hist(self.h, C.byref(n), d_counts, 1))
        return int(n.value)

    def chain_quantiles(self, q, d_out=None):
        """Quantiles q (each in [0, 1]) of every target's histogram, linear inside the bin, computed on the device: [nq, ntarget] in
        ln sigma -- or into the device pointer d_out (int), returning None."""
        q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
        if d_out is not None:
            self._check(self.lib.hmcmt_chain_hist_quantiles(self.h, len(q), _dp(q), d_out, 1))
            return None
        out = np.empty((len(q), self._hist_shape_or_raise()[0]))
        self._check(self.lib.hmcmt_chain_hist_quantiles(self.h, len(q), _dp(q), out.ctypes.data, 0))
        return out

    def _hist_shape_or_raise(self):
        # (the library knows whether a histogram is running: a zero-length call gets its error, and its message)
        n = C.c_int64()
        self._check(self.lib.hmcmt_chain_hist(self.h, C.byref(n), None, 0))
        return self._hist_shape

    def chain_data_moments_begin(self):
        """Starts the Welford moments of the chain's predicted data: every later commit behind the burn-in counts."""
        self._check(self.lib.hmcmt_chain_data_moments_begin(self.h))

    def chain_data_moments(self, raw=False):
        """(count, mean[nData], m2[nData]) of the predicted data at the counted commits: complex mean, and m2 = re + i im with the sums
        of squared deviations of the real and the imaginary parts (real arrays for a real data type, whose imaginary slots hold
        exact zeros).  raw=True: the library's own 2 nData doubles each, re and im interleaved."""
        n = C.c_int64()
        mean, m2 = np.empty(2 * self.nData), np.empty(2 * self.nData)
        self._check(self.lib.hmcmt_chain_data_moments(self.h, C.byref(n), mean.ctypes.data, m2.ctypes.data, 0))
        if raw:
            return int(n.value), mean, m2
        if self.args.real_data:
            return int(n.value), mean[0::2].copy(), m2[0::2].copy()
        return int(n.value), mean.view(np.complex128), m2.view(np.complex128)

    def _cell_list(self, arg, what):
        """(n, list, rows) of a begin's list of active cells: what the library takes (0, None for arg = None: every active cell) and
        the rows the accumulator gets; `what`: the error of an empty list."""
        if arg is None:
            return 0, None, self.nAC
        t = np.ascontiguousarray(arg, dtype=np.int64).reshape(-1)
        if len(t) == 0:
            raise ValueError(f"{what} (None means every active cell)")
        return len(t), t.ctypes.data_as(c_int64_p), len(t)

    def _chain_timing(self, fn, enable, names):
        """{name: (ms, launches)} of the two classes of a measurement-only timer of the commit (include/hmcmt_debug.h)."""
        ms, n = np.zeros(2), np.zeros(2, dtype=np.int64)
        self._check(fn(self.h, -1 if enable is None else int(bool(enable)), _dp(ms), n.ctypes.data_as(c_int64_p)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    # -- effective sample size from the chain's commit (hmcmt_chain_acov_*, hmcmt_chain_ess) --
    def chain_acov_begin(self, targets=None, maxlag=63):
        """Starts per-cell lagged autocovariances of ln sigma for the lags 0 .. maxlag (1 .. 1023) of the active-cell indices `targets`
        (0-based, repeats allowed; None: every active cell): every later commit behind the burn-in counts.  Replaces an accumulator
        that is running."""
        n, t, nt = self._cell_list(targets, "chain_acov_begin: no target")
        self._check(self.lib.hmcmt_chain_acov_begin(self.h, n, t, int(maxlag)))
        self._acov_shape = (int(maxlag) + 1, nt)

    def chain_acov_count(self):
        """Commits in the accumulator (the read-outs need at least one)."""
        n = C.c_int64()
        self._check(self.lib.hmcmt_chain_acov(self.h, C.byref(n), None, None, 0))
        return int(n.value)

    def _acov_shape_or_raise(self):
        self.chain_acov_count()
        return self._acov_shape

    def chain_acov_timing(self, enable=None):
        """Measurement only (hmcmt_debug_chain_acov_time): enable = True / False switches HIP-event pairs round every k_chain_acov
        launch on / off and zeroes the sums, None only reads.  Returns the sums up to the call: {"filling": (ms, launches), "steady": (ms, launches)}: the
        commits with count < maxlag, where some lag still fills its H_k, and those behind them."""
        return self._chain_timing(self.lib.hmcmt_debug_chain_acov_time, enable, ("filling", "steady"))

    def chain_acov(self):
        """(count, mean[ntarget], acov[maxlag + 1, ntarget]): commits in the accumulator, the targets' means and the biased
        autocovariance estimates c_k, lag-major (c_k = 0 for k >= count)."""
        n = C.c_int64()
        shape = self._acov_shape_or_raise()
        mean, acov = np.empty(shape[1]), np.empty(shape)
        self._check(self.lib.hmcmt_chain_acov(self.h, C.byref(n), mean.ctypes.data, acov.ctypes.data, 0))
        return int(n.value), mean, acov

    def chain_acov_device(self, d_mean=None, d_acov=None):
        """The same into device pointers (int; each may be None) to ntarget and (maxlag + 1) * ntarget doubles; returns count."""
        n = C.c_int64()
        self._check(self.lib.hmcmt_chain_acov(self.h, C.byref(n), d_mean, d_acov, 1))
        return int(n.value)

    def chain_ess(self, d_tau=None, d_ess=None, d_window=None):
        """(tau[ntarget], ess[ntarget], window[ntarget] int32) by Geyer's initial positive sequence, computed on the device
        (include/hmcmt.h) -- or, with any of the device pointers (int) given, into those, returning None."""
        if d_tau is not None or d_ess is not None or d_window is not None:
            self._check(self.lib.hmcmt_chain_ess(self.h, d_tau, d_ess, d_window, 1))
            return None
        nt = self._acov_shape_or_raise()[1]
        tau, ess, window = np.empty(nt), np.empty(nt), np.empty(nt, dtype=np.int32)
        self._check(self.lib.hmcmt_chain_ess(self.h, tau.ctypes.data, ess.ctypes.data, window.ctypes.data, 0))
        return tau, ess, window

    # -- posterior covariance and correlation from the chain's commit (hmcmt_chain_cov_*, hmcmt_chain_corr) --
    def chain_cov_begin(self, rows=None, batch=0):
        """Starts the cross moments of ln sigma between the active-cell indices `rows` (0-based, repeats allowed; None: every active
        cell, the full matrix) and every active cell: every later commit behind the burn-in counts.  `batch` commits (1 .. 16, 0: the
        default 8) are folded into the sums by one kernel; the results do not depend on it.  Replaces an accumulator that is running."""
        n, r, nr = self._cell_list(rows, "chain_cov_begin: no row")
        self._check(self.lib.hmcmt_chain_cov_begin(self.h, n, r, int(batch)))
        self._cov_shape = (nr, self.nAC)

    def chain_cov_count(self):
        """Commits in the accumulator (the read-outs need at least one)."""
        n = C.c_int64()
        self._check(self.lib.hmcmt_chain_cov(self.h, C.byref(n), None, None, None, 0))
        return int(n.value)

    def chain_cov_timing(self, enable=None):
        """Measurement only (hmcmt_debug_chain_cov_time): enable = True / False switches HIP-event pairs round every commit and flush
        kernel of the accumulator on / off and zeroes the sums, None only reads.  Returns the sums up to the call:
        {"commit": (ms, launches), "flush": (ms, launches)}."""
        return self._chain_timing(self.lib.hmcmt_debug_chain_cov_time, enable, ("commit", "flush"))

    def chain_cov(self):
        """(count, mean[nAC], var[nAC], cov[nrow, nAC]): commits in the accumulator, the cells' means and biased variances, and the
        biased covariance of every row's cell with every cell (include/hmcmt.h)."""
        n = C.c_int64()
        self.chain_cov_count()
        shape = self._cov_shape
        mean, var, cov = np.empty(shape[1]), np.empty(shape[1]), np.empty(shape)
        self._check(self.lib.hmcmt_chain_cov(self.h, C.byref(n), mean.ctypes.data, var.ctypes.data, cov.ctypes.data, 0))
        return int(n.value), mean, var, cov

    # -- posterior principal components by a row sketch (hmcmt_chain_sketch_*, hmcmt_chain_pca) --
    def chain_sketch_begin(self, ell=32, pivot=None):
        """Starts the frequent-directions sketch of the committed models: 2 <= ell <= 64 directions kept through every shrink,
        2 ell rows of nAC doubles on the device.  pivot[nAC] or None (the model of the first counted commit); sketches of several
        chains merge only under one given pivot (include/hmcmt.h has the algorithm and its guarantee)."""
        pv = None if pivot is None else np.ascontiguousarray(pivot, dtype=np.float64)
        if pv is not None and pv.shape != (self.nAC,):
            raise ValueError(f"chain_sketch_begin: pivot has shape {pv.shape}, not ({self.nAC},)")
        self._check(self.lib.hmcmt_chain_sketch_begin(self.h, int(ell), None if pv is None else _dp(pv)))
        self._sketch_ell = int(ell)

    def chain_sketch_info(self):
        """hmcmt_sketch_info as a dict: count, ell, fill, shrinks, Delta, pivot_given."""
        info = SketchInfo()
        self._check(self.lib.hmcmt_chain_sketch(self.h, C.byref(info), None, None, None, 0))
        return info.as_dict()

    def chain_sketch(self):
        """The sketch as it stands, a dict: the fields of chain_sketch_info, mean[nAC], var[nAC] (biased, the formulas of chain_cov),
        rows[fill, nAC] (unshrunk rows included) and x0, tot, q (chain_sketch_sums).  With A the rows y_t = m_t - x0 of the counted commits: 0 <= A'A - rows'rows <= Delta I."""
        info = self.chain_sketch_info()
        mean, var, rows = np.empty(self.nAC), np.empty(self.nAC), np.empty((info["fill"], self.nAC))
        got = SketchInfo()
        self._check(self.lib.hmcmt_chain_sketch(self.h, C.byref(got), mean.ctypes.data, var.ctypes.data, rows.ctypes.data if rows.size else None, 0))
        out = got.as_dict()
        out.update(mean=mean, var=var, rows=rows)
        out.update(self.chain_sketch_sums())
        return out

    def chain_sketch_sums(self):
        """{x0, tot, q} [nAC] of the running sketch -- the pivot, the sum of y and the sum of y^2 that mean and var are made of and that
        pcaFromSketch and mergeSketches need (hmcmt_debug_chain_sketch_sums)."""
        x0, tot, q = np.empty(self.nAC), np.empty(self.nAC), np.empty(self.nAC)
        self._check(self.lib.hmcmt_debug_chain_sketch_sums(self.h, x0.ctypes.data, tot.ctypes.data, q.ctypes.data, 0))
        return {"x0": x0, "tot": tot, "q": q}

    def chain_sketch_device(self, d_mean=None, d_var=None, d_rows=None):
        """As chain_sketch into device pointers (ints; each may be None; d_rows has room for 2 ell rows); returns the info dict."""
        info = SketchInfo()
        self._check(self.lib.hmcmt_chain_sketch(self.h, C.byref(info), d_mean, d_var, d_rows, 1))
        return info.as_dict()

    def chain_pca(self, rank=8, d_lambda=None, d_U=None):
        """(lam[kept], U[kept, nAC], err): the leading eigenpairs of the sketch's centred covariance estimate, descending, and the
        bound err = Delta / N within which every lam[k] lies of the exact k-th eigenvalue.  With d_lambda / d_U (device pointers as
        ints, room for rank rows) the results stay on the device and (kept, err) is returned."""
        kept, err = C.c_int32(), C.c_double()
        if d_lambda is not None or d_U is not None:
            self._check(self.lib.hmcmt_chain_pca(self.h, int(rank), C.byref(kept), d_lambda, d_U, C.byref(err), 1))
            return int(kept.value), float(err.value)
        rank = int(rank)
        lam, U = np.empty(max(rank, 1)), np.empty((max(rank, 1), self.nAC))
        self._check(self.lib.hmcmt_chain_pca(self.h, rank, C.byref(kept), lam.ctypes.data, U.ctypes.data, C.byref(err), 0))
        k = int(kept.value)
        return lam[:k].copy(), U[:k].copy(), float(err.value)

    def chain_sketch_timing(self, enable=None):
        """Measurement only (hmcmt_debug_chain_sketch_time): as chain_cov_timing, classes "commit" and "shrink" (the Gram and the
        shrink kernel: two launches per shrink), plus "host_ms", the host milliseconds of the shrinks' eigenproblems."""
        host = C.c_double()
        ms, launches = np.zeros(2), np.zeros(2, dtype=np.int64)
        self._check(self.lib.hmcmt_debug_chain_sketch_time(self.h, -1 if enable is None else int(bool(enable)), _dp(ms),
                                                           launches.ctypes.data_as(c_int64_p), C.byref(host)))
        out = {k: {"ms": float(ms[i]), "launches": int(launches[i])} for i, k in enumerate(("commit", "shrink"))}
        out["host_ms"] = float(host.value)
        return out

    def debug_chain_sketch(self, rows, ell, pivot=None, max_shrinks=None):
        """Test hook (hmcmt_debug_chain_sketch): rows [n, nAC] through the chain's commit and shrink launches without a chain.  Returns
        a dict: the info fields, x0, tot, q [nAC], rows [fill, nAC] and, per shrink, K [2 ell, 2 ell] and T [ell, 2 ell]."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.nAC:
            raise ValueError(f"debug_chain_sketch: rows has shape {rows.shape}, not (n, {self.nAC})")
        n, ell = rows.shape[0], int(ell)
        pv = None if pivot is None else np.ascontiguousarray(pivot, dtype=np.float64)
        ns = max(0, (n - ell) // ell) if max_shrinks is None else int(max_shrinks)
        info = SketchInfo()
        x0, tot, q, B = np.empty(self.nAC), np.empty(self.nAC), np.empty(self.nAC), np.zeros((2 * max(ell, 1), self.nAC))
        K, T = np.zeros((max(ns, 1), 2 * ell, 2 * ell)), np.zeros((max(ns, 1), ell, 2 * ell))
        self._check(self.lib.hmcmt_debug_chain_sketch(self.h, ell, n, _dp(rows), None if pv is None else _dp(pv), C.byref(info),
                                                      x0.ctypes.data, tot.ctypes.data, q.ctypes.data, B.ctypes.data, ns, K.ctypes.data, T.ctypes.data))
        out = info.as_dict()
        got = min(ns, out["shrinks"])
        out.update(x0=x0, tot=tot, q=q, rows=B[:out["fill"]].copy(), K=K[:got], T=T[:got])
        return out

    def chain_cov_device(self, d_mean=None, d_var=None, d_cov=None):
        """The same into device pointers (int; each may be None) to nAC, nAC and nrow * nAC doubles; returns count."""
        n = C.c_int64()
        self._check(self.lib.hmcmt_chain_cov(self.h, C.byref(n), d_mean, d_var, d_cov, 1))
        return int(n.value)

    def chain_corr(self, d_corr=None):
        """corr[nrow, nAC] = cov / sqrt(var_row var_cell) clamped into [-1, 1], 0 where a variance is not positive, computed on the
        device -- or, with the device pointer (int) given, into that, returning None."""
        if d_corr is not None:
            self._check(self.lib.hmcmt_chain_corr(self.h, d_corr, 1))
            return None
        self.chain_cov_count()
        corr = np.empty(self._cov_shape)
        self._check(self.lib.hmcmt_chain_corr(self.h, corr.ctypes.data, 0))
        return corr

    # -- step size and diagonal mass between two steps, and their warm-up (hmcmt_chain_set_*, hmcmt_chain_adapt_*) --
    def chain_set_dt(self, dt):
        """Replaces the chain's step size between two steps; everything the chain holds stays valid.  Refused while a warm-up is active."""
        self._check(self.lib.hmcmt_chain_set_dt(self.h, float(dt)))

    def chain_set_mass_diag(self, invM):
        """Replaces the diagonal of M^-1 (every entry finite and > 0) without ending the chain.  A momentum drawn before the call is
        dropped: draw a new one before the next step."""
        self._check(self.lib.hmcmt_chain_set_mass_diag(self.h, _dp(self._model(invM))))

    def chain_mass_diag(self, d_invM=None):
        """The diagonal of M^-1 in force: invM[nAC] -- or into the device pointer d_invM (int), returning None."""
        if d_invM is not None:
            self._check(self.lib.hmcmt_chain_mass_diag(self.h, d_invM, 1))
            return None
        invM = np.empty(self.nAC)
        self._check(self.lib.hmcmt_chain_mass_diag(self.h, invM.ctypes.data, 0))
        return invM

    def chain_adapt_begin(self, nwarmup, **options):
        """Starts a warm-up over the next `nwarmup` steps: dual averaging of dt towards the acceptance `delta` and, with adapt_mass
        (the default), Stan's windowed estimate of the diagonal of M^-1 from the chain's own samples.  options: the fields of
        hmcmt_adapt_options (include/hmcmt.h) -- adapt_mass, init_buffer, term_buffer, base_window, delta, gamma, t0, kappa,
        dt_min, dt_max; what is not given keeps the library's default."""
        unknown = sorted(set(options) - set(ADAPT_OPTION_KEYS))
        if unknown:
            raise ValueError(f"chain_adapt_begin: unknown option(s) {unknown}; known: {list(ADAPT_OPTION_KEYS)}")
        o = AdaptOptions()
        self.lib.hmcmt_default_adapt_options(C.byref(o))
        o.nwarmup = int(nwarmup)
        for k, v in options.items():
            setattr(o, k, type(getattr(o, k))(v))
        self._check(self.lib.hmcmt_chain_adapt_begin(self.h, C.byref(o)))

    def chain_adapt_info(self):
        """Where the warm-up stands (hmcmt_adapt_info as a dict): step, nwarmup, window_count, next_window_end, active, windows_done,
        dt (what the next step uses), dt_bar, mu, s_bar, alpha_last, alpha_sum."""
        info = AdaptInfo()
        self._check(self.lib.hmcmt_chain_adapt_info(self.h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in AdaptInfo._fields_}

    def chain_adapt_end(self):
        """Stops a warm-up now: dt = exp(x_bar) as at its regular end."""
        self._check(self.lib.hmcmt_chain_adapt_end(self.h))

    # -- the low-rank mass of a live chain: the warm-up's upgrade, the between-steps setter, the read-out --
    def chain_adapt_lowrank(self, **options):
        """Upgrades the warm-up just begun with adapt_mass (chain_adapt_begin, no step counted yet): every window end also estimates
        the directions U and factors lambda of the low-rank mass from the window's draws and gradients (hmcmt_chain_adapt_lowrank).
        options: rank (8), max_samples (64), cutoff (2), gamma (1e-5)."""
        o = adapt_lowrank_options(options)
        self._check(self.lib.hmcmt_chain_adapt_lowrank(self.h, C.byref(o)))
        self._adapt_lowrank_max = int(o.max_samples)

    def chain_adapt_lowrank_info(self):
        """The last closed window of the upgraded warm-up (hmcmt_adapt_lowrank_info as a dict): windows, stored, skipped, dims, rank,
        fallback, stride, theta_min, theta_max, defect, host_ms."""
        info = AdaptLowrankInfo()
        self._check(self.lib.hmcmt_chain_adapt_lowrank_info(self.h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in AdaptLowrankInfo._fields_}

    def chain_set_mass_lowrank(self, invM, U=None, lam=None):
        """hmcmt_chain_set_mass_lowrank: the low-rank mass between two steps of a live chain (set_mass_lowrank's arguments; the chain
        and its accumulators go on, a momentum already drawn is dropped).  U None or of rank 0 with invM: back to the plain diagonal."""
        if U is None or np.asarray(U).size == 0:
            if invM is None:
                raise ValueError("chain_set_mass_lowrank: rank 0 needs invM")
            self._check(self.lib.hmcmt_chain_set_mass_lowrank(self.h, _dp(self._model(invM)), 0, None, None))
            return
        invM, U, lam = lowrank_mass_arrays(self.nAC, invM, U, lam)
        self._check(self.lib.hmcmt_chain_set_mass_lowrank(self.h, None if invM is None else _dp(invM), int(U.shape[0]), _dp(U), _dp(lam)))

    def chain_mass_lowrank(self):
        """The mass in force (hmcmt_chain_mass_lowrank): (invM [nAC], U [rank, nAC], lam [rank]); rank 0 under the diagonal mass."""
        rank = C.c_int32(0)
        invM, U, lam = np.empty(self.nAC), np.empty((HMCMT_MASS_RANK_MAX, self.nAC)), np.empty(HMCMT_MASS_RANK_MAX)
        self._check(self.lib.hmcmt_chain_mass_lowrank(self.h, C.byref(rank), invM.ctypes.data, U.ctypes.data, lam.ctypes.data, 0))
        r = int(rank.value)
        return invM, U[:r].copy(), lam[:r].copy()

    def debug_adapt_lowrank(self, X, G, invM, B=None):
        """Test hook (hmcmt_debug_adapt_lowrank): K = W W' of the rows X, G [n, nAC] under invM, and with B [2n, r] also U = B' W with
        the sign convention -- the window end's kernels without a chain.  Returns (K, U or None)."""
        X, G = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(G, dtype=np.float64)
        n = X.shape[0]
        if X.ndim != 2 or X.shape != G.shape or X.shape[1] != self.nAC:
            raise ValueError(f"X and G must be [n, nAC = {self.nAC}]; got {X.shape}, {G.shape}")
        K = np.empty((2 * n, 2 * n))
        U, r = None, 0
        if B is not None:
            B = np.ascontiguousarray(B, dtype=np.float64)
            if B.ndim != 2 or B.shape[0] != 2 * n:
                raise ValueError(f"B must be [2n = {2 * n}, r]; got {B.shape}")
            r = B.shape[1]
            U = np.empty((r, self.nAC))
        self._check(self.lib.hmcmt_debug_adapt_lowrank(self.h, n, _dp(X), _dp(G), _dp(self._model(invM)), _dp(K), None if B is None else _dp(B),
                                                       r, None if U is None else _dp(U)))
        return K, U

    def debug_adapt_lowrank_time(self):
        """Measurement (hmcmt_debug_adapt_lowrank_time): the last window end's dict(gram_ms, lift_ms, wait_ms, check_ms)."""
        out = np.zeros(4)
        self._check(self.lib.hmcmt_debug_adapt_lowrank_time(self.h, _dp(out)))
        return dict(zip(("gram_ms", "lift_ms", "wait_ms", "check_ms"), (float(v) for v in out)))

    def debug_adapt_lowrank_rows(self):
        """Test hook (hmcmt_debug_adapt_lowrank_rows): the open window's stored pairs (X [n, nAC], G [n, nAC])."""
        cap = getattr(self, "_adapt_lowrank_max", ADAPT_LOWRANK_NMAX)
        n = C.c_int32(0)
        X, G = np.empty((cap, self.nAC)), np.empty((cap, self.nAC))
        self._check(self.lib.hmcmt_debug_adapt_lowrank_rows(self.h, C.byref(n), _dp(X), _dp(G)))
        return X[:n.value].copy(), G[:n.value].copy()

    # -- instrumentation ----------------------------------------------------------------------
    def profile(self, enable=True, every=1):
        """enable: True (all categories), False, or an iterable of category names to time;
        every: bracket the kernels of every n-th evaluation only."""
        self._check(self.lib.hmcmt_profile_every(self.h, int(every)))
        if enable is True:
            mask = (1 << HMCMT_NCAT) - 1
        elif not enable:
            mask = 0
        else:
            mask = sum(1 << CATEGORIES.index(c) for c in enable)
        self._check(self.lib.hmcmt_profile(self.h, mask))

    def profile_read(self):
        ms = np.zeros(HMCMT_NCAT)
        n = np.zeros(HMCMT_NCAT, dtype=np.int64)
        self._check(self.lib.hmcmt_profile_read(self.h, _dp(ms), n.ctypes.data_as(c_int64_p)))
        return {c: (float(ms[i]), int(n[i])) for i, c in enumerate(CATEGORIES)}

    def profile_overhead_us(self):
        us = C.c_double()
        self._check(self.lib.hmcmt_profile_overhead(self.h, C.byref(us)))
        return us.value

    def profile_counters(self):
        """{active_iter_systems, start_systems, evaluations, solves, solves_two_sweeps, serial_iterations, persistent_solves}
        of the sampled evaluations (hmcmt_profile_counters): serial_iterations = sum over the sampled solves of the slowest
        system's iterations + 1 (the preconditioner application in front of the first one)."""
        o = np.zeros(7, dtype=np.int64)
        self._check(self.lib.hmcmt_profile_counters(self.h, o.ctypes.data_as(c_int64_p)))
        return dict(zip(("active_iter_systems", "start_systems", "evaluations", "solves", "solves_two_sweeps", "serial_iterations",
                         "persistent_solves"), (int(x) for x in o)))

    def _vec(self, a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        if a.size != self.S * self.NZP * self.NYP:
            raise ValueError("vector must be in the padded nodal layout [S][NZP][NYP]")
        return a

    def debug_fdm_fwd(self, T):
        T = self._vec(T)
        out = np.empty((2,) + T.shape, dtype=np.complex128)
        self._check(self.lib.hmcmt_debug_fdm_fwd(self.h, _dp(T), _dp(out)))
        return out[0], out[1]

    def debug_back_post(self, Yv, R):
        Yv, R = self._vec(Yv), self._vec(R)
        out = np.empty((2,) + Yv.shape, dtype=np.complex128)
        sums = np.zeros(6)
        self._check(self.lib.hmcmt_debug_back_post(self.h, _dp(Yv), _dp(R), _dp(out), _dp(sums)))
        return out[0], out[1], sums

    def debug_transform(self, which, A):
        A = self._vec(A)
        Cc = np.empty_like(A)
        self._check(self.lib.hmcmt_debug_transform(self.h, which, _dp(A), _dp(Cc)))
        return Cc

    def debug_flags(self, freeze_boundary=False, no_boundary_terms=False, fail_placement=False, on="next", group=0):
        """Test hook (include/hmcmt_debug.h): hold the Dirichlet values at the previous evaluation's / leave dBC^T w out of the gradient /
        (one-shot) let the first system group -- `group`: the group of that index, xcd x slots_per_xcd + slot; fail_placement="all": EVERY
        group -- of the next persistent launch fail its placement check (on="adjoint": of the next adjoint launch; forward launches pass it by)."""
        if on not in ("next", "adjoint") or not 0 <= int(group) < 256:
            raise ValueError(f"debug_flags: on={on!r} (\"next\" or \"adjoint\"), group={group!r} (0 .. 255)")
        self._cache = None
        place = 8 if fail_placement == "all" else (4 | int(group) << 8 if fail_placement else 0)
        if place and on == "adjoint":
            place |= 16
        self._check(self.lib.hmcmt_debug_flags(self.h, (1 if freeze_boundary else 0) | (2 if no_boundary_terms else 0) | place))

    def debug_spmv(self, p):
        p = self._vec(p)
        q = np.empty_like(p)
        self._check(self.lib.hmcmt_debug_spmv(self.h, _dp(p), _dp(q)))
        return q

    def debug_precond(self, r):
        r = self._vec(r)
        z = np.empty_like(r)
        self._check(self.lib.hmcmt_debug_precond(self.h, _dp(r), _dp(z)))
        return z

    EXTRAP_POINTS = 6     # csrc/hmcmt_items.h: EXT_NP, the fields of the initial-guess extrapolation (the field ring has one slot less, the model ring one more)

    def debug_extrap(self, adjoint=False):
        """The extrapolation state of the forward (adjoint) solve as the last evaluation left it (hmcmt_debug_extrap): weights of
        x_k, x_{k-1}, ..., the repeat flag, the models in the history and the heads of the two rings."""
        out = np.empty(10)
        self._check(self.lib.hmcmt_debug_extrap(self.h, int(adjoint), _dp(out)))
        return {"weights": out[:6].copy(), "keep": int(out[6]), "count": int(out[7]), "head": int(out[8]), "model_head": int(out[9])}

    def debug_guess_capture(self, on=True):
        """Switches the capture of the solves' initial guesses on / off (hmcmt_debug_guess_capture)."""
        self._check(self.lib.hmcmt_debug_guess_capture(self.h, int(bool(on))))

    def debug_guess(self, adjoint=False):
        """The initial guess the last evaluation's forward (adjoint) solve started from: complex (S, NZP, NYP), the padded layout of
        debug_spmv; interior nodes [:, 1:nz, 1:ny] only (hmcmt_debug_guess)."""
        out = np.empty(self.S * self.NZP * self.NYP, dtype=np.complex128)
        self._check(self.lib.hmcmt_debug_guess(self.h, int(adjoint), _dp(out)))
        return out.reshape(self.S, self.NZP, self.NYP)

    def guard(self):
        """Production guard of the stopping rule (hmcmt_guard): true residuals formed every HMCMT_GUARD_EVERY-th evaluation."""
        out = (C.c_double * 4)()
        self._check(self.lib.hmcmt_guard(self.h, out))
        return {"checks": int(out[0]), "worst_true_res": float(out[1]), "last_true_res": float(out[2]), "trips": int(out[3])}

    def persist_info(self):
        """The persistent solve kernel and this context (kernels_persist.h): shape, whether it is enabled, how many solves it ran."""
        out = (C.c_int64 * 16)()
        self._check(self.lib.hmcmt_persist_info(self.h, out, 16))
        return dict(zip(("threads_half", "workgroups_per_system", "slots_per_xcd", "enabled", "solves", "placement_fallbacks", "usable_now", "slab_modes",
                         "column_parts", "timeouts", "cu_share_index", "cu_share_count", "strips", "why_off",
                         "fallback_kind", "fallback_stalled"), (int(x) for x in out)))

    def persist_width(self):
        """Row width (padded nodes) of the width-specialised persistent kernel this context launches; 0: the generic kernel."""
        w = C.c_int32(0)
        self._check(self.lib.hmcmt_persist_width(self.h, C.byref(w)))
        return int(w.value)

    def persist_order(self, kind=0):
        """(order, rebalanced): the order in which the persistent kernel's queues take the systems of a forward (0) / adjoint (1)
        solve -- position queue + queues * round -> system -- and how often the context has re-balanced it (hmcmt_persist_order)."""
        order = (C.c_int32 * self.S)()
        n = C.c_int64(0)
        self._check(self.lib.hmcmt_persist_order(self.h, int(kind), order, C.byref(n)))
        return np.array(list(order)), int(n.value)

    def debug_hog(self, nblocks, ms):
        """Test hook: nblocks workgroups holding a CU's LDS each for ms milliseconds on a stream of their own (returns once they are resident)."""
        self._check(self.lib.hmcmt_debug_hog(self.h, int(nblocks), int(ms)))

    def debug_persist_precond(self, r, sweeps=1):
        """z = P^-1 r by the persistent solve kernel's preconditioner (kernels_persist.h)."""
        r = self._vec(r)
        z = np.empty_like(r)
        self._check(self.lib.hmcmt_debug_persist_precond(self.h, int(sweeps), _dp(r), _dp(z)))
        return z

    def close(self):
        if getattr(self, "h", None):
            self.lib.hmcmt_destroy(self.h)
            self.h = None
            HipContext.live -= 1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
