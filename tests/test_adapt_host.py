"""The chain's warm-up adaptation without a GPU: the item functions of the dual averaging, the window schedule and the mass of a
window on the host (tests/emul/emul_adapt.cpp) against the longdouble reference tests/adapt_ref.py, the layouts of the two structs
in C, Python and Julia, the Julia bindings' argument counts, and the sampler's errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from hmcmt2d_amd import sampler
from hmcmt2d_amd import lib as L
from hmcmt2d_amd.structs import HMCPrior
from tests.conftest import ROOT
from tests import adapt_ref as A
from tests import chain_ref as R
from tests.emul import emul_adapt_py as E
from tests.helpers import make_problem

EPS = np.finfo(float).eps

# (nwarmup, init, term, base) -> window ends as steps completed, samples per window (None: not listed)
SCHEDULES = [((1000, 75, 50, 25), [100, 150, 250, 450, 950], [25, 50, 100, 200, 500]),
             ((200, 75, 50, 25), [100, 150], None),
             ((150, 75, 50, 25), [100], None),
             ((20, 3, 2, 5), [8, 18], None),
             ((16, 2, 2, 3), [5, 14], None),
             ((14, 2, 2, 3), [5, 12], [3, 7]),
             ((12, 2, 2, 3), [5, 10], None),
             ((9, 2, 2, 3), [5, 7], [3, 2]),
             ((8, 2, 2, 3), [5, 6], [3, 1]),
             ((7, 2, 2, 3), [5], None)]


@pytest.mark.parametrize("args,ends,counts", SCHEDULES)
def test_window_ends_of_the_item_function_and_of_the_reference(args, ends, counts):
    assert E.window_ends(*args) == ends
    assert A.window_ends(*args) == ends
    if counts is not None:
        assert A.window_counts(*args) == counts


def test_a_window_of_one_sample_updates_nothing_in_the_reference():
    """nwarmup 8, buffers 2 / 2, base 3: the second window closes with n = 1 -- no mass update, no restart of the dual averaging."""
    w = A.Warmup(0.01, 8, True, 2, 2, 3)
    rng = np.random.default_rng(0)
    for c in range(8):
        w.step(-0.3, rng.standard_normal(4))
        if c == 4:
            assert len(w.masses) == 1 and w.da.t == 0
    assert w.closed == [(5, 3), (6, 1)] and len(w.masses) == 1 and not w.active
    assert w.da.t == 3                                    # (steps 5, 6, 7 behind the one restart)


def _alphas(kind, n, rng):
    if kind == "zeros":
        return np.zeros(n)
    if kind == "ones":
        return np.ones(n)
    if kind == "uniform":
        return rng.random(n)
    return np.minimum(1.0, np.exp(rng.normal(0.0, 2.0, n)))


@pytest.mark.parametrize("kind", ["zeros", "ones", "uniform", "lognormal"])
def test_dual_averaging_item_against_the_longdouble_reference(kind):
    """200 updates from dt = 0.03; x and x_bar within 8 eps (sqrt(t) / gamma + 8) of the longdouble recurrence at every update.
    Reached by the host instantiation (g++ -O2, glibc) at its worst update, as fractions of the bound in x / in x_bar: zeros
    0.361 / 0.309, ones 0.106 / 0.063, uniform 0.182 / 0.231, lognormal 0.107 / 0.062 -- i.e. up to 2.9 eps (sqrt(t) / gamma + 8)."""
    rng = np.random.default_rng({"zeros": 1, "ones": 2, "uniform": 3, "lognormal": 4}[kind])
    alpha = _alphas(kind, 200, rng)
    x, x_bar, dt = E.dual_averaging(alpha, 0.03)
    ref = A.DualAveraging(0.03)
    worst = [0.0, 0.0]
    for i, a in enumerate(alpha):
        ref.update(a)
        b = ref.bound()
        ex, eb = abs(float(A.LD(x[i]) - ref.x)), abs(float(A.LD(x_bar[i]) - ref.x_bar))
        worst = [max(worst[0], ex / b), max(worst[1], eb / b)]
        assert ex <= b and eb <= b, (kind, i, ex, eb, b)
        assert abs(dt[i] - np.exp(x[i])) <= 2 * EPS * dt[i]      # (the C library's exp and numpy's may differ in the last bit)
    print(f"dual averaging {kind}: worst |x - ref| / bound {worst[0]:.3f}, |x_bar - ref| / bound {worst[1]:.3f}")
    # the direction: rejections shrink the step, acceptances grow it
    if kind == "zeros":
        assert x_bar[-1] < np.log(0.03) and np.all(np.diff(x[:20]) < 0)
    if kind == "ones":
        assert x_bar[-1] > np.log(0.03)


def test_dual_averaging_clip_and_other_settings():
    alpha = _alphas("uniform", 50, np.random.default_rng(7))
    x, x_bar, dt = E.dual_averaging(alpha, 0.5, delta=0.65, gamma=0.1, t0=5.0, kappa=0.9, dt_min=0.2, dt_max=0.9)
    ref = A.DualAveraging(0.5, delta=0.65, gamma=0.1, t0=5.0, kappa=0.9)
    for i, a in enumerate(alpha):
        ref.update(a)
        assert abs(float(A.LD(x[i]) - ref.x)) <= ref.bound() and abs(float(A.LD(x_bar[i]) - ref.x_bar)) <= ref.bound()
    assert np.all((dt >= 0.2) & (dt <= 0.9)) and ((dt == 0.2).any() or (dt == 0.9).any())
    assert np.allclose(dt, np.clip(np.exp(x), 0.2, 0.9), rtol=2 * EPS, atol=0)
    # both bounds at the start value: the step size stays what it was, bit for bit
    assert np.all(E.dual_averaging(alpha, 0.03, dt_min=0.03, dt_max=0.03)[2] == 0.03)
    # acceptances without end: dt stays finite
    assert np.all(np.isfinite(E.dual_averaging(np.ones(5000), 1.0)[2]))
    assert np.all(E.dual_averaging(np.zeros(5000), 1.0)[2] > 0)


@pytest.mark.parametrize("ncell,nsamp", [(7, 2), (390, 3), (96, 7), (1000, 25)])
def test_mass_of_a_window_against_the_two_pass_reference(ncell, nsamp):
    """Samples like a chain's: values of ln sigma around -4.6 that move by 0.02 per accepted step, rejections repeating a column,
    cell 3 never moving.  The variance within chain_ref.moments_bounds, var * w + f within 4 eps more; the fixed cell gives f exactly."""
    rng = np.random.default_rng(ncell + nsamp)
    cols = [-4.6 + 0.5 * rng.standard_normal(ncell)]
    for s in range(1, nsamp):
        cols.append(cols[-1].copy() if (s % 3 == 2 and nsamp > 2) else cols[-1] + 0.02 * rng.standard_normal(ncell))
    win = np.array(cols).T
    win[3, :] = win[3, 0]
    got = E.window_mass(win)
    mass, n, mean, m2, w, f = A.window_mass(win)
    assert n == nsamp and w == nsamp / (nsamp + 5.0) and f == 1e-3 * 5.0 / (nsamp + 5.0)
    bound = A.mass_bound(mass, mean, m2, n, w)
    err = np.abs(got - np.asarray(mass, dtype=np.float64))
    assert np.all(err <= bound), float((err / bound).max())
    assert got[3] == f and np.all(got >= f) and (got > f).sum() == ncell - 1
    # the bound is the one of the chain's moments, carried through the two further operations
    _, bvar = R.moments_bounds(np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64), n)
    assert np.allclose(bound - 4 * EPS * np.asarray(mass, dtype=np.float64), bvar * (n / (n - 1.0)) * w, rtol=1e-12, atol=0)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
STRUCTS = (("hmcmt_adapt_options", L.AdaptOptions, "HmcmtAdaptOptions"), ("hmcmt_adapt_info", L.AdaptInfo, "HmcmtAdaptInfo"))


def _prototypes():
    text = open(os.path.join(ROOT, "include", "hmcmt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
            for m in re.finditer(r"^\s*extern\s+(?:int|void)\s+(hmcmt_[a-z_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)}


def test_adapt_symbols_are_declared_exported_and_bound():
    so = ctypes.CDLL(L.build_library())
    protos = _prototypes()
    assert set(L.CHAIN_ADAPT_SYMBOLS) <= set(protos) and set(L.CHAIN_ADAPT_SYMBOLS) <= set(L.PRODUCT_SYMBOLS)
    assert sorted(L.CHAIN_ADAPT_SYMBOLS) == sorted(["hmcmt_chain_set_dt", "hmcmt_chain_set_mass_diag", "hmcmt_chain_mass_diag",
                                                    "hmcmt_default_adapt_options", "hmcmt_chain_adapt_begin", "hmcmt_chain_adapt_info",
                                                    "hmcmt_chain_adapt_end"])
    lib = L.load_library()
    for sym in L.CHAIN_ADAPT_SYMBOLS:
        assert hasattr(so, sym), sym
        assert len(getattr(lib, sym).argtypes) == len(protos[sym]), sym
    for name in ("chain_set_dt", "chain_set_mass_diag", "chain_mass_diag", "chain_adapt_begin", "chain_adapt_info", "chain_adapt_end"):
        assert callable(getattr(L.HipContext, name))


def test_default_adapt_options():
    o = L.AdaptOptions()
    L.load_library().hmcmt_default_adapt_options(ctypes.byref(o))
    assert (o.nwarmup, o.adapt_mass, o.init_buffer, o.term_buffer, o.base_window) == (0, 1, 75, 50, 25)
    assert (o.delta, o.gamma, o.t0, o.kappa, o.dt_min, o.dt_max) == (0.8, 0.05, 10.0, 0.75, 0.0, 0.0)
    assert set(L.ADAPT_OPTION_KEYS) == {f for f, _ in L.AdaptOptions._fields_} - {"nwarmup"}


def test_struct_layouts_in_c_python_and_julia(tmp_path):
    lines = []
    for cname, cls, _ in STRUCTS:
        lines.append(f'  printf("%zu\\n", sizeof({cname}));\n')
        lines += [f'  printf("%zu\\n", offsetof({cname}, {f}));\n' for f, _ in cls._fields_]
    src = tmp_path / "adapt.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmcmt.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "adapt"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    ctype = {ctypes.c_int32: "Int32", ctypes.c_int64: "Int64", ctypes.c_double: "Float64"}
    for cname, cls, jname in STRUCTS:
        k = 1 + len(cls._fields_)
        mine, out = out[:k], out[k:]
        assert mine[0] == ctypes.sizeof(cls), cname
        assert mine[1:] == [getattr(cls, f).offset for f, _ in cls._fields_], cname
        body = re.search(r"struct %s\b(.*?)\nend" % jname, jl, flags=re.S).group(1)
        assert re.findall(r"^\s*([A-Za-z_0-9]+)::(\w+)", body, flags=re.M) == [(f, ctype[t]) for f, t in cls._fields_], jname
    assert ctypes.sizeof(L.AdaptOptions) == 72 and ctypes.sizeof(L.AdaptInfo) == 88


JULIA_TYPES = {"hmcmt_chain_set_dt": ["Ptr{Cvoid}", "Float64"],
               "hmcmt_chain_set_mass_diag": ["Ptr{Cvoid}", "Ptr{Float64}"],
               "hmcmt_chain_mass_diag": ["Ptr{Cvoid}", "Ptr{Float64}", "Int32"],
               "hmcmt_chain_adapt_begin": ["Ptr{Cvoid}", "Ref{HmcmtAdaptOptions}"],
               "hmcmt_chain_adapt_info": ["Ptr{Cvoid}", "Ref{HmcmtAdaptInfo}"],
               "hmcmt_chain_adapt_end": ["Ptr{Cvoid}"]}
C_TYPES = {"hmcmt_chain_set_dt": ["hmcmt_ctx*", "double"],
           "hmcmt_chain_set_mass_diag": ["hmcmt_ctx*", "const double*"],
           "hmcmt_chain_mass_diag": ["hmcmt_ctx*", "double*", "int32_t"],
           "hmcmt_chain_adapt_begin": ["hmcmt_ctx*", "const hmcmt_adapt_options*"],
           "hmcmt_chain_adapt_info": ["hmcmt_ctx*", "hmcmt_adapt_info*"],
           "hmcmt_chain_adapt_end": ["hmcmt_ctx*"]}


def test_julia_binds_the_adaptation_with_the_prototypes_arguments():
    jl = open(os.path.join(ROOT, "julia", "HMCMTHip.jl")).read()
    protos = _prototypes()
    for sym, types in JULIA_TYPES.items():
        m = re.search(r"@ccall libhmcmt\.%s\((.*?)\)::Cint" % sym, jl, flags=re.S)
        assert m, f"{sym} is not bound in julia/HMCMTHip.jl with @ccall"
        assert re.findall(r"::\s*([A-Za-z0-9{}]+)", m.group(1)) == types, sym
        assert [" ".join(p.split()[:-1]) for p in protos[sym]] == C_TYPES[sym], sym
        assert len(types) == len(protos[sym])
    for name in ("chainSetDt!", "chainSetMassDiag!", "chainMassDiag", "chainAdaptBegin!", "chainAdaptInfo", "chainAdaptEnd!"):
        assert name in re.search(r"^export (.*?)\n\n", jl, flags=re.S | re.M).group(1), name
    assert re.search(r"function run_chain!\(.*?adapt::Union\{Nothing,NamedTuple\}=nothing\)", jl, flags=re.S)


# ---- the sampler's errors, before any GPU call ----------------------------------------------------------------------------------------
class NoDevice:
    """A context that fails the test when the sampler touches it"""

    def __getattr__(self, name):
        raise AssertionError(f"the sampler called ctx.{name} before it checked its arguments")


def test_sampler_refuses_bad_adapt_arguments_before_any_gpu_call():
    mesh, data, inv, _ = make_problem("tiny")
    n = len(inv.strModel)
    prior = HMCPrior(totalsamples=30, burninsamples=20, dt=0.02, timestep=[1, 2], sigBounds=[1e-4, 1.0])

    def run(p=prior, **kw):
        return sampler.runHMCSampler(mesh, data, inv, p, np.random.default_rng(1), ctx=NoDevice(), **kw)

    with pytest.raises(ValueError, match="device_chain"):
        run(adapt={})
    with pytest.raises(ValueError, match="device_chain"):
        run(invM=np.ones(n))
    with pytest.raises(ValueError, match="burninsamples"):
        run(device_chain=True, adapt={"nwarmup": 21})
    with pytest.raises(ValueError, match="nwarmup"):
        run(device_chain=True, adapt={"nwarmup": 0})
    with pytest.raises(ValueError, match="no key"):
        run(device_chain=True, adapt={"warmup": 10})
    wm = HMCPrior(totalsamples=30, burninsamples=20, dt=0.02, timestep=[1, 2], sigBounds=[1e-4, 1.0], massType="Wm")
    with pytest.raises(ValueError, match="diagonal"):
        run(wm, device_chain=True, adapt={"mass": True})
    with pytest.raises(ValueError, match="diagonal"):
        run(wm, device_chain=True, invM=np.ones(n))


def test_adapt_plan_defaults():
    p = HMCPrior(totalsamples=2000, burninsamples=1000)
    assert sampler.adaptPlan({}, p) == (1000, {"adapt_mass": 1})                      # (Stan's 75 / 50 / 25 fit: the library's defaults)
    assert sampler.adaptPlan({"nwarmup": 100, "delta": 0.65}, p) == \
        (100, {"delta": 0.65, "init_buffer": 15, "term_buffer": 10, "base_window": 75, "adapt_mass": 1})
    assert sampler.adaptPlan({"nwarmup": 19}, p) == (19, {"adapt_mass": 0})          # (below 20: the step size only)
    assert sampler.adaptPlan({"nwarmup": 14, "init_buffer": 2, "term_buffer": 2, "base_window": 3}, p) == \
        (14, {"init_buffer": 2, "term_buffer": 2, "base_window": 3, "adapt_mass": 1})
    assert sampler.adaptPlan({"mass": False}, p) == (1000, {"adapt_mass": 0})
    wm = HMCPrior(totalsamples=2000, burninsamples=1000, massType="Wm")
    assert sampler.adaptPlan({}, wm) == (1000, {"adapt_mass": 0})
