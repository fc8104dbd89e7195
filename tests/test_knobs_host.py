"""The environment reader of the library (hmcmt2d_amd/csrc/hmcmt_knobs.h) held to its parsing rules, without a GPU.

tests/emul/emul_knobs.cpp is a stand-alone program over the header: it prints what read_knobs makes of the environment it is
started in.  Every expected value below is a literal written from the rules of DESIGN.md section 6 (those of the code before
there was one reader), never from the reader itself.
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emul", "emul_knobs.cpp")
HDR = os.path.join(ROOT, "hmcmt2d_amd", "csrc", "hmcmt_knobs.h")
BUILD = os.path.join(HERE, "emul", "_build")

DEFAULTS = {
    "HMCMT_TICKS": "0", "HMCMT_NO_FUSED_START": "0", "HMCMT_NO_SIGMA_ROWS": "0", "HMCMT_NO_COEF_ALL": "0",
    "HMCMT_FWD_STAMPS": "0", "HMCMT_BACK_STAMPS": "0",
    "HMCMT_PERSIST": "1", "HMCMT_PS_START": "1", "HMCMT_PERSIST_BALANCE": "1", "HMCMT_TWIST": "1", "HMCMT_FUSED_BACK": "1",
    "HMCMT_SPEC": "1", "HMCMT_LAZY_DINV": "1", "HMCMT_STREAM_PRIORITY": "1", "HMCMT_PERSIST_WIDTHK": "1", "HMCMT_PERSIST_LOCK": "1",
    "HMCMT_FUSED_FWD": "1",        # 0 off, 1 on, 2 forced
    "HMCMT_SENS_FUSED": "2",       # 0 never, 1 always, 2 automatic
    "HMCMT_XFWD": "-1",            # -1 the size heuristic, 0 off, 1 on
    "HMCMT_PS_SPIN": "4194304", "HMCMT_SWEEPS": "0", "HMCMT_SWEEPS_UP": "12", "HMCMT_SWEEPS_DOWN": "6", "HMCMT_GUARD_EVERY": "100",
    "HMCMT_EXTRAP_POINTS": "6", "HMCMT_STALL_IT": "30",
    "HMCMT_SIDE_IT": "0",          # 0 automatic
    "HMCMT_EVENT_FLAGS": "1", "HMCMT_DEBUG_FLAGS": "0", "HMCMT_PERSIST_CS": "0", "HMCMT_PERSIST_STRIPS": "2",
    "HMCMT_RESID": "0", "HMCMT_UPD1": "0", "HMCMT_SPMV": "0",      # 0: not given, the heuristic's choice
    "HMCMT_JACOBI_W": "0.8", "HMCMT_PERSIST_BALANCE_SMOOTH": "0.75", "HMCMT_GUARD_LIMIT": "1e-06", "HMCMT_JACOBI_W2": "1",
    "HMCMT_RT": "unset", "HMCMT_RT2": "unset", "HMCMT_RTS": "unset", "HMCMT_BC_FUSED": "unset",
    "HMCMT_UPD2": "-", "HMCMT_BC_BLOCKED": "-",
    "HMCMT_STAMPS": "none", "HMCMT_LOCK_DIR": "/tmp",
}
OUT_OF_SCOPE = {"HMCMT_RCCL_PATH", "HMCMT_DEVICE", "HMCMT_LIB_PATH", "HMCMT_BENCH_NOPROF", "HMCMT_BENCH_FORCE_PG"}

FLAGS = ["HMCMT_TICKS", "HMCMT_NO_FUSED_START", "HMCMT_NO_SIGMA_ROWS", "HMCMT_NO_COEF_ALL", "HMCMT_FWD_STAMPS", "HMCMT_BACK_STAMPS"]
SWITCHES = ["HMCMT_PERSIST", "HMCMT_PS_START", "HMCMT_PERSIST_BALANCE", "HMCMT_TWIST", "HMCMT_FUSED_BACK", "HMCMT_SPEC",
            "HMCMT_LAZY_DINV", "HMCMT_STREAM_PRIORITY", "HMCMT_PERSIST_WIDTHK", "HMCMT_PERSIST_LOCK"]

# (variable, value) -> expected: both clamp edges, one step outside each, a value outside an accepted set
CASES = [
    ("HMCMT_FUSED_FWD", "0", "0"), ("HMCMT_FUSED_FWD", "2", "2"), ("HMCMT_FUSED_FWD", "1", "1"), ("HMCMT_FUSED_FWD", "3", "1"),
    ("HMCMT_FUSED_FWD", "", "1"), ("HMCMT_FUSED_FWD", "off", "1"),
    ("HMCMT_SENS_FUSED", "0", "0"), ("HMCMT_SENS_FUSED", "1", "1"), ("HMCMT_SENS_FUSED", "2", "2"), ("HMCMT_SENS_FUSED", "", "2"),
    ("HMCMT_XFWD", "0", "0"), ("HMCMT_XFWD", "1", "1"), ("HMCMT_XFWD", "", "1"), ("HMCMT_XFWD", "x", "1"),
    ("HMCMT_PS_SPIN", "1024", "1024"), ("HMCMT_PS_SPIN", "1023", "1024"), ("HMCMT_PS_SPIN", "1025", "1025"), ("HMCMT_PS_SPIN", "-5", "1024"),
    ("HMCMT_PS_SPIN", "abc", "1024"),
    ("HMCMT_SWEEPS", "0", "0"), ("HMCMT_SWEEPS", "2", "2"), ("HMCMT_SWEEPS", "-1", "0"), ("HMCMT_SWEEPS", "3", "2"), ("HMCMT_SWEEPS", "1", "1"),
    ("HMCMT_SWEEPS", "auto", "0"), ("HMCMT_SWEEPS", "abc", "0"),
    ("HMCMT_SWEEPS_UP", "1", "1"), ("HMCMT_SWEEPS_UP", "0", "1"), ("HMCMT_SWEEPS_UP", "30", "30"), ("HMCMT_SWEEPS_UP", "abc", "1"),
    ("HMCMT_SWEEPS_DOWN", "0", "0"), ("HMCMT_SWEEPS_DOWN", "-1", "0"), ("HMCMT_SWEEPS_DOWN", "12", "12"), ("HMCMT_SWEEPS_DOWN", "abc", "0"),
    ("HMCMT_GUARD_EVERY", "0", "0"), ("HMCMT_GUARD_EVERY", "-1", "0"), ("HMCMT_GUARD_EVERY", "7", "7"), ("HMCMT_GUARD_EVERY", "abc", "0"),
    ("HMCMT_EXTRAP_POINTS", "2", "2"), ("HMCMT_EXTRAP_POINTS", "1", "2"), ("HMCMT_EXTRAP_POINTS", "6", "6"), ("HMCMT_EXTRAP_POINTS", "7", "6"),
    ("HMCMT_EXTRAP_POINTS", "abc", "2"),
    ("HMCMT_STALL_IT", "1", "1"), ("HMCMT_STALL_IT", "0", "1"), ("HMCMT_STALL_IT", "3", "3"), ("HMCMT_STALL_IT", "abc", "1"),
    ("HMCMT_SIDE_IT", "1", "1"), ("HMCMT_SIDE_IT", "0", "0"), ("HMCMT_SIDE_IT", "-3", "0"), ("HMCMT_SIDE_IT", "9", "9"), ("HMCMT_SIDE_IT", "abc", "0"),
    ("HMCMT_EVENT_FLAGS", "0", "0"), ("HMCMT_EVENT_FLAGS", "1", "1"), ("HMCMT_EVENT_FLAGS", "2", "2"), ("HMCMT_EVENT_FLAGS", "3", "0"),
    ("HMCMT_EVENT_FLAGS", "-1", "0"), ("HMCMT_EVENT_FLAGS", "abc", "0"),
    ("HMCMT_DEBUG_FLAGS", "5", "5"), ("HMCMT_DEBUG_FLAGS", "-2", "-2"), ("HMCMT_DEBUG_FLAGS", "abc", "0"),
    ("HMCMT_PERSIST_CS", "1", "1"), ("HMCMT_PERSIST_CS", "2", "2"), ("HMCMT_PERSIST_CS", "3", "3"), ("HMCMT_PERSIST_CS", "abc", "0"),
    ("HMCMT_PERSIST_STRIPS", "4", "4"), ("HMCMT_PERSIST_STRIPS", "2", "2"), ("HMCMT_PERSIST_STRIPS", "3", "3"), ("HMCMT_PERSIST_STRIPS", "abc", "0"),
    ("HMCMT_RESID", "256", "256"), ("HMCMT_RESID", "512", "512"), ("HMCMT_RESID", "1024", "1024"), ("HMCMT_RESID", "128", "0"),
    ("HMCMT_RESID", "abc", "0"),
    ("HMCMT_UPD1", "256", "256"), ("HMCMT_UPD1", "512", "512"), ("HMCMT_UPD1", "1024", "0"), ("HMCMT_UPD1", "abc", "0"),
    ("HMCMT_SPMV", "256", "256"), ("HMCMT_SPMV", "512", "512"), ("HMCMT_SPMV", "1024", "1024"), ("HMCMT_SPMV", "2048", "0"), ("HMCMT_SPMV", "abc", "0"),
    ("HMCMT_JACOBI_W", "0.1", "0.1"), ("HMCMT_JACOBI_W", "0.05", "0.1"), ("HMCMT_JACOBI_W", "1.2", "1.2"), ("HMCMT_JACOBI_W", "1.3", "1.2"),
    ("HMCMT_JACOBI_W", "0.7", "0.7"), ("HMCMT_JACOBI_W", "abc", "0.1"),
    ("HMCMT_PERSIST_BALANCE_SMOOTH", "0", "0"), ("HMCMT_PERSIST_BALANCE_SMOOTH", "-0.1", "0"), ("HMCMT_PERSIST_BALANCE_SMOOTH", "0.95", "0.949999988"),
    ("HMCMT_PERSIST_BALANCE_SMOOTH", "0.96", "0.949999988"), ("HMCMT_PERSIST_BALANCE_SMOOTH", "0.5", "0.5"), ("HMCMT_PERSIST_BALANCE_SMOOTH", "abc", "0"),
    ("HMCMT_GUARD_LIMIT", "1e-3", "0.001"), ("HMCMT_GUARD_LIMIT", "-1", "-1"), ("HMCMT_GUARD_LIMIT", "abc", "0"),
    ("HMCMT_JACOBI_W2", "0.5", "0.5"), ("HMCMT_JACOBI_W2", "1.5", "1.5"), ("HMCMT_JACOBI_W2", "abc", "0"),
    ("HMCMT_RT", "5", "5"), ("HMCMT_RT", "-1", "-1"), ("HMCMT_RT", "abc", "0"), ("HMCMT_RT", "", "0"),
    ("HMCMT_RT2", "14", "14"), ("HMCMT_RT2", "abc", "0"), ("HMCMT_RTS", "65", "65"), ("HMCMT_RTS", "abc", "0"),
    ("HMCMT_BC_FUSED", "0", "0"), ("HMCMT_BC_FUSED", "4", "4"), ("HMCMT_BC_FUSED", "abc", "0"),
    # partial tuples: the fields parsed, nothing more
    ("HMCMT_UPD2", "512", "512"), ("HMCMT_UPD2", "512,4", "512,4"), ("HMCMT_UPD2", "512,4,14", "512,4,14"), ("HMCMT_UPD2", "512,4,14,9", "512,4,14"),
    ("HMCMT_UPD2", "abc", "-"), ("HMCMT_UPD2", "", "-"), ("HMCMT_UPD2", ",", "-"), ("HMCMT_UPD2", "512,x", "512"),
    ("HMCMT_BC_BLOCKED", "32,256", "32,256"), ("HMCMT_BC_BLOCKED", "0", "0"), ("HMCMT_BC_BLOCKED", "16,512,7,3", "16,512,7,3"),
    ("HMCMT_BC_BLOCKED", "abc", "-"), ("HMCMT_BC_BLOCKED", "", "-"),
    ("HMCMT_STAMPS", "upd", "upd"), ("HMCMT_STAMPS", "spmv", "spmv"), ("HMCMT_STAMPS", "persist", "persist"), ("HMCMT_STAMPS", "all", "none"),
    ("HMCMT_STAMPS", "", "none"), ("HMCMT_STAMPS", "UPD", "none"),
    ("HMCMT_LOCK_DIR", "/var/lock", "/var/lock"), ("HMCMT_LOCK_DIR", "", "/tmp"),
]
CASES += [(n, v, "1") for n in FLAGS for v in ("", "0", "1", "no")]                  # present means on
CASES += [(n, v, e) for n in SWITCHES for v, e in (("", "1"), ("0", "0"), ("1", "1"), ("00", "0"), ("0x", "0"), ("off", "1"), (" 0", "1"))]


def _build(sanitize=False):
    exe = os.path.join(BUILD, "emul_knobs_asan" if sanitize else "emul_knobs")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(BUILD, exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            if sanitize and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
                pytest.skip("the compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
            raise RuntimeError(r.stderr)
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build()


def _run(exe, env, *args):
    r = subprocess.run([exe, *args], env=dict(env), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _knobs(exe, env):
    return dict(line.split(" ", 1) for line in _run(exe, env).splitlines())


def test_empty_environment_gives_every_default(exe):
    assert _knobs(exe, {}) == DEFAULTS


def test_every_variable_is_printed_and_listed(exe):
    assert set(_run(exe, {}, "--list").split()) == set(DEFAULTS)


@pytest.mark.parametrize("name,value,expected", CASES, ids=[f"{n}={v!r}" for n, v, _ in CASES])
def test_parsing_rule(exe, name, value, expected):
    got = _knobs(exe, {name: value})
    assert got[name] == expected
    assert {k: v for k, v in got.items() if k != name} == {k: v for k, v in DEFAULTS.items() if k != name}     # ... and nothing else moves


def test_every_numeric_variable_has_a_non_numeric_case():
    numeric = {n for n, d in DEFAULTS.items() if re.fullmatch(r"-?[0-9.e-]+|unset|-", d)} - set(FLAGS) - set(SWITCHES) - {
        "HMCMT_FUSED_FWD", "HMCMT_SENS_FUSED", "HMCMT_XFWD"}
    assert numeric == {n for n, v, _ in CASES if v == "abc"}


def test_design_table_lists_what_the_reader_asks_for(exe):
    """--list equals, as a set, the variables of the table in DESIGN.md section 6 (the out-of-scope ones are named below it)"""
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    section = text[text.index("### Knobs"):text.index("## 7. Multi-GPU")]
    rows = re.findall(r"^\| `(HMCMT_[A-Z0-9_]+)` \|", section, flags=re.M)
    assert len(rows) == len(set(rows))
    assert set(rows) == set(_run(exe, {}, "--list").split())
    below = section[section.rindex(rows[-1]):]
    assert OUT_OF_SCOPE <= set(re.findall(r"HMCMT_[A-Z0-9_]+", below))
    assert not OUT_OF_SCOPE & set(rows)


def test_hostile_values_under_sanitizers():
    """the same stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, once over hostile values for every variable"""
    exe = _build(sanitize=True)
    for value in ("", "9" * 4096, ",", "-2147483649", "1e999"):
        r = subprocess.run([exe], env={n: value for n in DEFAULTS}, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (value[:16], r.stderr[-2000:])
        assert len(r.stdout.splitlines()) == len(DEFAULTS)
