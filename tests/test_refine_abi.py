"""The iterative-refinement additions at every boundary that needs no GPU: the
symbols librsp.so exports, their declarations in include/rsp.h, the fourth
solve reason, the Python mirror and the test_solve driver's --refine flag."""
import os
import re
import subprocess

from respasol_amd import _lib, sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rsp_refine_create", "rsp_refine_solve", "rsp_refine_history", "rsp_refine_destroy",
       "rsp_convert_scaled", "rsp_refine_update"]


def header():
    return open(os.path.join(ROOT, "include", "rsp.h")).read()


def test_library_exports_refine_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.LIB_DIR, "librsp.so")],
                         capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(rf"\bT {name}$", out, re.M), name
        assert hasattr(_lib.rsp, name), name
        assert name in _lib.RSP_PROTOS, name
    # the kernels behind them, one entry per FTZ namespace
    for ns in ("rsp_k", "rsp_k_ftz"):
        assert re.search(rf"\b_ZN{len(ns)}{ns}6refineE", out), ns


def test_header_declares_refine_calls():
    text = header()
    for name in NEW:
        assert re.search(rf"rsp_status_t\s+{name}\s*\(", text), name
    assert "typedef struct rsp_refine *rsp_refine_t;" in text
    m = re.search(r"typedef enum \{([^}]*)\} rsp_refine_method_t;", text)
    assert m and [s.strip() for s in m.group(1).split(",")] == [
        "RSP_REFINE_BICGSTAB = 0", "RSP_REFINE_CG = 1", "RSP_REFINE_GMRES = 2"]


def test_stagnated_is_the_fourth_reason():
    """RSP_SOLVE_STAGNATED is a value of rsp_solve_reason_t equal to 3, the
    three earlier values stand, and a C compiler agrees."""
    text = header()
    assert re.search(r"#define\s+RSP_SOLVE_STAGNATED\s+\(\(rsp_solve_reason_t\)3\)", text)
    m = re.search(r"typedef enum \{([^}]*)\} rsp_solve_reason_t;", text)
    assert m and [s.strip() for s in m.group(1).split(",")][:3] == [
        "RSP_SOLVE_CONVERGED = 0", "RSP_SOLVE_MAX_ITERS = 1", "RSP_SOLVE_BREAKDOWN = 2"]
    src = ('#include "rsp.h"\n'
           "_Static_assert(RSP_SOLVE_STAGNATED == 3 && RSP_SOLVE_BREAKDOWN == 2, \"reasons\");\n"
           "rsp_solve_reason_t r = RSP_SOLVE_STAGNATED;\n")
    r = subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert _lib.SOLVE_STAGNATED == 3
    assert (_lib.REFINE_BICGSTAB, _lib.REFINE_CG, _lib.REFINE_GMRES) == (0, 1, 2)


def test_python_mirror_exposes_refine():
    assert callable(sparse.Refine) and callable(sparse.convert_scaled) and callable(sparse.refine_update)
    for name in ("Refine", "convert_scaled", "refine_update"):
        assert name in sparse.__all__, name
    R = sparse.Refine
    assert (R.CONVERGED, R.MAX_ITERS, R.BREAKDOWN, R.STAGNATED) == (0, 1, 2, 3)
    assert R.METHODS == {"bicgstab": 0, "cg": 1, "gmres": 2}
    assert "rsp_refine_" in sparse.__doc__ and "rsp_convert_scaled" in sparse.__doc__
    res = sparse.SolveResult(None, 7, 0.5, 3, [1.0, 0.5], steps=1, inner_history=[0, 7])
    assert (res.steps, res.inner_history, res.history) == (1, [0, 7], [1.0, 0.5])
    assert sparse.SolveResult(None, 1, 0.0, 0, []).steps is None  # the other solvers' results are what they were


def test_solve_driver_usage_shows_refine():
    exe = os.path.join(_lib.BIN_DIR, "test_solve")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "[--refine[=inner_rtol]]" in r.stderr and "--refine:" in r.stderr
    # everything the earlier ABI tests check is still there
    assert "--method=bicgstab|gmres|cg" in r.stderr and "--restart" in r.stderr and "both triangles" in r.stderr
    assert "Usage" in r.stderr and "--precond=fp64|fp32|none" in r.stderr
    assert "--full-symmetric" in r.stderr and "lower triangle" in r.stderr


def test_solve_driver_refuses_refine_outside_fp64_over_fp32():
    """--refine with an fp32 iteration, or with an fp64 preconditioner (given or
    by default), exits 2 with a message before anything is loaded."""
    exe = os.path.join(_lib.BIN_DIR, "test_solve")
    for extra in (["--prec=fp32"], ["--prec=fp32", "--precond=fp32"], ["--precond=fp64"], []):
        r = subprocess.run([exe, "surrogate:G2_circuit@0.01", "--refine", *extra], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert "--refine needs --prec=fp64 and --precond=fp32 or none" in r.stderr
        assert r.stdout == ""
