"""The BiCGStab / dot additions at every boundary that needs no GPU: the
symbols librsp.so exports, their declarations in include/rsp.h, the Python
mirror, and the test_solve driver's usage path."""
import os
import re
import subprocess

from respasol_amd import _lib, sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rsp_bicgstab_create", "rsp_bicgstab_solve", "rsp_bicgstab_history", "rsp_bicgstab_destroy",
       "rsp_dot"]


def test_library_exports_solver_symbols():
    for name in NEW:
        assert hasattr(_lib.rsp, name), name
        assert name in _lib.RSP_PROTOS, name
    # the sixth: the device kernels' entry behind them, one per FTZ namespace
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.LIB_DIR, "librsp.so")],
                         capture_output=True, text=True, check=True).stdout
    for ns in ("rsp_k", "rsp_k_ftz"):
        assert re.search(rf"\b_ZN{len(ns)}{ns}6krylovE", out), ns


def test_header_declares_solver_calls():
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    for name in NEW:
        assert re.search(rf"rsp_status_t\s+{name}\s*\(", text), name
    assert "typedef struct rsp_bicgstab *rsp_bicgstab_t;" in text
    m = re.search(r"typedef enum \{([^}]*)\} rsp_solve_reason_t;", text)
    assert m and [s.strip() for s in m.group(1).split(",")] == [
        "RSP_SOLVE_CONVERGED = 0", "RSP_SOLVE_MAX_ITERS = 1", "RSP_SOLVE_BREAKDOWN = 2"]


def test_python_mirror_exposes_solver():
    assert callable(sparse.BiCGStab) and callable(sparse.dot)
    assert "BiCGStab" in sparse.__all__ and "dot" in sparse.__all__
    assert (sparse.BiCGStab.CONVERGED, sparse.BiCGStab.MAX_ITERS, sparse.BiCGStab.BREAKDOWN) == (0, 1, 2)


def test_reduction_geometry_matches_kernels():
    """_lib.KRY_CHUNK / KRY_MAX_GRID (what the GPU tests size their cases
    from) are the constants the kernels are compiled with."""
    text = open(os.path.join(ROOT, "respasol_amd", "csrc", "rsp_kernels.h")).read()
    assert int(re.search(r"constexpr int kKryChunk = (\d+);", text).group(1)) == _lib.KRY_CHUNK
    assert int(re.search(r"constexpr int kKryMaxGrid = (\d+);", text).group(1)) == _lib.KRY_MAX_GRID


def test_solve_driver_usage():
    r = subprocess.run([os.path.join(_lib.BIN_DIR, "test_solve")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "Usage" in r.stderr and "--precond=fp64|fp32|none" in r.stderr
    assert "--full-symmetric" in r.stderr and "lower triangle" in r.stderr
