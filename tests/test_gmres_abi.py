"""The GMRES additions at every boundary that needs no GPU: the symbols
librsp.so exports, their declarations in include/rsp.h, the Python mirror, the
test_solve driver's usage text, and the solver's small least-squares step
(rsp_gmres_lsq_host: the Givens rotations and the back-substitution that the
kernels run, on host arrays) against numpy.linalg.lstsq.

Least-squares bound: H = uniform(-1, 1) upper Hessenberg + 4 on the diagonal
has a condition number <= 1e3 (asserted), a sequence of k rotations is
backward stable with an error of order k * 2^-52, so
|y - y_ref| <= 1e3 * k * 2^-52 * ||y_ref||, and the same bound, relative to
beta, for the residual norm est[k - 1]. numpy's own solution is checked for
stability on these inputs through its normal-equations residual.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from respasol_amd import _lib, sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rsp_gmres_create", "rsp_gmres_solve", "rsp_gmres_history", "rsp_gmres_destroy",
       "rsp_orthogonalize", "rsp_gmres_lsq_host"]
dp = C.POINTER(C.c_double)


def test_library_exports_gmres_symbols():
    for name in NEW:
        assert hasattr(_lib.rsp, name), name
        assert name in _lib.RSP_PROTOS, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.LIB_DIR, "librsp.so")],
                         capture_output=True, text=True, check=True).stdout
    for ns in ("rsp_k", "rsp_k_ftz"):
        assert re.search(rf"\b_ZN{len(ns)}{ns}5gmresE", out), ns


def test_header_declares_gmres_calls():
    text = open(os.path.join(ROOT, "include", "rsp.h")).read()
    for name in NEW:
        assert re.search(rf"rsp_status_t\s+{name}\s*\(", text), name
    assert "typedef struct rsp_gmres *rsp_gmres_t;" in text
    m = re.search(r"#define\s+RSP_GMRES_MAX_RESTART\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.GMRES_MAX_RESTART == 64
    kern = open(os.path.join(ROOT, "respasol_amd", "csrc", "rsp_kernels.h")).read()
    assert int(re.search(r"constexpr int kGmMax = (\d+);", kern).group(1)) == _lib.GMRES_MAX_RESTART


def test_python_mirror_exposes_gmres():
    assert callable(sparse.GMRES) and callable(sparse.orthogonalize)
    assert "GMRES" in sparse.__all__ and "orthogonalize" in sparse.__all__
    assert (sparse.GMRES.CONVERGED, sparse.GMRES.MAX_ITERS, sparse.GMRES.BREAKDOWN) == (0, 1, 2)


def test_solve_driver_usage_shows_method_and_restart():
    r = subprocess.run([os.path.join(_lib.BIN_DIR, "test_solve")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0
    assert "--method=bicgstab|gmres" in r.stderr and "--restart" in r.stderr
    # what the usage text held before stays
    assert "Usage" in r.stderr and "--precond=fp64|fp32|none" in r.stderr
    assert "--full-symmetric" in r.stderr and "lower triangle" in r.stderr


def lsq_host(H, beta):
    k = H.shape[1]
    Hf = np.asfortranarray(H, dtype=np.float64)
    y, est = np.zeros(k), np.zeros(k)
    st = _lib.rsp.rsp_gmres_lsq_host(k, k + 1, Hf.ctypes.data_as(dp), float(beta), y.ctypes.data_as(dp),
                                     est.ctypes.data_as(dp))
    return st, y, est


def hessenberg(k, seed):
    rng = np.random.default_rng(seed)
    H = np.triu(rng.uniform(-1.0, 1.0, (k + 1, k)), -1)
    H[np.arange(k), np.arange(k)] += 4.0
    return H


@pytest.mark.parametrize("k", [1, 2, 5, 30, 64])
def test_lsq_host_against_numpy(k):
    H = hessenberg(k, 1000 + k)
    beta = 2.5
    rhs = np.zeros(k + 1)
    rhs[0] = beta
    cond = np.linalg.cond(H)
    assert cond <= 1e3
    y_ref, _, rank, _ = np.linalg.lstsq(H, rhs, rcond=None)
    assert rank == k
    res_ref = float(np.linalg.norm(rhs - H @ y_ref))
    bound = 1e3 * k * 2.0 ** -52
    # numpy's side is itself stable here: H^T (rhs - H y_ref) = 0 to rounding
    assert np.linalg.norm(H.T @ (rhs - H @ y_ref)) <= bound * np.linalg.norm(H, 2) * beta
    st, y, est = lsq_host(H, beta)
    assert st == _lib.STATUS_SUCCESS
    err = float(np.max(np.abs(y - y_ref)))
    print(f"k={k} cond={cond:.2f} err={err:.3e} bound={bound * np.linalg.norm(y_ref):.3e} "
          f"est={est[-1]:.17g} ref={res_ref:.17g}")
    assert err <= bound * np.linalg.norm(y_ref)
    assert abs(est[k - 1] - res_ref) <= bound * beta
    assert np.all(np.diff(est) <= 0.0) and est[0] <= beta
    # every prefix is its own least-squares problem
    for j in {1, k // 2, k - 1} - {0}:
        r_j = np.linalg.lstsq(H[:j + 1, :j], rhs[:j + 1], rcond=None)[0]
        assert abs(est[j - 1] - np.linalg.norm(rhs[:j + 1] - H[:j + 1, :j] @ r_j)) <= bound * beta


def test_lsq_host_argument_checks():
    H = hessenberg(3, 7)
    y, est = np.zeros(3), np.zeros(3)
    f = _lib.rsp.rsp_gmres_lsq_host
    Hf = np.asfortranarray(H)
    H_ptr, y_ptr, e_ptr = Hf.ctypes.data_as(dp), y.ctypes.data_as(dp), est.ctypes.data_as(dp)
    assert f(0, 4, H_ptr, 1.0, y_ptr, e_ptr) == _lib.STATUS_INVALID_VALUE
    assert f(_lib.GMRES_MAX_RESTART + 1, 100, H_ptr, 1.0, y_ptr, e_ptr) == _lib.STATUS_INVALID_VALUE
    assert f(3, 3, H_ptr, 1.0, y_ptr, e_ptr) == _lib.STATUS_INVALID_VALUE
    assert f(3, 4, None, 1.0, y_ptr, e_ptr) == _lib.STATUS_INVALID_VALUE
    # a singular first column: the rotated diagonal is 0
    Z = np.zeros((2, 1), order="F")
    assert f(1, 2, Z.ctypes.data_as(dp), 1.0, y_ptr, e_ptr) == _lib.STATUS_INVALID_VALUE
    # the BiCGStab breakdown case's Hessenberg matrix: [[0, -1], [1, 0], [0, 0]], beta = 1
    Hs = np.asfortranarray(np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 0.0]]))
    y2, e2 = np.zeros(2), np.zeros(2)
    assert f(2, 3, Hs.ctypes.data_as(dp), 1.0, y2.ctypes.data_as(dp), e2.ctypes.data_as(dp)) == 0
    assert y2.tolist() == [0.0, -1.0] and e2.tolist() == [1.0, 0.0]
