"""Python host mirror of the operator boundary (include/rsp.h) on torch
device tensors. torch provides device memory, the stream and events —
plumbing only; every operation runs the HIP kernels of librsp.so.

Mapping to the reference's cuSPARSE usage:
  Handle                 cusparseCreate / cusparseDestroy   (GPU/spmv.cu:128,282)
  SpMat                  cusparseCreateCsr + SpMV_bufferSize (builds the
                         schedule) + the caller's workspace cudaMalloc
                                                             (GPU/spmv.cu:148-164)
  SpMat.spmv             cusparseSpMV                        (GPU/spmv.cu:184-186);
                         transpose=True: op = CUSPARSE_OPERATION_TRANSPOSE, on a
                         transposed side built on first use
                         (SpMat.preprocess_transpose rebuilds it)
  csr2csc                cusparseCsr2cscEx2: the CSR arrays of A^T in the order
                         SpMat.spmv(transpose=True) uses (rsp_csr2csc)
  csr_transpose_host     the same transpose of a host pattern, no device
                         (rsp_csr_transpose_host)
  SpmvBatch              cusparseSpMV over several matrices as one launch (no
                         cuSPARSE counterpart; bits equal to SpMat.spmv each)
  Ilu0.analysis          csrilu02_analysis + 2x csrsv2_analysis (GPU/ilu0.cu:203-252)
  Ilu0.zero_pivot        cusparseXcsrilu02_zeroPivot         (GPU/ilu0.cu:222,278)
  Ilu0.solve_zero_pivot  cusparseXcsrsv2_zeroPivot (the csrsv2 infos, GPU/ilu0.cu:143-150)
  Ilu0.factor            cusparse?csrilu02                   (GPU/ilu0.cu:264-268)
  Ilu0.solve_lower       cusparse?csrsv2_solve, desc_L, op N / op T (GPU/ilu0.cu:296-302)
  BiCGStab               the loop those calls are normally used in: ILU(0)-
                         preconditioned BiCGStab (rsp_bicgstab_*; no single
                         cuSPARSE call)
  CG                     ILU(0)-preconditioned conjugate gradients for a
                         symmetric positive definite A (rsp_cg_*)
  GMRES                  restarted flexible GMRES(m) on the same operators
                         (rsp_gmres_*)
  Refine                 mixed-precision iterative refinement: fp64 residuals
                         and updates around an all-fp32 BiCGStab / CG / GMRES
                         solve of the correction (rsp_refine_*)
  Cheby                  a Chebyshev polynomial preconditioner z = p_k(D^-1 A)
                         D^-1 r made of SpMVs alone (rsp_cheby_*); the solvers
                         take it as cheby= in the place of ilu= / factor=
  cheby_coefficients     its coefficients in fp64, no device
                         (rsp_cheby_coefficients_host)
  convert_scaled         dst = dst_type(src * 2^exp2), one rounding
                         (rsp_convert_scaled)
  refine_update          x_old = x; x += 2^exp2 * double(d) (rsp_refine_update)
  dot                    cublasDdot on the solver's reduction (rsp_dot)
  orthogonalize          one twice-applied Gram-Schmidt step of GMRES
                         (rsp_orthogonalize)
Errors raise RspError carrying the rsp_status_t (numbered like cusparseStatus_t).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import RspError, check, rsp

_DT = {torch.float64: _lib.R_64F, torch.float32: _lib.R_32F}


def _ptr(t: torch.Tensor | None) -> C.c_void_p:
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def _scalar(value: float, dtype: torch.dtype):
    return C.c_double(value) if dtype == torch.float64 else C.c_float(value)


class Handle:
    """rsp_handle_t bound to the current HIP device and a stream (default:
    torch's current stream, so torch events time the kernels)."""

    def __init__(self, stream: torch.cuda.Stream | None = None, ftz: bool = False):
        if not torch.cuda.is_available():
            raise RuntimeError("respasol_amd.sparse needs a HIP device (MI355X, gfx950)")
        self._h = C.c_void_p()
        check(rsp.rsp_create(C.byref(self._h)), "rsp_create")
        self.set_stream(stream if stream is not None else torch.cuda.current_stream())
        self.set_ftz(ftz)

    @property
    def ptr(self) -> C.c_void_p:
        return self._h

    def set_stream(self, stream: torch.cuda.Stream) -> None:
        self.stream = stream
        check(rsp.rsp_set_stream(self._h, C.c_void_p(stream.cuda_stream)), "rsp_set_stream")

    def set_ftz(self, on: bool) -> None:
        self.ftz = bool(on)
        check(rsp.rsp_set_ftz(self._h, 1 if on else 0), "rsp_set_ftz")

    def close(self) -> None:
        if self._h:
            rsp.rsp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


def upload_csr(rowptr: np.ndarray, colidx: np.ndarray, values: np.ndarray,
               dtype: torch.dtype = torch.float64, device: str | torch.device = "cuda"):
    """Host CSR arrays -> device tensors (values cast on the host with
    round-to-nearest, as the reference's fp32 demotion, GPU/spmv.cu:64-67)."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    rp = torch.from_numpy(np.ascontiguousarray(rowptr, np.int32)).to(device)
    ci = torch.from_numpy(np.ascontiguousarray(colidx, np.int32)).to(device)
    va = torch.from_numpy(np.ascontiguousarray(values).astype(np_dt)).to(device)
    return rp, ci, va


class SpMat:
    """A device CSR matrix with its SpMV schedule (rsp_spmat_t + workspace)."""

    def __init__(self, handle: Handle, rowptr: torch.Tensor, colidx: torch.Tensor,
                 values: torch.Tensor, n_cols: int, nnz: int | None = None):
        if values.dtype not in _DT:
            raise TypeError("values must be float64 or float32")
        if rowptr.dtype != torch.int32 or colidx.dtype != torch.int32:
            raise TypeError("rowptr/colidx must be int32 (CUSPARSE_INDEX_32I)")
        self.handle = handle
        self.rowptr, self.colidx, self.values = rowptr, colidx, values
        self.m = rowptr.numel() - 1
        self.n = int(n_cols)
        self.dtype = values.dtype
        self.nnz = int(nnz if nnz is not None else colidx.numel())
        self._mat = C.c_void_p()
        check(rsp.rsp_create_csr(C.byref(self._mat), self.m, self.n, self.nnz, _ptr(rowptr),
                                 _ptr(colidx), _ptr(values), _DT[self.dtype]), "rsp_create_csr")
        one, zero = _scalar(1.0, self.dtype), _scalar(0.0, self.dtype)
        size = C.c_size_t()
        check(rsp.rsp_spmv_buffer_size(handle.ptr, _lib.OP_N, C.byref(one), self._mat,
                                       C.byref(zero), _DT[self.dtype], C.byref(size)),
              "rsp_spmv_buffer_size")
        # the reference's sequence (GPU/spmv.cu:159-164): bufferSize (which
        # builds the schedule inside the matrix) and the caller's workspace
        self.buffer = torch.empty(max(int(size.value), 1), dtype=torch.uint8, device=values.device)

    @property
    def nnz_stored(self) -> int:
        return int(self.colidx.numel())

    def spmv(self, x: torch.Tensor, y: torch.Tensor | None = None, alpha: float = 1.0,
             beta: float = 0.0, transpose: bool = False) -> torch.Tensor:
        """y = alpha*A*x + beta*y on the handle's stream (cusparseSpMV), or with
        transpose=True y = alpha*A^T*x + beta*y (x of m, y of n elements): the
        first such call builds the matrix's transposed side (host-blocking),
        and every one permutes the current values before the product."""
        n_in, n_out = (self.m, self.n) if transpose else (self.n, self.m)
        if x.dtype != self.dtype or x.numel() < n_in:
            raise ValueError("x has the wrong dtype or length")
        if y is None:
            y = torch.empty(n_out, dtype=self.dtype, device=x.device)
        elif transpose and (y.dtype != self.dtype or y.numel() < n_out):
            raise ValueError("y has the wrong dtype or length")
        a, b = _scalar(alpha, self.dtype), _scalar(beta, self.dtype)
        check(rsp.rsp_spmv(self.handle.ptr, _lib.OP_T if transpose else _lib.OP_N, C.byref(a), self._mat,
                           _ptr(x), C.byref(b), _ptr(y), _DT[self.dtype], _ptr(self.buffer)), "rsp_spmv")
        return y

    def preprocess_transpose(self) -> None:
        """Rebuild the transposed side from the pattern arrays as they are now
        (rsp_spmv_preprocess, op = TRANSPOSE; host-blocking). Only needed after
        the pattern changed in place: spmv(transpose=True) builds it on first use."""
        one, zero = _scalar(1.0, self.dtype), _scalar(0.0, self.dtype)
        check(rsp.rsp_spmv_preprocess(self.handle.ptr, _lib.OP_T, C.byref(one), self._mat, None,
                                      C.byref(zero), None, _DT[self.dtype], _ptr(self.buffer)),
              "rsp_spmv_preprocess")

    def bind(self, x: torch.Tensor, y: torch.Tensor, alpha: float = 1.0, beta: float = 0.0):
        """The call y = alpha*A*x + beta*y with its C arguments converted once:
        returns a no-argument callable that issues exactly one rsp_spmv (the
        C driver's per-call cost, without the per-call Python argument
        conversion of spmv(); for timing loops of many short calls)."""
        if x.dtype != self.dtype or x.numel() < self.n or y.dtype != self.dtype or y.numel() < self.m:
            raise ValueError("x / y have the wrong dtype or length")
        a, b = _scalar(alpha, self.dtype), _scalar(beta, self.dtype)
        args = (self.handle.ptr, _lib.OP_N, C.byref(a), self._mat, _ptr(x), C.byref(b), _ptr(y),
                _DT[self.dtype], _ptr(self.buffer))
        keep = (a, b, x, y)  # the scalars and tensors the pointers refer to
        fn = rsp.rsp_spmv

        def call():
            st = fn(*args)
            if st:
                check(st, "rsp_spmv")
        call.keep = keep
        return call

    def set_values(self, values: torch.Tensor) -> None:
        """Re-point the values array, of either type (rsp_csr_set_values): the
        schedule is kept for the same type and rebuilt by the next call for
        another; batches created before hold the old pointer and become stale.
        The tensor is kept alive."""
        if values.dtype not in _DT:
            raise TypeError("values must be float64 or float32")
        if values.numel() < self.nnz_stored:
            raise ValueError("values is shorter than the pattern")
        check(rsp.rsp_csr_set_values(self._mat, _ptr(values), _DT[values.dtype]), "rsp_csr_set_values")
        self.values = values
        self.dtype = values.dtype

    def set_local_cols(self, ncols_local: int) -> None:
        """Split the schedule for halo overlap (rsp_spmat_set_local_cols): tiles
        reading columns < ncols_local only (the rank's own x) run as part 1."""
        check(rsp.rsp_spmat_set_local_cols(self._mat, int(ncols_local)), "rsp_spmat_set_local_cols")
        one, zero = _scalar(1.0, self.dtype), _scalar(0.0, self.dtype)
        check(rsp.rsp_spmv_preprocess(self.handle.ptr, _lib.OP_N, C.byref(one), self._mat, None,
                                      C.byref(zero), None, _DT[self.dtype], _ptr(self.buffer)),
              "rsp_spmv_preprocess")

    def plan_info(self) -> dict:
        """{"tiles", "entries_16bit"} of the current schedule (rsp_spmv_plan_info)."""
        t, e = C.c_int64(), C.c_int64()
        check(rsp.rsp_spmv_plan_info(self._mat, C.byref(t), C.byref(e)), "rsp_spmv_plan_info")
        return {"tiles": t.value, "entries_16bit": e.value}

    def spmv_part(self, x: torch.Tensor, y: torch.Tensor, part: int, alpha: float = 1.0) -> torch.Tensor:
        """Part 1 (interior tiles) or 2 (the rest + fixup) of y = alpha*A*x (rsp_spmv_part)."""
        if x.dtype != self.dtype or x.numel() < self.n:
            raise ValueError("x has the wrong dtype or length")
        a, b = _scalar(alpha, self.dtype), _scalar(0.0, self.dtype)
        check(rsp.rsp_spmv_part(self.handle.ptr, C.byref(a), self._mat, _ptr(x), C.byref(b), _ptr(y),
                                _DT[self.dtype], _ptr(self.buffer), int(part)), "rsp_spmv_part")
        return y

    def close(self) -> None:
        if self._mat:
            rsp.rsp_destroy_spmat(self._mat)
            self._mat = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


PLAN_STATS = ("tiles", "packed_tiles", "packed_entries", "schedule_bytes", "rowptr_bytes", "staged_tiles",
              "index_bytes", "packed_rowoff_bytes")


def spmv_plan_stats(rowptr, colidx, fp32: bool = False, nnz: int | None = None) -> dict:
    """What one SpMV over the schedule of a HOST pattern reads besides the
    values, x and y (rsp_spmv_plan_stats; no device needed). RSP_SPMV_PACK in
    the environment selects the packed records, as for every schedule."""
    import numpy as np

    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colidx, np.int32)
    out = (C.c_int64 * len(PLAN_STATS))()
    check(rsp.rsp_spmv_plan_stats(len(rp) - 1, rp.ctypes.data, ci.ctypes.data,
                                  int(nnz if nnz is not None else len(ci)), 1 if fp32 else 0, out),
          "rsp_spmv_plan_stats")
    return dict(zip(PLAN_STATS, (int(v) for v in out)))


TILE_FACTS = ("r0", "r1", "k0", "k1", "kind", "base", "U", "R", "packed", "packed_rows")
TILE_KINDS = ("int32", "gather16", "runs", "list")


def spmv_plan_tiles(rowptr, colidx, fp32: bool = False, nnz: int | None = None, spread: int = 0,
                    local_cols: int = -1, row_align: int = 1, use_c16: bool = True, use_stage: bool = True) -> dict:
    """The verified schedule of a HOST pattern tile by tile
    (rsp_spmv_plan_tiles_host; no device needed): {"tiles": [one dict of
    TILE_FACTS per tile, "kind" as a TILE_KINDS name], "nint", "nlong",
    "nslots"}. The plan-time knobs come from the environment."""
    import numpy as np

    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colidx, np.int32)
    args = (len(rp) - 1, rp.ctypes.data, ci.ctypes.data, int(nnz if nnz is not None else len(ci)), 1 if fp32 else 0,
            int(spread), int(local_cols), int(row_align), int(use_c16), int(use_stage))
    counts = (C.c_int64 * 4)()
    check(rsp.rsp_spmv_plan_tiles_host(*args, None, 0, counts), "rsp_spmv_plan_tiles_host")
    facts = np.zeros((counts[0], len(TILE_FACTS)), np.int64)
    check(rsp.rsp_spmv_plan_tiles_host(*args, facts.ctypes.data, facts.shape[0], counts), "rsp_spmv_plan_tiles_host")
    tiles = [dict(zip(TILE_FACTS, (int(v) for v in row))) for row in facts]
    for t in tiles:
        t["kind"] = TILE_KINDS[t["kind"]]
    return {"tiles": tiles, "nint": int(counts[1]), "nlong": int(counts[2]), "nslots": int(counts[3])}


class SpmvBatch:
    """Several independent products y_j = alpha*A_j*x_j (+ beta*y_j) as one
    launch (rsp_spmv_batch_*): the same bits per matrix as SpMat.spmv /
    spmv_part, without one kernel ramp and drain per matrix. The x/y tensors
    are recorded: keep them (and the matrices) alive and in place."""

    def __init__(self, handle: Handle, mats: list[SpMat], xs: list[torch.Tensor],
                 ys: list[torch.Tensor], part: int = 0):
        if not (len(mats) == len(xs) == len(ys)):
            raise ValueError("mats, xs and ys must have the same length")
        dt = mats[0].dtype if mats else torch.float64
        for A, x, y in zip(mats, xs, ys):
            if A.dtype != dt or x.dtype != dt or y.dtype != dt:
                raise ValueError("one compute type per batch")
            if x.numel() < A.n or y.numel() < A.m:
                raise ValueError("x or y too short")
        self.handle, self.dtype, self.part = handle, dt, int(part)
        self._keep = (list(mats), list(xs), list(ys))
        n = len(mats)
        arr = C.c_void_p * max(n, 1)
        self._b = C.c_void_p()
        check(rsp.rsp_spmv_batch_create(
            handle.ptr, n, arr(*[A._mat.value for A in mats]), arr(*[x.data_ptr() for x in xs]),
            arr(*[y.data_ptr() for y in ys]), arr(*[A.buffer.data_ptr() for A in mats]),
            _DT[dt], self.part, C.byref(self._b)), "rsp_spmv_batch_create")

    def run(self, alpha: float = 1.0, beta: float = 0.0) -> None:
        a, b = _scalar(alpha, self.dtype), _scalar(beta, self.dtype)
        check(rsp.rsp_spmv_batch_run(self.handle.ptr, self._b, C.byref(a), C.byref(b)),
              "rsp_spmv_batch_run")

    def info(self) -> dict:
        """{"tiles", "entries_16bit"} of the batch's own schedule (rsp_spmv_batch_info)."""
        t, e = C.c_int64(), C.c_int64()
        check(rsp.rsp_spmv_batch_info(self._b, C.byref(t), C.byref(e)), "rsp_spmv_batch_info")
        return {"tiles": t.value, "entries_16bit": e.value}

    def close(self) -> None:
        if self._b:
            rsp.rsp_spmv_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class Ilu0:
    """ILU(0) + unit-lower triangular solves on one analysed pattern."""

    def __init__(self, handle: Handle, rowptr: torch.Tensor, colidx: torch.Tensor,
                 nnz: int | None = None):
        self.handle = handle
        self.rowptr, self.colidx = rowptr, colidx
        self.n = rowptr.numel() - 1
        self.nnz = int(nnz if nnz is not None else colidx.numel())
        self._info = C.c_void_p()
        check(rsp.rsp_create_ilu0_info(C.byref(self._info)), "rsp_create_ilu0_info")

    def analysis(self) -> None:
        """cusparse?csrilu02_analysis (rsp_ilu0_analysis): the solve plans
        are finished by trsv_analysis() or the first solve."""
        check(rsp.rsp_ilu0_analysis(self.handle.ptr, self.n, self.nnz, _ptr(self.rowptr),
                                    _ptr(self.colidx), self._info), "rsp_ilu0_analysis")

    def trsv_analysis(self, transpose: bool = False) -> None:
        """cusparse?csrsv2_analysis (rsp_trsv_analysis) for the L (or L^T) solve."""
        op = _lib.OP_T if transpose else _lib.OP_N
        check(rsp.rsp_trsv_analysis(self.handle.ptr, op, self._info), "rsp_trsv_analysis")

    def zero_pivot(self) -> int:
        """-1 if none, else the 0-based row (cusparseXcsrilu02_zeroPivot)."""
        pos = C.c_int(-1)
        st = rsp.rsp_ilu0_zero_pivot(self.handle.ptr, self._info, C.byref(pos))
        if st == _lib.STATUS_ZERO_PIVOT:
            return pos.value
        check(st, "rsp_ilu0_zero_pivot")
        return -1

    TRSV_L, TRSV_LT, TRSV_U = 0, 1, 2

    def solve_zero_pivot(self, which: int) -> int:
        """cusparseXcsrsv2_zeroPivot for the last solve of kind `which`
        (TRSV_L / TRSV_LT / TRSV_U): -1 if none, else the 0-based row (U
        only); raises RspError(EXECUTION_FAILED) if that solve's persistent
        launch gave up a dependency wait."""
        pos = C.c_int(-1)
        st = rsp.rsp_trsv_zero_pivot(self.handle.ptr, self._info, which, C.byref(pos))
        if st == _lib.STATUS_ZERO_PIVOT:
            return pos.value
        check(st, "rsp_trsv_zero_pivot")
        return -1

    def levels(self) -> tuple[int, int]:
        lo, up = C.c_int(), C.c_int()
        check(rsp.rsp_ilu0_levels(self._info, C.byref(lo), C.byref(up)), "rsp_ilu0_levels")
        return lo.value, up.value

    def solve_blocks(self) -> tuple[int, int]:
        """Blocks of the block-inverse L / L^T solves (0: level-scheduled)."""
        lo, up = C.c_int(), C.c_int()
        check(rsp.rsp_ilu0_solve_blocks(self._info, C.byref(lo), C.byref(up)), "rsp_ilu0_solve_blocks")
        return lo.value, up.value

    def factor(self, values: torch.Tensor) -> None:
        check(rsp.rsp_ilu0_factor(self.handle.ptr, self._info, _DT[values.dtype], _ptr(values)),
              "rsp_ilu0_factor")

    def solve_lower(self, values: torch.Tensor, x: torch.Tensor, y: torch.Tensor | None = None,
                    transpose: bool = False, alpha: float = 1.0) -> torch.Tensor:
        if y is None:
            y = torch.empty_like(x)
        a = _scalar(alpha, values.dtype)
        check(rsp.rsp_trsv_lower_unit(self.handle.ptr, _lib.OP_T if transpose else _lib.OP_N,
                                      C.byref(a), self._info, _DT[values.dtype], _ptr(values),
                                      _ptr(x), _ptr(y)), "rsp_trsv_lower_unit")
        return y

    def solve_upper(self, values: torch.Tensor, x: torch.Tensor, y: torch.Tensor | None = None,
                    alpha: float = 1.0) -> torch.Tensor:
        if y is None:
            y = torch.empty_like(x)
        a = _scalar(alpha, values.dtype)
        check(rsp.rsp_trsv_upper(self.handle.ptr, C.byref(a), self._info, _DT[values.dtype],
                                 _ptr(values), _ptr(x), _ptr(y)), "rsp_trsv_upper")
        return y

    def close(self) -> None:
        if self._info:
            rsp.rsp_destroy_ilu0_info(self._info)
            self._info = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class Cheby:
    """A Chebyshev polynomial preconditioner on A (rsp_cheby_*): z = p_k(D^-1 A)
    D^-1 r with `degree` terms (degree - 1 SpMVs per apply), D the diagonal
    (scaling="jacobi") or I ("none"), on [lmax / ratio, lmax], lmax the
    Gershgorin bound of D^-1 A. A's dtype is the polynomial's type. A missing,
    zero or non-finite diagonal raises RspError(ZERO_PIVOT) whose `position` is
    the smallest such row. A is kept alive; one Cheby serves one solve at a time."""

    SCALINGS = {"none": _lib.CHEBY_SCALE_NONE, "jacobi": _lib.CHEBY_SCALE_JACOBI}

    def __init__(self, handle: Handle, A: SpMat, degree: int = 4, scaling: str = "jacobi", ratio: float = 30.0):
        if scaling not in self.SCALINGS:
            raise ValueError("scaling is jacobi or none")
        self.handle, self.A = handle, A
        self.degree, self.scaling, self.dtype = int(degree), scaling, A.dtype
        self._c = C.c_void_p()
        pos = C.c_int(-1)
        st = rsp.rsp_cheby_create(handle.ptr, A._mat, self.degree, self.SCALINGS[scaling], float(ratio),
                                  C.byref(pos), C.byref(self._c))
        if st != _lib.STATUS_SUCCESS:
            err = RspError(st, "rsp_cheby_create")
            err.position = pos.value
            raise err

    @property
    def bounds(self) -> tuple[float, float]:
        """(lmin, lmax) the coefficients are computed from."""
        lo, hi = C.c_double(), C.c_double()
        check(rsp.rsp_cheby_get_bounds(self._c, C.byref(lo), C.byref(hi)), "rsp_cheby_get_bounds")
        return lo.value, hi.value

    def set_bounds(self, lmin: float, lmax: float) -> None:
        check(rsp.rsp_cheby_set_bounds(self._c, float(lmin), float(lmax)), "rsp_cheby_set_bounds")

    def apply(self, r: torch.Tensor, z: torch.Tensor | None = None) -> torch.Tensor:
        """z = M^-1 r on the handle's stream; r is unchanged and may not be z."""
        if r.dtype != self.dtype or r.numel() != self.A.m:
            raise ValueError("r has the wrong dtype or length")
        if z is None:
            z = torch.empty_like(r)
        elif z.dtype != self.dtype or z.numel() != self.A.m:
            raise ValueError("z has the wrong dtype or length")
        check(rsp.rsp_cheby_apply(self.handle.ptr, self._c, C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr())),
              "rsp_cheby_apply")
        return z

    def close(self) -> None:
        if self._c:
            rsp.rsp_cheby_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def cheby_coefficients(degree: int, lmin: float, lmax: float):
    """(c0, a, b) of the polynomial in fp64, before the rounding to its type:
    a[j - 1], b[j - 1] belong to term j = 1 .. degree - 1
    (rsp_cheby_coefficients_host; no device needed)."""
    c0 = C.c_double()
    a, b = np.zeros(max(int(degree) - 1, 1)), np.zeros(max(int(degree) - 1, 1))
    dp = C.POINTER(C.c_double)
    check(rsp.rsp_cheby_coefficients_host(int(degree), float(lmin), float(lmax), C.byref(c0),
                                          a.ctypes.data_as(dp), b.ctypes.data_as(dp)),
          "rsp_cheby_coefficients_host")
    return c0.value, a[:int(degree) - 1], b[:int(degree) - 1]


def _precond_args(ilu, factor, cheby):
    """The checks the solvers share on ilu= / factor= / cheby=."""
    if cheby is not None and (ilu is not None or factor is not None):
        raise ValueError("cheby= and ilu= / factor= exclude each other")
    if ilu is not None and factor is None:
        raise ValueError("an ILU(0) preconditioner needs its factored values")


class SolveResult:
    """What BiCGStab.solve, CG.solve and GMRES.solve return: x (the solution tensor), iters, relres
    (recurrence ||r|| / ||b|| at the last check), reason (_lib.SOLVE_*) and
    history (relres after each checked iteration). Refine.solve: iters is the
    sum of the inner solves' iterations, steps the accepted corrections, relres
    the true ||b - A x|| / ||b|| of x, history its value at every step (a
    rejected one included) and inner_history, as long, the inner iterations
    that produced each step's x (None for the other solvers, as steps is)."""

    __slots__ = ("x", "iters", "relres", "reason", "history", "steps", "inner_history")

    def __init__(self, x, iters, relres, reason, history, steps=None, inner_history=None):
        self.x, self.iters, self.relres, self.reason, self.history = x, iters, relres, reason, history
        self.steps, self.inner_history = steps, inner_history

    @property
    def converged(self) -> bool:
        return self.reason == _lib.SOLVE_CONVERGED

    def __repr__(self) -> str:
        return (f"SolveResult(iters={self.iters}, relres={self.relres:.3e}, "
                f"reason={self.reason}, n={self.x.numel()})")


class BiCGStab:
    """Right-preconditioned BiCGStab on A (rsp_bicgstab_*), M = L U from the
    ILU(0) `factor` values of `ilu` (analysed, factored by the caller), or
    M = I without `ilu`. A's dtype is the iteration type; factor's dtype (the
    preconditioner type) must not be wider. A, ilu and factor are kept alive.
    cheby= (a Cheby on A, or on a float32 SpMat of the same pattern) uses that
    polynomial as M^-1 instead; it excludes ilu= and factor=."""

    CONVERGED, MAX_ITERS, BREAKDOWN = _lib.SOLVE_CONVERGED, _lib.SOLVE_MAX_ITERS, _lib.SOLVE_BREAKDOWN

    def __init__(self, handle: Handle, A: SpMat, ilu: Ilu0 | None = None,
                 factor: torch.Tensor | None = None, cheby: Cheby | None = None):
        _precond_args(ilu, factor, cheby)
        if factor is not None and factor.dtype not in _DT:
            raise TypeError("factor must be float64 or float32")
        self.handle, self.A, self.ilu, self.factor, self.cheby = handle, A, ilu, factor, cheby
        self.dtype = A.dtype
        self._s = C.c_void_p()
        if cheby is not None:
            check(rsp.rsp_bicgstab_create_cheby(handle.ptr, A._mat, cheby._c, C.byref(self._s)),
                  "rsp_bicgstab_create_cheby")
            return
        check(rsp.rsp_bicgstab_create(handle.ptr, A._mat, ilu._info if ilu is not None else None,
                                      _DT[factor.dtype] if ilu is not None else _DT[A.dtype],
                                      _ptr(factor) if ilu is not None else None, C.byref(self._s)),
              "rsp_bicgstab_create")

    def solve(self, b: torch.Tensor, x0: torch.Tensor | None = None, rtol: float = 1e-10,
              max_iters: int = 1000, check_every: int = 1) -> SolveResult:
        """Solve A x = b from x0 (default 0); x0 is not modified."""
        if b.dtype != self.dtype or b.numel() != self.A.m:
            raise ValueError("b has the wrong dtype or length")
        if x0 is not None and (x0.dtype != self.dtype or x0.numel() != self.A.m):
            raise ValueError("x0 has the wrong dtype or length")
        with torch.cuda.stream(self.handle.stream):
            x = torch.zeros_like(b) if x0 is None else x0.clone()
        iters, reason, rel = C.c_int(), C.c_int(), C.c_double()
        check(rsp.rsp_bicgstab_solve(self.handle.ptr, self._s, _ptr(b), _ptr(x), float(rtol),
                                     int(max_iters), int(check_every), C.byref(iters), C.byref(rel),
                                     C.byref(reason)), "rsp_bicgstab_solve")
        count = C.c_int()
        check(rsp.rsp_bicgstab_history(self._s, 0, None, C.byref(count)), "rsp_bicgstab_history")
        hist = (C.c_double * max(count.value, 1))()
        check(rsp.rsp_bicgstab_history(self._s, count.value, hist, C.byref(count)), "rsp_bicgstab_history")
        return SolveResult(x, iters.value, rel.value, reason.value, list(hist[:count.value]))

    def close(self) -> None:
        if self._s:
            rsp.rsp_bicgstab_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class CG:
    """Preconditioned conjugate gradients on a symmetric positive definite A
    (rsp_cg_*); the arguments are BiCGStab's. A's symmetry is not verified: an
    A or M that is not positive definite ends in BREAKDOWN. Memory: 4 vectors
    of A's dtype (3 without `ilu`)."""

    CONVERGED, MAX_ITERS, BREAKDOWN = _lib.SOLVE_CONVERGED, _lib.SOLVE_MAX_ITERS, _lib.SOLVE_BREAKDOWN

    def __init__(self, handle: Handle, A: SpMat, ilu: Ilu0 | None = None,
                 factor: torch.Tensor | None = None, cheby: Cheby | None = None):
        _precond_args(ilu, factor, cheby)
        if factor is not None and factor.dtype not in _DT:
            raise TypeError("factor must be float64 or float32")
        self.handle, self.A, self.ilu, self.factor, self.cheby = handle, A, ilu, factor, cheby
        self.dtype = A.dtype
        self._s = C.c_void_p()
        if cheby is not None:
            check(rsp.rsp_cg_create_cheby(handle.ptr, A._mat, cheby._c, C.byref(self._s)),
                  "rsp_cg_create_cheby")
            return
        check(rsp.rsp_cg_create(handle.ptr, A._mat, ilu._info if ilu is not None else None,
                                _DT[factor.dtype] if ilu is not None else _DT[A.dtype],
                                _ptr(factor) if ilu is not None else None, C.byref(self._s)),
              "rsp_cg_create")

    def solve(self, b: torch.Tensor, x0: torch.Tensor | None = None, rtol: float = 1e-10,
              max_iters: int = 1000, check_every: int = 1) -> SolveResult:
        """Solve A x = b from x0 (default 0); x0 is not modified."""
        if b.dtype != self.dtype or b.numel() != self.A.m:
            raise ValueError("b has the wrong dtype or length")
        if x0 is not None and (x0.dtype != self.dtype or x0.numel() != self.A.m):
            raise ValueError("x0 has the wrong dtype or length")
        with torch.cuda.stream(self.handle.stream):
            x = torch.zeros_like(b) if x0 is None else x0.clone()
        iters, reason, rel = C.c_int(), C.c_int(), C.c_double()
        check(rsp.rsp_cg_solve(self.handle.ptr, self._s, _ptr(b), _ptr(x), float(rtol), int(max_iters),
                               int(check_every), C.byref(iters), C.byref(rel), C.byref(reason)),
              "rsp_cg_solve")
        count = C.c_int()
        check(rsp.rsp_cg_history(self._s, 0, None, C.byref(count)), "rsp_cg_history")
        hist = (C.c_double * max(count.value, 1))()
        check(rsp.rsp_cg_history(self._s, count.value, hist, C.byref(count)), "rsp_cg_history")
        return SolveResult(x, iters.value, rel.value, reason.value, list(hist[:count.value]))

    def close(self) -> None:
        if self._s:
            rsp.rsp_cg_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class GMRES:
    """Restarted right-preconditioned flexible GMRES(restart) on A
    (rsp_gmres_*); the arguments are BiCGStab's, plus the restart length
    (1 .. _lib.GMRES_MAX_RESTART). Memory: 2 restart + 2 vectors of A's dtype."""

    CONVERGED, MAX_ITERS, BREAKDOWN = _lib.SOLVE_CONVERGED, _lib.SOLVE_MAX_ITERS, _lib.SOLVE_BREAKDOWN

    def __init__(self, handle: Handle, A: SpMat, ilu: Ilu0 | None = None,
                 factor: torch.Tensor | None = None, restart: int = 30, cheby: Cheby | None = None):
        _precond_args(ilu, factor, cheby)
        if factor is not None and factor.dtype not in _DT:
            raise TypeError("factor must be float64 or float32")
        self.handle, self.A, self.ilu, self.factor, self.cheby = handle, A, ilu, factor, cheby
        self.dtype = A.dtype
        self.restart = int(restart)
        self._s = C.c_void_p()
        if cheby is not None:
            check(rsp.rsp_gmres_create_cheby(handle.ptr, A._mat, cheby._c, self.restart, C.byref(self._s)),
                  "rsp_gmres_create_cheby")
            return
        check(rsp.rsp_gmres_create(handle.ptr, A._mat, ilu._info if ilu is not None else None,
                                   _DT[factor.dtype] if ilu is not None else _DT[A.dtype],
                                   _ptr(factor) if ilu is not None else None, self.restart,
                                   C.byref(self._s)), "rsp_gmres_create")

    def solve(self, b: torch.Tensor, x0: torch.Tensor | None = None, rtol: float = 1e-10,
              max_iters: int = 1000, check_every: int = 1) -> SolveResult:
        """Solve A x = b from x0 (default 0); x0 is not modified. history
        holds the value of every check: the estimate inside a cycle, the
        recomputed ||b - A x|| / ||b|| at a cycle's end."""
        if b.dtype != self.dtype or b.numel() != self.A.m:
            raise ValueError("b has the wrong dtype or length")
        if x0 is not None and (x0.dtype != self.dtype or x0.numel() != self.A.m):
            raise ValueError("x0 has the wrong dtype or length")
        with torch.cuda.stream(self.handle.stream):
            x = torch.zeros_like(b) if x0 is None else x0.clone()
        iters, reason, rel = C.c_int(), C.c_int(), C.c_double()
        check(rsp.rsp_gmres_solve(self.handle.ptr, self._s, _ptr(b), _ptr(x), float(rtol), int(max_iters),
                                  int(check_every), C.byref(iters), C.byref(rel), C.byref(reason)),
              "rsp_gmres_solve")
        count = C.c_int()
        check(rsp.rsp_gmres_history(self._s, 0, None, C.byref(count)), "rsp_gmres_history")
        hist = (C.c_double * max(count.value, 1))()
        check(rsp.rsp_gmres_history(self._s, count.value, hist, C.byref(count)), "rsp_gmres_history")
        return SolveResult(x, iters.value, rel.value, reason.value, list(hist[:count.value]))

    def close(self) -> None:
        if self._s:
            rsp.rsp_gmres_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class Refine:
    """Mixed-precision iterative refinement (rsp_refine_*): fp64 residual and
    update around an all-fp32 inner solve of A_low d = r by `method`
    ("bicgstab", "cg" or "gmres" with `restart`). A is the fp64 matrix, A_low an
    fp32 SpMat over the same pattern (values narrowed, e.g. by convert_scaled);
    `ilu` (analysed) with its fp32 `factor_low` is the inner preconditioner, or
    M = I without; cheby= (a Cheby built on A_low) uses that polynomial instead.
    A, A_low, ilu and factor_low are kept alive."""

    CONVERGED, MAX_ITERS, BREAKDOWN = _lib.SOLVE_CONVERGED, _lib.SOLVE_MAX_ITERS, _lib.SOLVE_BREAKDOWN
    STAGNATED = _lib.SOLVE_STAGNATED
    METHODS = {"bicgstab": _lib.REFINE_BICGSTAB, "cg": _lib.REFINE_CG, "gmres": _lib.REFINE_GMRES}

    def __init__(self, handle: Handle, A: SpMat, A_low: SpMat, ilu: Ilu0 | None = None,
                 factor_low: torch.Tensor | None = None, method: str = "gmres", restart: int = 30,
                 cheby: Cheby | None = None):
        if method not in self.METHODS:
            raise ValueError("method is bicgstab, cg or gmres")
        _precond_args(ilu, factor_low, cheby)
        if factor_low is not None and factor_low.dtype != torch.float32:
            raise TypeError("factor_low must be float32")
        self.handle, self.A, self.A_low, self.ilu, self.factor_low = handle, A, A_low, ilu, factor_low
        self.cheby = cheby
        self.method, self.restart = method, int(restart)
        self._s = C.c_void_p()
        if cheby is not None:
            check(rsp.rsp_refine_create_cheby(handle.ptr, A._mat, A_low._mat, cheby._c, self.METHODS[method],
                                              self.restart, C.byref(self._s)), "rsp_refine_create_cheby")
            return
        check(rsp.rsp_refine_create(handle.ptr, A._mat, A_low._mat, ilu._info if ilu is not None else None,
                                    _ptr(factor_low) if ilu is not None else None, self.METHODS[method],
                                    self.restart, C.byref(self._s)), "rsp_refine_create")

    def solve(self, b: torch.Tensor, x0: torch.Tensor | None = None, rtol: float = 1e-10, max_steps: int = 20,
              inner_rtol: float = 1e-4, inner_max_iters: int = 1000, check_every: int = 1) -> SolveResult:
        """Solve A x = b from x0 (default 0) in fp64; x0 is not modified."""
        if b.dtype != torch.float64 or b.numel() != self.A.m:
            raise ValueError("b has the wrong dtype or length")
        if x0 is not None and (x0.dtype != torch.float64 or x0.numel() != self.A.m):
            raise ValueError("x0 has the wrong dtype or length")
        with torch.cuda.stream(self.handle.stream):
            x = torch.zeros_like(b) if x0 is None else x0.clone()
        steps, inner, reason, rel = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        check(rsp.rsp_refine_solve(self.handle.ptr, self._s, _ptr(b), _ptr(x), float(rtol), int(max_steps),
                                   float(inner_rtol), int(inner_max_iters), int(check_every), C.byref(steps),
                                   C.byref(inner), C.byref(rel), C.byref(reason)), "rsp_refine_solve")
        count = C.c_int()
        check(rsp.rsp_refine_history(self._s, 0, None, None, C.byref(count)), "rsp_refine_history")
        hist = (C.c_double * max(count.value, 1))()
        its = (C.c_int * max(count.value, 1))()
        check(rsp.rsp_refine_history(self._s, count.value, hist, its, C.byref(count)), "rsp_refine_history")
        return SolveResult(x, inner.value, rel.value, reason.value, list(hist[:count.value]), steps.value,
                           list(its[:count.value]))

    def close(self) -> None:
        if self._s:
            rsp.rsp_refine_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def convert_scaled(handle: Handle, src: torch.Tensor, dst: torch.Tensor | None = None, exp2: int = 0,
                   dtype: torch.dtype | None = None) -> torch.Tensor:
    """dst = dst.dtype(src * 2^exp2), the product in fp64 and one rounding
    (rsp_convert_scaled); dst defaults to a new tensor of `dtype` (default
    float32). dst may be src itself."""
    if dst is None:
        dst = torch.empty(src.numel(), dtype=dtype or torch.float32, device=src.device)
    if src.dtype not in _DT or dst.dtype not in _DT or dst.numel() < src.numel():
        raise ValueError("convert_scaled: float64 / float32 tensors, dst at least as long as src")
    check(rsp.rsp_convert_scaled(handle.ptr, src.numel(), _DT[src.dtype], _ptr(src), int(exp2), _DT[dst.dtype],
                                 _ptr(dst)), "rsp_convert_scaled")
    return dst


def refine_update(handle: Handle, d: torch.Tensor, x: torch.Tensor, exp2: int = 0,
                  x_old: torch.Tensor | None = None) -> torch.Tensor:
    """x_old = x (if given), then x += 2^exp2 * double(d) in place
    (rsp_refine_update); d float32, x and x_old float64."""
    if d.dtype != torch.float32 or x.dtype != torch.float64 or x.numel() != d.numel():
        raise ValueError("refine_update: d float32 and x float64 of one length")
    if x_old is not None and (x_old.dtype != torch.float64 or x_old.numel() < x.numel()):
        raise ValueError("refine_update: x_old float64, as long as x")
    check(rsp.rsp_refine_update(handle.ptr, x.numel(), _ptr(d), int(exp2), _ptr(x), _ptr(x_old)),
          "rsp_refine_update")
    return x


def dot(handle: Handle, x: torch.Tensor, y: torch.Tensor) -> float:
    """sum x_i y_i in fp64, in an order fixed by the length (rsp_dot)."""
    if x.dtype != y.dtype or x.dtype not in _DT or x.numel() != y.numel():
        raise ValueError("dot: x and y must share dtype (float64 / float32) and length")
    r = C.c_double()
    check(rsp.rsp_dot(handle.ptr, _DT[x.dtype], x.numel(), C.c_void_p(x.data_ptr()),
                      C.c_void_p(y.data_ptr()), C.byref(r)), "rsp_dot")
    return r.value


def orthogonalize(handle: Handle, V: torch.Tensor, w: torch.Tensor) -> np.ndarray:
    """One Gram-Schmidt step of GMRES, applied twice (rsp_orthogonalize): V is
    (k, n) with unit-stride rows, the k basis vectors (row stride >= n); w (n)
    is orthogonalised against them in place. Returns h (k + 1, float64): the
    summed coefficients and, last, ||w|| afterwards."""
    if V.dim() != 2 or w.dim() != 1 or V.dtype != w.dtype or V.dtype not in _DT or V.shape[1] != w.numel():
        raise ValueError("orthogonalize: V must be (k, n) and w (n,), one dtype (float64 / float32)")
    if V.shape[1] > 1 and V.stride(1) != 1:
        raise ValueError("orthogonalize: the rows of V must have unit stride")
    k, n = V.shape
    ldv = V.stride(0) if k > 1 else max(n, 1)
    h = np.zeros(k + 1)
    check(rsp.rsp_orthogonalize(handle.ptr, _DT[V.dtype], n, k, C.c_void_p(V.data_ptr()), ldv,
                                C.c_void_p(w.data_ptr()), h.ctypes.data_as(C.POINTER(C.c_double))),
          "rsp_orthogonalize")
    return h


def gather(handle: Handle, idx: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> None:
    """dst[i] = src[idx[i]] (rsp_gather; idx int64, all on the device)."""
    if idx.dtype != torch.int64 or src.dtype != dst.dtype or dst.numel() < idx.numel():
        raise ValueError("gather: bad arguments")
    check(rsp.rsp_gather(handle.ptr, _DT[src.dtype], idx.numel(), _ptr(idx), _ptr(src), _ptr(dst)),
          "rsp_gather")


def scatter(handle: Handle, idx: torch.Tensor, src: torch.Tensor, dst: torch.Tensor) -> None:
    """dst[idx[i]] = src[i] (rsp_scatter; idx int64 without duplicates)."""
    if idx.dtype != torch.int64 or src.dtype != dst.dtype or src.numel() < idx.numel():
        raise ValueError("scatter: bad arguments")
    check(rsp.rsp_scatter(handle.ptr, _DT[src.dtype], idx.numel(), _ptr(idx), _ptr(src), _ptr(dst)),
          "rsp_scatter")


def csr2csc(handle: Handle, rowptr: torch.Tensor, colidx: torch.Tensor, values: torch.Tensor | None,
            n_cols: int):
    """The CSR arrays (rowptr, colidx, values) of A^T — A's CSC form — as three
    new device tensors, in the order SpMat.spmv(transpose=True) uses
    (rsp_csr2csc; host-blocking). values=None: the pattern only, and None is
    returned for the values."""
    if rowptr.dtype != torch.int32 or colidx.dtype != torch.int32:
        raise TypeError("rowptr/colidx must be int32 (CUSPARSE_INDEX_32I)")
    if values is not None and values.dtype not in _DT:
        raise TypeError("values must be float64 or float32")
    m = rowptr.numel() - 1
    nnz = int(rowptr[-1].item()) if m > 0 else 0  # (host-blocking anyway)
    if nnz > colidx.numel() or (values is not None and nnz > values.numel()):
        raise ValueError("colidx / values are shorter than the pattern")
    t_rp = torch.empty(int(n_cols) + 1, dtype=torch.int32, device=rowptr.device)
    t_ci = torch.empty(nnz, dtype=torch.int32, device=rowptr.device)
    t_va = None if values is None else torch.empty(nnz, dtype=values.dtype, device=rowptr.device)
    check(rsp.rsp_csr2csc(handle.ptr, m, int(n_cols), colidx.numel(), _ptr(rowptr), _ptr(colidx), _ptr(values),
                          _DT[values.dtype] if values is not None else _lib.R_64F, _ptr(t_rp), _ptr(t_ci),
                          _ptr(t_va)), "rsp_csr2csc")
    return t_rp, t_ci, t_va


def csr_transpose_host(rowptr, colidx, n_cols: int):
    """(t_rowptr, t_colidx, perm) of a HOST pattern (rsp_csr_transpose_host; no
    device needed): the CSR pattern of A^T and, for each of its entries, the
    index of the entry of A it is."""
    rp = np.ascontiguousarray(rowptr, np.int32)
    ci = np.ascontiguousarray(colidx, np.int32)
    m = len(rp) - 1
    nnz = max(int(rp[-1]), 0) if m > 0 else 0
    if nnz > len(ci):
        raise ValueError("colidx is shorter than the pattern")
    t_rp = np.zeros(int(n_cols) + 1, np.int32)
    t_ci, perm = np.zeros(nnz, np.int32), np.zeros(nnz, np.int32)
    check(rsp.rsp_csr_transpose_host(m, int(n_cols), rp.ctypes.data, ci.ctypes.data, t_rp.ctypes.data,
                                     t_ci.ctypes.data, perm.ctypes.data), "rsp_csr_transpose_host")
    return t_rp, t_ci, perm


__all__ = ["Handle", "SpMat", "Ilu0", "Cheby", "cheby_coefficients", "BiCGStab", "CG", "GMRES", "Refine",
           "SolveResult", "dot", "orthogonalize",
           "convert_scaled", "refine_update", "upload_csr", "gather", "scatter", "csr2csc", "csr_transpose_host",
           "RspError"]
