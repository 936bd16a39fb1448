/*
 * rsp.h — C-ABI of the MI355X (gfx950) sparse operator library `librsp.so`.
 *
 * This is the drop-in boundary for the vendor-math layer of ReSpaSol's GPU
 * drivers: every entry point below replaces one cuSPARSE call (or call family)
 * made by /root/reference/GPU/spmv.cu or /root/reference/GPU/ilu0.cu, with the
 * same argument meaning, the same lifecycle (create -> bufferSize ->
 * analysis -> compute -> zeroPivot -> destroy) and status codes numbered like
 * cusparseStatus_t so that the drivers' error printing is unchanged.
 *
 * Conventions
 *   - Plain C types only: device pointers are `void*`/typed pointers obtained
 *     from hipMalloc (or any HIP allocator), sizes are int64_t / size_t, the
 *     stream is an opaque `void*` holding a hipStream_t (NULL = default stream).
 *   - CSR with int32 row offsets / column indices, index base 0 (the only form
 *     the reference uses: GPU/spmv.cu:132-151, GPU/ilu0.cu:122-126).
 *   - alpha / beta are HOST pointers of the compute type (cuSPARSE default
 *     pointer mode, GPU/spmv.cu:61-62,77-78).
 *   - Every call is stream-ordered on the handle's stream; only the calls
 *     marked "host-blocking" synchronise (as their cuSPARSE counterparts do).
 *   - No call aborts or exits: failures return a status code.
 *
 * Precision: RSP_R_64F / RSP_R_32F select fp64 or fp32 storage AND
 * accumulation (GPU/spmv.cu:131-162 with and without `#define FLOAT`).
 * Flush-to-zero is an EXTENSION, not reference parity: the reference's nvcc
 * flag is commented out (`CFLAGS = -arch=sm_70 -O3  #-ftz=true`,
 * GPU/Makefile:5) and would not reach cuSPARSE's precompiled kernels anyway.
 * It is a handle mode here (rsp_set_ftz) selecting kernels compiled with fp32
 * denormal flushing, for the "fp32+FTZ" experiment the README describes
 * (README.md:79-80). The parity configuration is fp32 without FTZ.
 */
#ifndef RSP_H
#define RSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSP_VERSION_MAJOR 0
#define RSP_VERSION_MINOR 1

/* Numbered exactly like cusparseStatus_t (GPU/spmv.cu:24-29 prints the
 * integer), so drivers print identical codes. */
typedef enum {
    RSP_STATUS_SUCCESS = 0,
    RSP_STATUS_NOT_INITIALIZED = 1,
    RSP_STATUS_ALLOC_FAILED = 2,
    RSP_STATUS_INVALID_VALUE = 3,
    RSP_STATUS_ARCH_MISMATCH = 4,
    RSP_STATUS_EXECUTION_FAILED = 6,
    RSP_STATUS_INTERNAL_ERROR = 7,
    RSP_STATUS_MATRIX_TYPE_NOT_SUPPORTED = 8,
    RSP_STATUS_ZERO_PIVOT = 9,
    RSP_STATUS_NOT_SUPPORTED = 10
} rsp_status_t;

/* CUDA_R_64F / CUDA_R_32F (GPU/spmv.cu:135,151). */
typedef enum { RSP_R_64F = 0, RSP_R_32F = 1 } rsp_datatype_t;

/* CUSPARSE_OPERATION_NON_TRANSPOSE / _TRANSPOSE (GPU/ilu0.cu:296,300). */
typedef enum { RSP_OPERATION_NON_TRANSPOSE = 0, RSP_OPERATION_TRANSPOSE = 1 } rsp_operation_t;

typedef struct rsp_context *rsp_handle_t;       /* cusparseHandle_t       */
typedef struct rsp_spmat *rsp_spmat_t;          /* cusparseSpMatDescr_t   */
typedef struct rsp_ilu0_info *rsp_ilu0_info_t;  /* csrilu02Info_t + both csrsv2Info_t */
typedef struct rsp_spmv_batch *rsp_spmv_batch_t; /* no cuSPARSE counterpart (below) */

/* ---------------------------------------------------------------- handle */

/* cusparseCreate (GPU/spmv.cu:128, GPU/ilu0.cu:85). Binds the current HIP
 * device; fails with ARCH_MISMATCH if it is not gfx950. */
rsp_status_t rsp_create(rsp_handle_t *handle);
/* cusparseDestroy (GPU/spmv.cu:282, GPU/ilu0.cu:340). */
rsp_status_t rsp_destroy(rsp_handle_t handle);
/* cusparseSetStream. `stream` is a hipStream_t (NULL = default stream). */
rsp_status_t rsp_set_stream(rsp_handle_t handle, void *stream);
rsp_status_t rsp_get_stream(rsp_handle_t handle, void **stream);
/* Extension (the reference's `-ftz=true` at GPU/Makefile:5 is commented
 * out): fp32 kernels flush denormal inputs and results to zero when enabled.
 * fp64 is never flushed (as with nvcc -ftz). Default off = parity mode. */
rsp_status_t rsp_set_ftz(rsp_handle_t handle, int enable);
rsp_status_t rsp_get_ftz(rsp_handle_t handle, int *enable);
/* cusparseGetErrorString analogue. Never NULL. */
const char *rsp_get_error_string(rsp_status_t status);
/* Library version: major*1000 + minor. */
int rsp_get_version(void);

/* ------------------------------------------------------- CSR descriptor */

/* cusparseCreateCsr(&matA, rows, cols, nnz, offsets, columns, values,
 * CUSPARSE_INDEX_32I, CUSPARSE_INDEX_32I, CUSPARSE_INDEX_BASE_ZERO, dtype)
 * (GPU/spmv.cu:132-135,148-151). `nnz` is the caller's count; like cuSPARSE
 * the kernels use offsets[rows] (the reference passes A.nnz, which exceeds
 * offsets[rows] for symmetric inputs: SURVEY §0.3). Host-side object only. */
rsp_status_t rsp_create_csr(rsp_spmat_t *mat, int64_t rows, int64_t cols, int64_t nnz,
                            void *d_row_offsets, void *d_col_ind, void *d_values,
                            rsp_datatype_t value_type);
/* Re-point the values array (e.g. fp64 -> fp32 copy) keeping the analysis:
 * the schedule stays for the same value_type; another type re-plans on the next
 * bufferSize / preprocess / SpMV (a tile's capacity depends on the type).
 * The transposed side (rsp_spmv, op == TRANSPOSE), if built, follows suit.
 * INVALID_VALUE: a NULL mat, a value_type outside the enum. */
rsp_status_t rsp_csr_set_values(rsp_spmat_t mat, void *d_values, rsp_datatype_t value_type);
rsp_status_t rsp_destroy_spmat(rsp_spmat_t mat); /* cusparseDestroySpMat (GPU/spmv.cu:279) */

/* ------------------------------------------------------------------ SpMV */

/* cusparseSpMV_bufferSize (GPU/spmv.cu:143-145,159-161). Host-blocking: builds
 * the row-block schedule of `mat` for `compute_type` (reads the row offsets and
 * column indices once, validates them — INVALID_VALUE for a malformed
 * pattern — and keeps a 16-bit copy of the column indices, relative to each
 * tile's first column, for tiles spanning < 65536 columns) in device memory
 * owned by `mat` (freed by rsp_destroy_spmat), so that the reference's call
 * sequence create_csr -> bufferSize -> malloc -> SpMV x50 (GPU/spmv.cu:143-195)
 * plans nothing inside a timed call. *buffer_size is 0: rsp_spmv needs no
 * caller workspace (any pointer, NULL included, is accepted), and several
 * matrices may share one. The schedule is reused while it is valid; as with
 * cuSPARSE, the sparsity pattern must not change afterwards without a new
 * rsp_spmv_preprocess (values may: they are read on every call). */
rsp_status_t rsp_spmv_buffer_size(rsp_handle_t handle, rsp_operation_t op, const void *alpha,
                                  rsp_spmat_t mat, const void *beta, rsp_datatype_t compute_type,
                                  size_t *buffer_size);
/* cusparseSpMV_preprocess analogue (cuSPARSE 12; the reference has no such
 * call): rebuilds the schedule of `mat` (host-blocking, as bufferSize). Only
 * needed after the pattern changed; rsp_spmv plans lazily if neither call was
 * made. `d_buffer` is unused. */
rsp_status_t rsp_spmv_preprocess(rsp_handle_t handle, rsp_operation_t op, const void *alpha,
                                 rsp_spmat_t mat, const void *d_x, const void *beta, void *d_y,
                                 rsp_datatype_t compute_type, void *d_buffer);
/* cusparseSpMV (GPU/spmv.cu:179-186): y = alpha * op(A) * x + beta * y, op
 * NON_TRANSPOSE (the only form the reference uses) or TRANSPOSE (below). The
 * rounding is fixed: with T the compute type and s the row's products summed in the
 * canonical order (spmv.hip; oracle_spmv_canon_* of oracle/rsp_oracle.h),
 *     y = round(round(alpha * s) + round(beta * y)),
 * each round() to T: two rounded products and one rounded sum, never a fused
 * multiply-add, never a wider type, alpha applied once to the whole row's sum
 * (also for a row cut into chunks); an empty row has s = +0. If *beta == 0,
 * of either sign, y is write-only: it is not read (a NaN in it is ignored) and
 * y = round(alpha * s). rsp_spmv_part and rsp_spmv_batch_run follow the same
 * rule, so parts and batches are bit for bit equal to the single call
 * (tests/spmv_epilogue_ref.py restates it). compute_type must equal the matrix value type (here and in
 * bufferSize / preprocess / rsp_spmv_part / rsp_spmv_batch_create: INVALID_VALUE
 * otherwise, e.g. a type left over from before rsp_csr_set_values). Deterministic:
 * the same inputs give bitwise identical y on every call. `d_buffer` is
 * accepted for signature parity and unused. Calls on one matrix must be
 * stream-ordered (its long-row tickets live in its schedule).
 *
 * op == TRANSPOSE: y = alpha * A^T * x + beta * y, x of `rows` elements, y of
 * `cols` (d_x is required when rows > 0, d_y when cols > 0; INVALID_VALUE
 * otherwise). A^T is DEFINED as a CSR matrix: its row j holds the entries of
 * column j of A in storage order — ascending row of A, and within a row the
 * order they are stored in (a stable counting sort by column; duplicates and
 * unsorted rows of A are legal and keep that order) — and s is the canonical
 * order applied to that matrix. So the result is bit for bit that of op ==
 * NON_TRANSPOSE on a descriptor over the rsp_csr2csc output, of
 * oracle_spmv_canon_* on that transpose, and of itself on every repeat; no
 * atomics, nothing depends on arrival order. The epilogue rule is the one
 * above. Cost: the first bufferSize / preprocess / SpMV with op == TRANSPOSE
 * builds (host-blocking, as bufferSize) a transposed side owned by `mat`:
 * device memory of nnz * (8 + element size) + 4 * (cols + 1) bytes plus the
 * schedule of A^T, freed by rsp_destroy_spmat; and every call runs a
 * permutation pass over the values (they are read on every call, as for op ==
 * NON_TRANSPOSE) before the product, both on the handle's stream. A caller
 * whose values are static transposes once with rsp_csr2csc, creates a
 * descriptor on the result and pays neither. bufferSize(op = TRANSPOSE) builds
 * the side if absent (*buffer_size = 0), preprocess(op = TRANSPOSE) always
 * rebuilds it from the pattern as it is then; neither touches the forward
 * schedule. After rsp_csr_set_values the next call permutes the new values
 * (another type: the permuted values are reallocated and A^T re-planned by
 * that call; pattern arrays and permutation stay). rsp_spmat_set_local_cols
 * concerns the forward schedule only; rsp_spmv_part and the batch calls are
 * NON_TRANSPOSE only. A matrix never used with op == TRANSPOSE allocates
 * nothing for it. An op outside the enum: NOT_SUPPORTED (all three calls). */
rsp_status_t rsp_spmv(rsp_handle_t handle, rsp_operation_t op, const void *alpha, rsp_spmat_t mat,
                      const void *d_x, const void *beta, void *d_y, rsp_datatype_t compute_type,
                      void *d_buffer);

/* --------------------------------------------------------- ILU(0) + trsv */

/* cusparseCreateCsrilu02Info + 2x cusparseCreateCsrsv2Info (GPU/ilu0.cu:143-150). */
rsp_status_t rsp_create_ilu0_info(rsp_ilu0_info_t *info);
rsp_status_t rsp_destroy_ilu0_info(rsp_ilu0_info_t info);

/* cusparse?csrilu02_bufferSize / csrsv2_bufferSize (GPU/ilu0.cu:166-186).
 * The schedule lives in `info` (library-owned), so the external buffer size
 * is 0; kept for lifecycle parity. */
rsp_status_t rsp_ilu0_buffer_size(rsp_handle_t handle, int n, int nnz, rsp_datatype_t value_type,
                                  rsp_ilu0_info_t info, size_t *buffer_size);

/* cusparse?csrilu02_analysis (GPU/ilu0.cu:203-217, the reference's timed
 * "Symbolic"): diagonal positions, structural-zero detection, the symbolic
 * factor, level sets of the lower triangle (factor + L-solve) and of its
 * transpose (L^T-solve), and the factor plan. The two solve plans (the
 * csrsv2_analysis half, rsp_trsv_analysis below) are started on a worker
 * thread as soon as the levels exist and left running when this call
 * returns. `nnz` may exceed offsets[n] (the
 * reference passes A.nnz, GPU/ilu0.cu:166); offsets[n] is what is analysed.
 * Each row's column indices must be strictly increasing (sorted, no
 * duplicates — as csrilu02 requires); otherwise INVALID_VALUE. The reference
 * loader sorts rows but keeps duplicate entries of a file, so a file with
 * repeated coordinates is rejected here rather than factored as undefined.
 * Host-blocking (reads the pattern once). */
rsp_status_t rsp_ilu0_analysis(rsp_handle_t handle, int n, int nnz, const int *d_row_offsets,
                               const int *d_col_ind, rsp_ilu0_info_t info);

/* cusparse?csrsv2_analysis for the L (op NON_TRANSPOSE) or L^T (op
 * TRANSPOSE) solve of an analysed info (GPU/ilu0.cu:228-252, untimed there):
 * waits for the solve plans rsp_ilu0_analysis started and uploads them (the
 * first call does both kinds; later calls return at once). Optional — the
 * first solve does it if it was not called. Host-blocking. */
rsp_status_t rsp_trsv_analysis(rsp_handle_t handle, rsp_operation_t op, rsp_ilu0_info_t info);

/* cusparseXcsrilu02_zeroPivot (GPU/ilu0.cu:222,278). Host-blocking. Returns
 * RSP_STATUS_ZERO_PIVOT and *position = j (0-based) when A(j,j) is
 * structurally missing (after analysis) or U(j,j) == 0 (after the numeric
 * factorisation); the smallest such j is reported. Otherwise SUCCESS, -1. */
rsp_status_t rsp_ilu0_zero_pivot(rsp_handle_t handle, rsp_ilu0_info_t info, int *position);
/* Flow launches (one launch over a run of fat levels) take their work items by
 * start tickets (the default since round 6): a workgroup owns the items of the
 * ticket it claimed when it started, and a workgroup that has waited long
 * while some tickets are still unclaimed (their workgroups have not started:
 * another kernel holds the CUs) claims those too, so progress never depends on
 * other kernels leaving CUs free and no wait gives up in normal operation. The
 * bounded wait (RSP_ILU_FLOW_TIMEOUT_US, default 0.2 s) stays as a backstop,
 * and it is what the older static item walk (RSP_ILU_FLOW_MODE=0) needs: a
 * factor whose flow wait gave up is RECOVERED here — its input values (kept
 * by the factor call) are restored, the factor runs again without flow
 * launches, and so does every solve made after it — and the call reports as
 * usual. The buffers of the recorded calls (values, x) must then be unchanged
 * since those calls; a later recorded solve that wrote its y over one of them
 * (e.g. L: r -> z, then L^T: z -> r) makes the recovery impossible and the
 * call returns RSP_STATUS_EXECUTION_FAILED, as it does when recovery is off
 * (RSP_ILU_FLOW_RECOVER=0). About the LAST factor call only. */

/* cusparseXcsrsv2_zeroPivot (the csrsv2 infos of GPU/ilu0.cu:143-150) for
 * the solves below; which = RSP_TRSV_L (op N), RSP_TRSV_LT (op T) or
 * RSP_TRSV_U (rsp_trsv_upper). Host-blocking. Reports on the LAST solve of
 * that kind. If its flow launch gave up a wait, the solve (its x is
 * unchanged: x != y) and every solve made after it are run again without
 * flow launches first (their x and values must be unchanged, as above);
 * RSP_STATUS_EXECUTION_FAILED with RSP_ILU_FLOW_RECOVER=0 or when a later
 * recorded solve overwrote one of those inputs. For RSP_TRSV_U, ZERO_PIVOT + *position as
 * rsp_ilu0_zero_pivot (U divides by u_jj); else SUCCESS, -1. */
#define RSP_TRSV_L 0
#define RSP_TRSV_LT 1
#define RSP_TRSV_U 2
rsp_status_t rsp_trsv_zero_pivot(rsp_handle_t handle, rsp_ilu0_info_t info, int which, int *position);

/* cusparse?csrilu02 (GPU/ilu0.cu:264-268): in-place ILU(0) on the CSR
 * pattern, IKJ order: for each row i, for each k < i in the pattern
 * (ascending): a_ik /= u_kk; a_ij -= a_ik * u_kj for j > k in both rows.
 * value_type selects fp64 or fp32 arithmetic (FTZ per handle mode). Like
 * csrilu02, the factor completes after a zero pivot with IEEE inf / NaN
 * propagation (x / 0 = +-inf, inf - inf = NaN), and rsp_ilu0_zero_pivot then
 * reports the smallest row j with U(j,j) == 0, whatever the schedule. */
rsp_status_t rsp_ilu0_factor(rsp_handle_t handle, rsp_ilu0_info_t info, rsp_datatype_t value_type,
                             void *d_values);

/* cusparse?csrsv2_solve with desc_L = {LOWER, UNIT} (GPU/ilu0.cu:129-134):
 *   op == NON_TRANSPOSE: solve L   y = alpha x   (GPU/ilu0.cu:296-298)
 *   op == TRANSPOSE:     solve L^T y = alpha x   (GPU/ilu0.cu:300-302)
 * where L is the unit-diagonal strictly-lower part of `d_values` on the
 * analysed pattern. x and y must not alias. */
rsp_status_t rsp_trsv_lower_unit(rsp_handle_t handle, rsp_operation_t op, const void *alpha,
                                 rsp_ilu0_info_t info, rsp_datatype_t value_type,
                                 const void *d_values, const void *d_x, void *d_y);

/* Extension (off by default): solve with the upper factor
 * U (non-unit diagonal, upper part incl. diagonal), i.e. the true ILU(0)
 * apply that the reference's unused desc_U describes (GPU/ilu0.cu:136-141). */
rsp_status_t rsp_trsv_upper(rsp_handle_t handle, const void *alpha, rsp_ilu0_info_t info,
                            rsp_datatype_t value_type, const void *d_values, const void *d_x,
                            void *d_y);

/* --------------------------------- ILU(0)-preconditioned BiCGStab, dot */

/* No single cuSPARSE call: this is the loop the csrilu02 + csrsv2 + SpMV call
 * set is normally used in (an ILU-preconditioned Krylov solver), with the
 * cuBLAS level-1 calls of that loop (cublasDdot / Daxpy / Dscal, and the
 * cudaMemcpy of each scalar) replaced by fused kernels whose scalars stay on
 * the device. Right-preconditioned BiCGStab, M = L U: L the unit lower part
 * (rsp_trsv_lower_unit, op N), U the upper part with the diagonal
 * (rsp_trsv_upper) of the factored values — the true ILU(0) apply, not the
 * L L^T of GPU/ilu0.cu:296-302. Per iteration: two rsp_spmv, four triangular
 * solves (alpha = 1, beta = 0) and five kernels of the solver's own (seven
 * with a narrower preconditioner: its fp32 result is widened for the fp64
 * SpMV). Deterministic: every dot product is summed in an order fixed by n,
 * so equal inputs give bitwise equal x, iteration counts and histories. */
typedef struct rsp_bicgstab *rsp_bicgstab_t;
typedef enum { RSP_SOLVE_CONVERGED = 0, RSP_SOLVE_MAX_ITERS = 1, RSP_SOLVE_BREAKDOWN = 2 } rsp_solve_reason_t;

/* A: square CSR (rows >= 1) with a schedule or plannable; its value type is
 * the iteration type T (fp64 or fp32). info: an analysed ILU(0) info of A's
 * pattern, or NULL = no preconditioner (M = I; precond_type and d_factor are
 * then ignored). d_factor: the factored values (rsp_ilu0_factor output) in
 * precond_type, which must not be wider than T; with fp32 under rsp_set_ftz(1)
 * this is the fp32+FTZ preconditioner. Host-blocking: finishes the L and U
 * solve plans and allocates all work vectors here, so solve plans and
 * allocates nothing. A, info and d_factor must outlive the solver.
 * INVALID_VALUE: a NULL argument, a non-square A, an un-analysed info,
 * info's n != rows, precond_type wider than T. ZERO_PIVOT: rsp_ilu0_zero_pivot
 * of info reports one (U divides by its diagonal). */
rsp_status_t rsp_bicgstab_create(rsp_handle_t handle, rsp_spmat_t A, rsp_ilu0_info_t info,
                                 rsp_datatype_t precond_type, const void *d_factor, rsp_bicgstab_t *s);
/* Solves A x = b. d_x: in = x0, out = the solution; d_b, d_x of type T, n
 * elements, any 8-byte-aligned pointers. Stops when the recurrence residual
 * meets ||r||_2 <= rtol ||b||_2 (rtol = 0: run max_iters), tested on the host
 * every check_every iterations (>= 1; one asynchronous copy into pinned memory
 * and one event wait — the only host wait of the loop) and after the last;
 * check_every changes no bit of x for a given iteration count. Host-blocking.
 * SUCCESS for all three reasons: *iters = iterations completed, *relres =
 * ||r|| / ||b|| of the recurrence residual at the last check.
 *   - b = 0: x = 0, 0 iterations, CONVERGED; an x0 that already meets rtol:
 *     0 iterations, x untouched.
 *   - BREAKDOWN: an iteration would have divided by a zero or non-finite rho,
 *     omega, (rhat,v) or (t,t) (or b / x0 are not finite). Detected on the
 *     device; x keeps the value of the last completed iteration, no NaN
 *     reaches it. (t,t) == 0 exactly is the exact half step (s = 0): it is
 *     taken with omega = 0 and is no breakdown.
 * INVALID_VALUE: a NULL argument, max_iters < 0, check_every < 1, rtol < 0.
 * EXECUTION_FAILED: cusparseXcsrsv2_zeroPivot's report for the L and U solves
 * of this call, read once after the loop: a flow launch of one of them gave
 * up a wait. The solver reuses its buffers every iteration, so the give-up
 * recovery of rsp_trsv_zero_pivot (which re-runs recorded solves from their
 * unchanged inputs) cannot apply here; x is then not a solution. */
rsp_status_t rsp_bicgstab_solve(rsp_handle_t handle, rsp_bicgstab_t s, const void *d_b, void *d_x,
                                double rtol, int max_iters, int check_every,
                                int *iters, double *relres, rsp_solve_reason_t *reason);
/* Relative residual after each checked iteration of the last solve: *count =
 * how many there are, the first min(cap, *count) are written to relres. */
rsp_status_t rsp_bicgstab_history(rsp_bicgstab_t s, int cap, double *relres, int *count);
rsp_status_t rsp_bicgstab_destroy(rsp_bicgstab_t s);
/* cublasDdot analogue on the solver's reduction: *result (HOST, fp64) =
 * sum x_i y_i, products and sums in fp64 whatever value_type, in an order
 * fixed by n (bitwise repeatable). Host-blocking. */
rsp_status_t rsp_dot(rsp_handle_t handle, rsp_datatype_t value_type, int64_t n, const void *d_x,
                     const void *d_y, double *result);

/* ------------------- preconditioned conjugate gradients (CG), for SPD systems
 *
 * For a symmetric positive definite A, with M = L U as in rsp_bicgstab_* (or
 * M = I). T is the iteration type (A's value type), P <= T the preconditioner
 * type. A's symmetry is not verified: the caller is trusted, and a matrix or
 * preconditioner that is not positive definite ends in BREAKDOWN.
 *
 *   set-up:  r = b - A x0
 *   it = 1, 2, ...:
 *       z = M^-1 r                        (M = I: z is r, nothing is copied)
 *       rho' = (r,z)                      BREAKDOWN if rho' <= 0 or not finite
 *       p = z               if it == 1
 *       p = z + T(beta) p   otherwise     beta = rho'/rho in fp64, rounded to T once
 *       q = A p
 *       alpha = rho'/(p,q) in fp64        BREAKDOWN if (p,q) <= 0 or not finite
 *       x = x + T(alpha) p;  r = r - T(alpha) q
 *
 * The plain (Fletcher-Reeves) beta: the Polak-Ribiere form costs one more
 * vector and dot and recovers none of the iterations an fp32 preconditioner
 * adds. All dots are fp64 whatever T; vectors are stored in T.
 * Per iteration: one rsp_spmv, two triangular solves and four kernels of the
 * solver's own (five with a narrower preconditioner: the widening of its
 * result; three and no solve when M = I); the scalars stay on the device.
 * Memory: 4 vectors of T (3 when M = I) plus the apply's buffers.
 * Deterministic as rsp_bicgstab_*. */
typedef struct rsp_cg *rsp_cg_t;
/* As rsp_bicgstab_create: the same arguments, checks and statuses (ZERO_PIVOT
 * included). All vectors are allocated here. */
rsp_status_t rsp_cg_create(rsp_handle_t handle, rsp_spmat_t A, rsp_ilu0_info_t info,
                           rsp_datatype_t precond_type, const void *d_factor, rsp_cg_t *s);
/* Solves A x = b; arguments, the stopping test, the checks, INVALID_VALUE and
 * EXECUTION_FAILED as rsp_bicgstab_solve. *relres = ||r|| / ||b|| of the
 * recurrence residual at the last check; check_every changes no bit of x for
 * a given iteration count.
 *   - b = 0, an x0 inside rtol, a non-finite b / x0: as rsp_bicgstab_solve.
 *   - BREAKDOWN: (r,z) or (p,q) was <= 0 or not finite (M or A is not positive
 *     definite), detected on the device before the iteration wrote x or r:
 *     they keep the values of the last completed iteration, *iters counts
 *     those, no NaN reaches x.
 *   - r == 0 exactly is CONVERGED (also at rtol = 0), at the first check that
 *     sees it, with *iters = the iteration that reached it. */
rsp_status_t rsp_cg_solve(rsp_handle_t handle, rsp_cg_t s, const void *d_b, void *d_x, double rtol,
                          int max_iters, int check_every, int *iters, double *relres,
                          rsp_solve_reason_t *reason);
/* The value of each check of the last solve, as rsp_bicgstab_history. */
rsp_status_t rsp_cg_history(rsp_cg_t s, int cap, double *relres, int *count);
rsp_status_t rsp_cg_destroy(rsp_cg_t s);

/* -------------------------------------- restarted flexible GMRES(m) (FGMRES)
 *
 * The second Krylov method on the same operator set: right-preconditioned
 * flexible GMRES with restart m, M = L U as in rsp_bicgstab_* (or M = I). T is
 * the iteration type (A's value type), P <= T the preconditioner type.
 *
 *   bn = ||b||;  r = b - A x;  beta = ||r||      (each cycle starts from the recomputed residual)
 *   cycle:  v_0 = r / beta;  g = (beta, 0, ..)
 *     for j = 0 .. m-1:
 *         z_j = M^-1 v_j;  w = A z_j
 *         h  = V_j^T w;  w -= V_j h               (V_j = [v_0 .. v_j]; classical Gram-Schmidt,
 *         h' = V_j^T w;  w -= V_j h';  h += h'     done twice)
 *         h_{j+1,j} = ||w||
 *         the j earlier Givens rotations on column j, rotation j, g rotated;  est = |g_{j+1}| / bn
 *         if h_{j+1,j} != 0:  v_{j+1} = w / h_{j+1,j}
 *     R y = g over the k completed columns;  x += Z_k y   (Z = V when M = I)
 *     r = b - A x;  beta = ||r||;  next cycle unless stopped
 *
 * Flexible: z_j is kept, so x += Z y is exact for whatever M^-1 v_j came out
 * of a narrower preconditioner (plain GMRES forms M^-1 (V y), which is not
 * sum y_j M^-1 v_j once M^-1 rounds to fp32, and stalls near 1e-7 ||b||).
 * All dots, norms, the Hessenberg column, the rotations and y are fp64
 * whatever T; vectors are stored in T. Per iteration: one rsp_spmv, two
 * triangular solves and four kernels of the solver's own (five with a narrower
 * preconditioner: the widening of its result); the scalars stay on the device.
 * Memory: 2 m + 2 vectors of T (m + 2 when M = I) plus the apply's buffers.
 * Deterministic as rsp_bicgstab_*. */
#define RSP_GMRES_MAX_RESTART 64
typedef struct rsp_gmres *rsp_gmres_t;
/* As rsp_bicgstab_create (same arguments, checks and statuses), with the
 * restart length: INVALID_VALUE outside [1, RSP_GMRES_MAX_RESTART]. All
 * vectors are allocated here. */
rsp_status_t rsp_gmres_create(rsp_handle_t handle, rsp_spmat_t A, rsp_ilu0_info_t info,
                              rsp_datatype_t precond_type, const void *d_factor, int restart,
                              rsp_gmres_t *s);
/* Solves A x = b; arguments, INVALID_VALUE and EXECUTION_FAILED as
 * rsp_bicgstab_solve. A check is one asynchronous copy into pinned memory and
 * one event wait, made every check_every iterations (its value: est), at
 * every cycle end and after the last iteration (its value: the recomputed
 * ||b - A x|| / ||b||). Stops when est <= rtol at a check (x += Z y follows;
 * no further residual is computed), or when a cycle's recomputed residual
 * meets rtol. *relres = the value of the last check; check_every changes no
 * bit of x for a given iteration count.
 *   - b = 0, an x0 inside rtol, a non-finite b / x0: as rsp_bicgstab_solve.
 *   - BREAKDOWN: a non-finite h, or a rotated diagonal that is 0 or not finite
 *     (A is singular on the Krylov space), detected on the device: x receives
 *     the update of the completed iterations only, *iters counts those, no NaN
 *     reaches x. h_{j+1,j} = 0 with a non-zero rotated diagonal is the exact
 *     solve: it ends the cycle and is no breakdown. */
rsp_status_t rsp_gmres_solve(rsp_handle_t handle, rsp_gmres_t s, const void *d_b, void *d_x, double rtol,
                             int max_iters, int check_every, int *iters, double *relres,
                             rsp_solve_reason_t *reason);
/* The value of each check of the last solve, as rsp_bicgstab_history. */
rsp_status_t rsp_gmres_history(rsp_gmres_t s, int cap, double *relres, int *count);
rsp_status_t rsp_gmres_destroy(rsp_gmres_t s);
/* One Gram-Schmidt step of the solver on its own, by the solver's three
 * kernels: d_V holds k columns of n elements, ldv >= n elements apart
 * (1 <= k <= RSP_GMRES_MAX_RESTART), orthonormal or nearly so; d_w (n
 * elements) is orthogonalised against them in place, twice. h (HOST, k + 1):
 * h[0..k) the summed coefficients of both passes, h[k] = ||w|| on return.
 * Host-blocking; n = 0 gives h = 0. INVALID_VALUE: k outside the range,
 * ldv < n, n < 0, a NULL pointer. */
rsp_status_t rsp_orthogonalize(rsp_handle_t handle, rsp_datatype_t value_type, int64_t n, int k,
                               const void *d_V, int64_t ldv, void *d_w, double *h);
/* Tests (no device needed): the solver's small least-squares step on HOST
 * arrays. H: column-major (k + 1) x k upper Hessenberg, columns ldh >= k + 1
 * apart; minimises ||beta e_1 - H y|| by the solver's Givens rotations and
 * back-substitution: y (k) and est (k): |g_{j+1}| after column j.
 * INVALID_VALUE: k outside [1, RSP_GMRES_MAX_RESTART], ldh < k + 1, a NULL
 * pointer, a non-finite entry or a rotated diagonal that is 0. */
rsp_status_t rsp_gmres_lsq_host(int k, int ldh, const double *H, double beta, double *y, double *est);

/* --------------------- mixed-precision iterative refinement (rsp_refine_*)
 *
 * An fp64-accurate solution out of fp32 Krylov solves: the residual is formed
 * in fp64, the correction equation is solved entirely in fp32 (fp32 matrix,
 * fp32 vectors, fp32 ILU(0)) by one of the three solvers above, and the
 * correction is added in fp64.
 *
 *   bn = ||b||                                    b = 0: x = 0, CONVERGED, 0 steps
 *   k = 0, 1, ...
 *      v = A x;  r = b - v;  rn = ||r||           (fp64; one rsp_spmv, one kernel, one read-back)
 *      history[k] = rn / bn
 *      rn or bn not finite:        BREAKDOWN      k = 0: x untouched;  k > 0: x = x_old
 *      rn / bn <= rtol:            CONVERGED, steps = k
 *      k > 0 and rn >= rn of k-1:  x = x_old, STAGNATED, steps = k - 1, relres = history[k-1]
 *      k == max_steps:             MAX_ITERS, steps = k
 *      rn = m * 2^e, 0.5 <= m < 1
 *      r32_i = fp32(r_i * 2^-e);  d = 0           (one kernel; ||r32|| lies in [0.5, 1))
 *      inner solve  A_low d = r32  from d = 0 to inner_rtol, inner_max_iters, check_every
 *          inner BREAKDOWN before one iteration completed: BREAKDOWN, steps = k, x untouched
 *      x_old = x;  x_i = x_i + 2^e * double(d_i)  (one kernel)
 *
 * A product with a power of two is exact, so r32 is r rounded once (to nearest
 * even) and the update rounds once; the scaling lets the fp32 solve see
 * residuals far below fp32's range, also under rsp_set_ftz(1) (e is kept
 * within [-1022, 1022]). STAGNATED: a step that does not reduce ||r|| is
 * undone and ends the solve — the floor of this A, A_low and inner solve is
 * reached, and further steps would walk around it. Deterministic as
 * rsp_bicgstab_*: equal inputs give bitwise equal x, counts and history.
 * Memory: the inner solver's fp32 vectors, three fp64 and two fp32 vectors. */
#define RSP_SOLVE_STAGNATED ((rsp_solve_reason_t)3) /* the fourth rsp_solve_reason_t; only rsp_refine_solve gives it */
typedef enum { RSP_REFINE_BICGSTAB = 0, RSP_REFINE_CG = 1, RSP_REFINE_GMRES = 2 } rsp_refine_method_t;
typedef struct rsp_refine *rsp_refine_t;
/* A: square fp64 CSR (rows >= 1). A_low: an fp32 descriptor of the same size;
 * the caller makes it over the same pattern arrays with the values narrowed by
 * rsp_convert_scaled(exp2 = 0). info / d_factor_low: an analysed ILU(0) info of
 * the pattern and its fp32 factor, or info = NULL for M = I. The inner solver
 * is rsp_<method>_create(handle, A_low, info, RSP_R_32F, d_factor_low[,
 * restart]); its statuses pass through, ZERO_PIVOT included. All vectors, the
 * reduction block and its pinned mirror are allocated here. A, A_low, info and
 * the factor must outlive the solver. INVALID_VALUE: a NULL argument (info may
 * be NULL), A not fp64 or A_low not fp32, sizes that differ or are not square,
 * a method outside the enum, for RSP_REFINE_GMRES a restart outside
 * [1, RSP_GMRES_MAX_RESTART] (the other methods ignore restart). */
rsp_status_t rsp_refine_create(rsp_handle_t handle, rsp_spmat_t A, rsp_spmat_t A_low, rsp_ilu0_info_t info,
                               const void *d_factor_low, rsp_refine_method_t method, int restart,
                               rsp_refine_t *s);
/* The loop above; host-blocking. d_b, d_x: fp64, n elements; x is x0 on entry
 * and the solution on return. *steps: accepted corrections; *inner_iters: the
 * iterations of all inner solves, a rejected step's included; *relres: the
 * last accepted history value, the true fp64 residual of the returned x over
 * ||b||. max_steps = 0 computes the residual only. inner_max_iters = 0 makes
 * every correction zero: STAGNATED with 0 steps. The inner solve's set-up
 * product with d = 0 is not skipped: the inner solvers run as they are.
 * INVALID_VALUE: a NULL pointer, max_steps < 0, inner_max_iters < 0,
 * check_every < 1, a negative or NaN rtol or inner_rtol.
 * EXECUTION_FAILED: an inner solve reported it (rsp_bicgstab_solve). */
rsp_status_t rsp_refine_solve(rsp_handle_t handle, rsp_refine_t s, const void *d_b, void *d_x, double rtol,
                              int max_steps, double inner_rtol, int inner_max_iters, int check_every,
                              int *steps, int *inner_iters, double *relres, rsp_solve_reason_t *reason);
/* The last solve step by step: relres[k] = history[k] above and inner_iters[k]
 * = the iterations of the inner solve that produced x_k (0 for k = 0); a
 * rejected step's entry is included, so *count = steps + 1 or steps + 2 (0
 * after b = 0). The first min(cap, *count) entries of both are written.
 * INVALID_VALUE: s or count NULL, cap < 0, cap > 0 with an array NULL. */
rsp_status_t rsp_refine_history(rsp_refine_t s, int cap, double *relres, int *inner_iters, int *count);
rsp_status_t rsp_refine_destroy(rsp_refine_t s);
/* The refinement's building blocks on their own, as rsp_dot is the solvers'.
 * dst_i = dst_type(src_i * 2^exp2) for i < n, |exp2| <= 1022, any of the four
 * type pairs: the product is formed in fp64 (exact short of fp64's range), then
 * rounded once to dst_type, to nearest even. Overflow gives +-inf, NaN stays
 * NaN. fp32 denormals are read and written as they are; under rsp_set_ftz(1)
 * an fp32 denormal read counts as a zero of its sign and an fp32 result that is
 * denormal after rounding becomes one, as in the other fp32 kernels. Any
 * naturally aligned pointers; 16-byte aligned ones move whole groups.
 * d_src == d_dst is allowed when the types are equal. n = 0 does nothing.
 * INVALID_VALUE: n < 0, a type outside the enum, exp2 out of range, a NULL
 * pointer with n > 0, d_src == d_dst with different types. */
rsp_status_t rsp_convert_scaled(rsp_handle_t handle, int64_t n, rsp_datatype_t src_type, const void *d_src,
                                int exp2, rsp_datatype_t dst_type, void *d_dst);
/* The update of a refinement step: x_old_i = x_i, then x_i = x_i + 2^exp2 *
 * double(d_i) for i < n (|exp2| <= 1022): the product is exact, the sum is
 * rounded once. d_x_old = NULL: x is not saved; otherwise it may not be d_x.
 * INVALID_VALUE: n < 0, exp2 out of range, with n > 0 a NULL d_d or d_x or
 * d_x_old == d_x. */
rsp_status_t rsp_refine_update(rsp_handle_t handle, int64_t n, const float *d_d, int exp2, double *d_x,
                               double *d_x_old);

/* ------------------- Chebyshev polynomial preconditioner (rsp_cheby_*)
 *
 * A preconditioner made of rsp_spmv alone, beside the ILU(0) one: z = M^-1 r =
 * p_k(D^-1 A) D^-1 r, p_k the polynomial of the Chebyshev iteration on
 * [lmin, lmax] started from zero, so that 1 - x p_k(x) = T_k((theta - x) /
 * delta) / T_k(sigma) (T_k the Chebyshev polynomial). No analysis, no levels,
 * no flow launch (nothing can give up a wait), no dot product. P is the value
 * type of the matrix it is built on; dinv is the inverse diagonal
 * (RSP_CHEBY_SCALE_JACOBI) or all ones (RSP_CHEBY_SCALE_NONE: the product with
 * it is skipped). The degree k >= 1 counts terms: k - 1 rsp_spmv per apply;
 * k = 1 is the scaled Jacobi preconditioner.
 *
 * Coefficients, on the host in fp64 without fused multiply-add, in this order,
 * then rounded once to P:
 *
 *   theta = (lmax + lmin) / 2;  delta = (lmax - lmin) / 2;  sigma = theta / delta
 *   rho_0 = 1 / sigma;          c0 = 1 / theta
 *   j = 1 .. k-1:  rho_j = 1 / (2*sigma - rho_{j-1});  a_j = rho_j * rho_{j-1};  b_j = 2 * rho_j / delta
 *
 * The apply keeps r unchanged and needs r != z; d and w are work vectors of the
 * object; every product and sum is rounded to P:
 *
 *   d_i = c0 * (dinv_i * r_i);  z_i = d_i;  w_i = r_i          (k = 1: only z is written)
 *   j = 1 .. k-1:
 *       w = w - A d                      rsp_spmv(alpha = -1, A, d, beta = 1, w)
 *       t = dinv_i * w_i;  d_i = (a_j * d_i) + (b_j * t);  z_i = z_i + d_i
 *
 * The kernels between the products are element-wise, so the result is the bits
 * of that restatement over rsp_spmv's canonical order, for any alignment.
 * Per apply, in vectors of P beside the k - 1 rsp_spmv: the first kernel reads
 * 2 and writes 3, a step reads 4 and writes 2 (the last: 1); without scaling
 * one read less each.
 *
 * Set-up (one kernel): diag_i = the sum in P, in storage order, of the stored
 * entries of row i with column i (duplicates and unsorted rows are legal);
 * dinv_i = P(1) / diag_i; g_i = (sum_j |double(a_ij)| in fp64, storage order) /
 * |double(diag_i)| (NONE: / 1); lmax = max_i g_i, Gershgorin's bound on the
 * spectrum of D^-1 A, and lmin = lmax / ratio. For a symmetric positive
 * definite A the bound is guaranteed, which keeps p_k positive on the whole
 * spectrum: M is positive definite, as rsp_cg_* needs. An estimated lmax that
 * falls short makes M indefinite (CG then ends in BREAKDOWN); callers who know
 * better bounds set them. */
#define RSP_CHEBY_MAX_DEGREE 64
typedef enum { RSP_CHEBY_SCALE_NONE = 0, RSP_CHEBY_SCALE_JACOBI = 1 } rsp_cheby_scaling_t;
typedef struct rsp_cheby *rsp_cheby_t;
/* Host-blocking: plans A if needed, allocates dinv, d and w, runs the set-up.
 * *position (may be NULL) = -1, or the row ZERO_PIVOT reports. A's values and
 * pattern must not change while c lives; c must outlive every solver made on
 * it and serves one solve at a time (its work vectors are its own).
 * INVALID_VALUE: a NULL argument, a non-square A or one with no rows, a degree
 * outside [1, RSP_CHEBY_MAX_DEGREE], a scaling outside the enum, a ratio that
 * is not finite or <= 1, a bound that is not finite or <= 0. ZERO_PIVOT (JACOBI
 * only): the smallest row whose diagonal is missing, 0 or not finite. */
rsp_status_t rsp_cheby_create(rsp_handle_t handle, rsp_spmat_t A, int degree, rsp_cheby_scaling_t scaling,
                              double ratio, int *position /* may be NULL */, rsp_cheby_t *c);
rsp_status_t rsp_cheby_get_bounds(rsp_cheby_t c, double *lmin, double *lmax);
/* Recomputes the coefficients (host only; an apply already enqueued keeps the
 * old ones). INVALID_VALUE unless 0 < lmin < lmax and both are finite. */
rsp_status_t rsp_cheby_set_bounds(rsp_cheby_t c, double lmin, double lmax);
/* z = M^-1 r on the handle's stream, not host-blocking; d_r, d_z: n elements
 * of P, naturally aligned (16-byte aligned ones move whole groups). Under
 * rsp_set_ftz(1) an fp32 polynomial runs the flushing kernels.
 * INVALID_VALUE: a NULL argument, d_r == d_z. */
rsp_status_t rsp_cheby_apply(rsp_handle_t handle, rsp_cheby_t c, const void *d_r, void *d_z);
rsp_status_t rsp_cheby_destroy(rsp_cheby_t c);
/* Tests (no device needed): c0, a[degree - 1], b[degree - 1] (a[j-1] = a_j) in
 * fp64, before the rounding to P. INVALID_VALUE: the degree or the bounds as
 * above, a NULL c0, with degree > 1 a NULL a or b. */
rsp_status_t rsp_cheby_coefficients_host(int degree, double lmin, double lmax, double *c0, double *a, double *b);
/* The solvers on M = the polynomial c: as rsp_<solver>_create with c in the
 * place of info, precond_type and d_factor; solve, history and destroy are
 * unchanged. c's matrix may be A itself or a narrower descriptor over the same
 * pattern (an fp32 polynomial under an fp64 iteration: its fp32 result is
 * widened, as the fp32 ILU(0) apply's). INVALID_VALUE also for: a NULL c, P
 * wider than A's type, c's n != rows; rsp_refine_create_cheby: a c that is not
 * built on an fp32 matrix (normally A_low). */
rsp_status_t rsp_bicgstab_create_cheby(rsp_handle_t handle, rsp_spmat_t A, rsp_cheby_t c, rsp_bicgstab_t *s);
rsp_status_t rsp_cg_create_cheby(rsp_handle_t handle, rsp_spmat_t A, rsp_cheby_t c, rsp_cg_t *s);
rsp_status_t rsp_gmres_create_cheby(rsp_handle_t handle, rsp_spmat_t A, rsp_cheby_t c, int restart,
                                    rsp_gmres_t *s);
rsp_status_t rsp_refine_create_cheby(rsp_handle_t handle, rsp_spmat_t A, rsp_spmat_t A_low, rsp_cheby_t c,
                                     rsp_refine_method_t method, int restart, rsp_refine_t *s);

/* ------------------------------------------------ multi-GPU halo exchange */

/* Indexed gather dst[i] = src[idx[i]] for i < n (value_type elements). The
 * pack / unpack step of the row-partitioned SpMV's halo exchange (SURVEY
 * §8e-f): pack the x entries peers need into an RCCL send buffer, and unpack
 * the received halo into each slice's extended x. idx must be in range. */
rsp_status_t rsp_gather(rsp_handle_t handle, rsp_datatype_t value_type, int64_t n,
                        const int64_t *d_idx, const void *d_src, void *d_dst);
/* Indexed scatter dst[idx[i]] = src[i] for i < n (idx without duplicates). */
rsp_status_t rsp_scatter(rsp_handle_t handle, rsp_datatype_t value_type, int64_t n,
                         const int64_t *d_idx, const void *d_src, void *d_dst);

/* cusparseCsr2cscEx2 (CUSPARSE_ACTION_NUMERIC, index base 0): the CSC form
 * of a rows x cols CSR matrix, i.e. the CSR form of A^T: d_csc_col_offsets
 * (cols + 1), d_csc_row_ind and d_csc_values (offsets[rows] entries each), in
 * the order rsp_spmv(op = TRANSPOSE) defines and uses (the same code). `nnz`
 * is the caller's count, as in rsp_create_csr; offsets[rows] entries are
 * transposed. Host-blocking: the pattern is read once and transposed on the
 * host, the values are moved on the device as bits (a NaN payload or a
 * denormal survives in every handle mode). d_values == NULL and
 * d_csc_values == NULL: symbolic only. INVALID_VALUE: a malformed pattern (an
 * offset that is negative or decreases, offsets[0] != 0, offsets[rows] > nnz,
 * a column outside [0, cols)), a size outside int32, a NULL pointer that is
 * needed (one of the two value arrays alone, too); nothing is written then. */
rsp_status_t rsp_csr2csc(rsp_handle_t handle, int64_t rows, int64_t cols, int64_t nnz,
                         const int *d_row_offsets, const int *d_col_ind, const void *d_values,
                         rsp_datatype_t value_type, int *d_csc_col_offsets, int *d_csc_row_ind,
                         void *d_csc_values);

/* Schedule facts of the current schedule of `mat` (no cuSPARSE
 * counterpart; for byte accounting): its tile count, and how many stored
 * entries it reads through 16-bit column offsets (2 B each instead of the
 * 4-B colidx: tiles whose columns span < 65536; the rest read colidx).
 * NOT_INITIALIZED before the first bufferSize / preprocess / SpMV. */
rsp_status_t rsp_spmv_plan_info(rsp_spmat_t mat, int64_t *tiles, int64_t *entries_16bit);

/* Overlap of the halo exchange with the SpMV. Columns [0, ncols_local) of
 * `mat` are the rank's own x entries, the others arrive with the exchange.
 * Invalidates the schedule (the next bufferSize / preprocess / SpMV re-plans
 * it, and batches holding the old one become stale): the schedule then
 * puts the tiles that read own columns only first. rsp_spmv_part runs
 * part 1 = those interior tiles (launch it while the exchange is in flight),
 * part 2 = the remaining tiles, long rows included; part 0 = everything
 * (== rsp_spmv). Part 1 followed by part 2 gives y bit for bit equal to
 * rsp_spmv. beta must be 0 for parts 1 and 2. */
rsp_status_t rsp_spmat_set_local_cols(rsp_spmat_t mat, int64_t ncols_local);
rsp_status_t rsp_spmv_part(rsp_handle_t handle, const void *alpha, rsp_spmat_t mat,
                           const void *d_x, const void *beta, void *d_y,
                           rsp_datatype_t compute_type, void *d_buffer, int part);

/* Batched SpMV: y_j = alpha*A_j*x_j + beta*y_j for `count` independent
 * matrices of one compute type, as ONE kernel launch per 32 matrices (rows
 * longer than a tile are finished inside it by their last-arriving chunk).
 * No cuSPARSE counterpart: the reference calls cusparseSpMV once per matrix
 * (GPU/spmv.cu:179-186); this is the same product per matrix, bit for bit
 * equal to rsp_spmv / rsp_spmv_part on each, without the per-launch ramp and
 * drain. `part` selects the schedule part of every matrix as rsp_spmv_part
 * (0 = whole product). Create records the pointers (x_j, y_j stay valid
 * until destroy) and plans the batch's own tiling of every matrix (full tiles
 * once the launch fills the chip; a matrix without a schedule is planned
 * first, its long-row partials stay in its schedule, so a matrix may appear
 * once per batch: INVALID_VALUE otherwise). d_buffers is unused (may be
 * NULL). Run fails with INVALID_VALUE if a matrix has been re-planned or
 * given other values (rsp_csr_set_values) since. Create and destroy are
 * host-blocking. */
rsp_status_t rsp_spmv_batch_create(rsp_handle_t handle, int count, const rsp_spmat_t *mats,
                                   const void *const *d_x, void *const *d_y,
                                   void *const *d_buffers, rsp_datatype_t compute_type,
                                   int part, rsp_spmv_batch_t *batch);
rsp_status_t rsp_spmv_batch_run(rsp_handle_t handle, rsp_spmv_batch_t batch, const void *alpha,
                                const void *beta);
rsp_status_t rsp_spmv_batch_destroy(rsp_spmv_batch_t batch);
/* rsp_spmv_plan_info of a batch's own schedule (its part of every matrix):
 * tiles of all its launches, and the entries they read through 16-bit
 * column offsets. */
rsp_status_t rsp_spmv_batch_info(rsp_spmv_batch_t batch, int64_t *tiles, int64_t *entries_16bit);

/* Number of dependency levels found by the analysis (L DAG, L^T DAG). */
rsp_status_t rsp_ilu0_levels(rsp_ilu0_info_t info, int *levels_lower, int *levels_upper);
/* Extension (round 6): the blocks of the block-inverse solve the analysis
 * planned for the L and L^T solves (0: that solve is level-scheduled). Deep
 * DAGs (<= 32 rows per level on average; RSP_ILU_BLOCKS=1 / 0 at analysis
 * time forces it on / off) are solved block by block, each row's unknown
 * written as a combination of its block's right-hand sides and of earlier
 * blocks' unknowns: same unknowns, rounding of that order (restated in the
 * oracle), within SURVEY 8c's tolerance of the reference's order.
 * LDS rule: the solve builds each block's coefficients in the LDS of one CU,
 * the largest block staged whole. A DAG whose plan needs more than
 * 160 KiB (163,840 B) there, counted for fp64 values as
 *   8 * max over blocks (dependencies + 1 + pattern entries)
 * + 4 * max over blocks (2 * pattern entries + 1 + recipe items + levels + 1),
 * gets no block plan: 0 is reported for it and its solve is level-scheduled
 * in the reference's order, for fp64 and fp32 alike. L and L^T are decided
 * separately. A dense 64-row diagonal block or a full band of half-width 12
 * are such patterns. */
rsp_status_t rsp_ilu0_solve_blocks(rsp_ilu0_info_t info, int *blocks_lower, int *blocks_upper);

/* Tests and profiling (no cuSPARSE counterpart, no device needed): the host
 * phases of rsp_ilu0_analysis on HOST arrays (base 0) — validation, levels,
 * symbolic factor, factor and solve plans. Returns the level counts, a 64-bit
 * digest of every array built (equal to rsp_ilu0_plan_digest of a device
 * analysis of the same pattern, whatever runs where) and, if phase_ms is not
 * NULL, the wall time of its 6 phases in ms. The slot layout's budget is
 * RSP_ILU_SLOT_CAP_MB as in the analysis, else 2 GB. Same status codes as the
 * analysis (INVALID_VALUE for a malformed or unsorted pattern). */
rsp_status_t rsp_ilu0_analysis_host(int n, const int *row_offsets, const int *col_ind,
                                    int *levels_lower, int *levels_upper, uint64_t *digest,
                                    double *phase_ms);
/* Tests (no cuSPARSE counterpart, no device needed): the level plans of the
 * same host phases — the L, L^T and U solve plans and the factor plan —
 * checked and counted. The slot layout's budget is RSP_ILU_SLOT_CAP_MB if the
 * environment sets it, else rsp_ilu0_analysis_host's.
 * The check (INTERNAL_ERROR if it fails; the first violation goes to stderr),
 * per solve plan: every row is one task, in level order, a level's short rows
 * before its wave rows before its hub rows; a task's flat terms are its row's
 * terms in the solve's order, pad terms only where a thin row's term groups
 * end; a thin level's term reads the y window slot of a producer that lies
 * earlier in the run and at most 4096 slots before the end of the consumer's
 * level, or is staged once in its own chunk and produced before that chunk;
 * chunks tile their run within 1024 rows and 4096 terms; every thin row
 * record decodes to its task (16-bit halves included); flow items cover each
 * level's rows once, in order, short groups of 1 to 64 rows, with the gate
 * the gate distance defines. Factor plan: every position of a thin level's
 * rows is an item of one chunk once, within the chunk budgets, its pair
 * start | count << 16 intact; a slot level's rm <= 256 and qm <= 1024 cover
 * its rows, slots do not overlap and end within slot_total <= the budget; a
 * flow run holds only slot levels without global-path rows, its items' rm |
 * qm << 16 and offsets the level's.
 * facts[0 .. nfacts): RSP_ILU_PLAN_FACTS values (less are cut, more are 0).
 * Three blocks of 26 for the L, L^T and U DAG (d = 0, 26, 52):
 *   d+0 levels; d+1 term group (2 / 4); d+2 thin segments; d+3 fat segments
 *   launched level by level; d+4 flow segments; d+5 thin chunks; d+6 / d+7
 *   most rows / flat terms of a chunk; d+8 staged terms; d+9 window terms;
 *   d+10 slots of the longest thin run; d+11 / d+12 thin short / wave rows;
 *   d+13 / d+14 / d+15 fat short / wave / hub rows; flow items: d+16 of 64
 *   short rows, d+17 of 1 to 63 short rows (d+21: of those, of one row),
 *   d+18 of one wave or hub row; d+19 levels in the padded short-row layout;
 *   d+20 most padded terms of a thin level; d+22 / d+23 thin / fat levels;
 *   d+24 flow items with a gate; d+25 levels of the longest flow segment.
 * Then the factor (q = 78): q+0 fac_one (one level: no update pairs); q+1
 *   fac_scale (one scaling launch, no plan: the rest is 0); q+2 thin
 *   segments; q+3 fat levels; q+4 of them in the slot layout; q+5 / q+6 fat
 *   levels the padding rule / the budget kept off it; q+7 fat levels' rows on the
 *   global path (> 256 entries or > 1024 update pairs); q+8 flow runs; q+9 levels in
 *   them; q+10 thin chunks; q+11 .. q+14 most items / pairs / staged values /
 *   rounds of a chunk; q+15 most update pairs of one position in a thin
 *   level; q+16 / q+17 most entries / update pairs of a fat level's row within those limits (rm / qm); q+18 slot_total
 *   (ints); q+19 factor levels; q+20 most positions of a thin level; q+21
 *   fewest positions of a fat level; q+22 thin levels; q+23 fat levels with
 *   global-path rows; q+24 thin levels that hold such a row (hub levels);
 *   q+25 most rows of a thin level. */
#define RSP_ILU_PLAN_FACTS 104
rsp_status_t rsp_ilu0_plan_facts_host(int n, const int *row_offsets, const int *col_ind, int64_t *facts,
                                      int nfacts);
/* Tests (no cuSPARSE counterpart, no device needed): the SpMV schedule
 * rsp_spmv_buffer_size builds (tiles, 16-bit column offsets, staged tiles'
 * column runs) for HOST arrays (base 0, m rows, compute type fp64 / fp32),
 * checked for consistency: every entry of a 16-bit tile decodes to its own
 * column (cbase + offset, or the staged tile's runs at its slot index), every
 * staged tile's runs are ascending and within its slot and run caps; a packed
 * tile's slots are read from its record (12-bit fields, padding 0) and its
 * 16-bit row offsets are checked against row_offsets. Returns
 * the tile count, the entries read through 16-bit values and, of those, the
 * entries of staged tiles; INTERNAL_ERROR if a check fails. */
rsp_status_t rsp_spmv_plan_host(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                rsp_datatype_t compute_type, int64_t *tiles, int64_t *entries_16bit,
                                int64_t *entries_staged);
/* Tests (no device needed): the same schedule tile by tile. The plan is made
 * for the given planner options (spread: resident workgroup slots a small plan
 * is spread over, 0 none; local_cols: rsp_spmat_set_local_cols, -1 none;
 * row_align >= 1: rows a packed tile's end is aligned to; use_c16 / use_stage:
 * 0 switches the 16-bit offsets / the staged tiles off) and the environment's
 * plan-time knobs, checked as rsp_spmv_plan_host checks it (INTERNAL_ERROR if
 * the check fails), and the first max_tiles tiles are written in plan order as
 * RSP_SPMV_TILE_FACTS integers each:
 *   +0 r0, the first row; +1 r1 as stored: the row after the last, INT_MIN for
 *   a whole long row, -(slot + 1) for a chunk of a longer one; +2 / +3 k0 / k1,
 *   the entries; +4 kind: 0 int32 col_ind, 1 16-bit offsets from a base, 2
 *   staged by runs, 3 staged by a column list; +5 the column base (kind 1) or
 *   the smallest column (kinds 2, 3), 0 for kind 0; +6 U, the distinct columns
 *   of a staged tile; +7 R, the contiguous runs they form (kind 2: the
 *   descriptors before the sentinel); +8 1 with a packed record; +9 1 if the
 *   record holds the row offsets.
 * counts[0] tiles (all of them, also past max_tiles); [1] interior tiles of a
 * split schedule; [2] rows cut into chunks; [3] their partial slots. */
#define RSP_SPMV_TILE_FACTS 10
rsp_status_t rsp_spmv_plan_tiles_host(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                      rsp_datatype_t compute_type, int64_t spread, int64_t local_cols, int row_align,
                                      int use_c16, int use_stage, int64_t *facts, int64_t max_tiles,
                                      int64_t counts[4]);
/* Profiling (no cuSPARSE counterpart; scripts/bench_spmv_t.py): the
 * permutation pass of rsp_spmv(op = TRANSPOSE) alone, on the handle's stream:
 * the current values of `mat` into its transposed side, no product.
 * NOT_INITIALIZED before the transposed side exists (or while it is of another
 * type than the matrix, after rsp_csr_set_values). */
rsp_status_t rsp_spmv_transpose_permute(rsp_handle_t handle, rsp_spmat_t mat);
/* Tests (no device needed): the transposer behind rsp_spmv(op = TRANSPOSE)
 * and rsp_csr2csc on HOST arrays (base 0): t_row_offsets (cols + 1),
 * t_col_ind and perm (row_offsets[rows] entries each; entry k of A^T is entry
 * perm[k] of A), a serial stable counting sort by column. Only
 * row_offsets[rows] entries of col_ind are read. INVALID_VALUE for a
 * malformed pattern (as rsp_csr2csc) or a NULL array that is needed; nothing
 * is written then. */
rsp_status_t rsp_csr_transpose_host(int64_t rows, int64_t cols, const int *row_offsets, const int *col_ind,
                                    int *t_row_offsets, int *t_col_ind, int *perm);
/* Tests and records (no device needed): what ONE call over the schedule of the
 * same host pattern reads besides the values, x and y, counted per tile on the
 * vector path. RSP_SPMV_PACK (0, 1, 2 = default; read when a schedule is built) selects
 * the packed records of staged tiles. stats[0] tiles; [1] packed tiles; [2]
 * their entries; [3] schedule bytes = 24 per tile (its record, column base and
 * packed offset) + [6] + the staged tiles' descriptors (8 per run and sentinel,
 * or 8 + 2 per listed column) + [7]; [4] bytes of the caller's row offsets
 * still read: 4 (rows + 1) per tile without packed row offsets (4 per long-row
 * tile); [5] staged tiles; [6] index bytes: 4 per entry of an int32 tile, 2 per
 * entry of a 16-bit tile, 4 * 256 * NW per packed tile (NW = 3 fp64, 6 fp32);
 * [7] packed row offsets: 2 (rows + 1) per packed tile, rounded up to 4. */
rsp_status_t rsp_spmv_plan_stats(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                 rsp_datatype_t compute_type, int64_t stats[8]);
/* The digest of the plan an rsp_ilu0_analysis built (see above); computed
 * only when the environment sets RSP_ILU_DIGEST=1 at analysis time
 * (INVALID_VALUE otherwise). */
rsp_status_t rsp_ilu0_plan_digest(rsp_ilu0_info_t info, uint64_t *digest);

#ifdef __cplusplus
}
#endif

#endif /* RSP_H */
