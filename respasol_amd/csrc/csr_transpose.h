// csr_transpose.h — the host-side transposer behind rsp_spmv(op = TRANSPOSE)
// and rsp_csr2csc: the CSR pattern of A^T and the permutation that carries A's
// values into it. Pure host C++ (no HIP calls, no allocation): rsp_api.cpp
// downloads the pattern, calls csr_transpose and uploads the result;
// rsp_csr_transpose_host runs it on host arrays; drivers/csr_transpose_check.cpp
// runs it under the sanitizers (make asan-transpose).
//
// The order is the library's definition of A^T ("Transposed SpMV"):
// row j of A^T holds the entries of column j of A in storage order — ascending
// row of A, and within a row the order they are stored in. That is a stable
// counting sort of the stored entries by column; duplicates and unsorted rows
// of A are legal and keep that order.
#ifndef RSP_CSR_TRANSPOSE_H
#define RSP_CSR_TRANSPOSE_H

#include <stdint.h>

#include "rsp.h"

namespace rsp_tr {

// True if `rp` (rows + 1 offsets, base 0, non-decreasing) and the rp[rows]
// column indices `ci` (each inside [0, cols)) are a CSR pattern the transposer
// takes; rows, cols and rp[rows] fit an int32.
bool pattern_ok(int64_t rows, int64_t cols, const int *rp, const int *ci);

// The transpose of a `rows` x `cols` pattern with nnz = rp[rows] stored entries
// (arrays past that are not read): t_rp[cols + 1] the row offsets of A^T,
// t_ci[nnz] its column indices (rows of A), perm[nnz]: entry k of A^T is entry
// perm[k] of A. Serial. INVALID_VALUE for a pattern that is not pattern_ok
// (nothing is written then) or a NULL array that is needed.
rsp_status_t csr_transpose(int64_t rows, int64_t cols, const int *rp, const int *ci, int *t_rp, int *t_ci,
                           int *perm);

}  // namespace rsp_tr

#endif
