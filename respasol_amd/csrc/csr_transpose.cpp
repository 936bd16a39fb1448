// csr_transpose.cpp — see csr_transpose.h. A stable counting sort by column,
// with t_rp itself as the counters and the cursors (no allocation, so nothing
// here throws).

#include "csr_transpose.h"

#include <limits.h>

namespace rsp_tr {

bool pattern_ok(int64_t rows, int64_t cols, const int *rp, const int *ci) {
    if (rows < 0 || cols < 0 || rows > INT_MAX - 1 || cols > INT_MAX - 1) return false;
    if (rows == 0) return true;
    if (!rp || rp[0] != 0) return false;  // base 0 only
    for (int64_t i = 0; i < rows; i++)
        if (rp[i + 1] < rp[i]) return false;  // (rp[0] == 0: none is negative either)
    const int64_t nnz = rp[rows];
    if (nnz > 0 && !ci) return false;
    for (int64_t k = 0; k < nnz; k++)
        if ((unsigned)ci[k] >= (unsigned)cols) return false;
    return true;
}

rsp_status_t csr_transpose(int64_t rows, int64_t cols, const int *rp, const int *ci, int *t_rp, int *t_ci,
                           int *perm) {
    if (!pattern_ok(rows, cols, rp, ci) || !t_rp) return RSP_STATUS_INVALID_VALUE;
    const int64_t nnz = rows > 0 ? rp[rows] : 0;
    if (nnz > 0 && (!t_ci || !perm)) return RSP_STATUS_INVALID_VALUE;
    for (int64_t c = 0; c <= cols; c++) t_rp[c] = 0;
    // entries per column, at t_rp[c + 1]; then the exclusive scan in place
    for (int64_t k = 0; k < nnz; k++) t_rp[(int64_t)ci[k] + 1]++;
    for (int64_t c = 0; c < cols; c++) t_rp[c + 1] += t_rp[c];
    // t_rp[c] is column c's cursor while the entries are placed in storage order ...
    for (int64_t i = 0; i < rows; i++)
        for (int k = rp[i]; k < rp[i + 1]; k++) {
            const int at = t_rp[ci[k]]++;
            t_ci[at] = (int)i;
            perm[at] = k;
        }
    // ... which leaves it at column c's end, the start of column c + 1
    for (int64_t c = cols; c > 0; c--) t_rp[c] = t_rp[c - 1];
    t_rp[0] = 0;
    return RSP_STATUS_SUCCESS;
}

}  // namespace rsp_tr

extern "C" rsp_status_t rsp_csr_transpose_host(int64_t rows, int64_t cols, const int *row_offsets,
                                               const int *col_ind, int *t_row_offsets, int *t_col_ind,
                                               int *perm) {
    return rsp_tr::csr_transpose(rows, cols, row_offsets, col_ind, t_row_offsets, t_col_ind, perm);
}
