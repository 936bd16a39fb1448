// csr_transpose.hip — the value permutation of the transposed SpMV and of
// rsp_csr2csc: vt[k] = v[perm[k]] for k < nnz, perm from csr_transpose.h.
//
// A bit move: the elements are loaded and stored as 32- or 64-bit integers,
// never as floats, so no build flag can flush a denormal or quieten a NaN, and
// the unit is built once (no _ftz twin).
//
// perm and vt are the library's own arrays (256-B aligned) or, for
// rsp_csr2csc, checked for 16-B alignment by the launcher: each lane reads 16 B
// of perm (fp32: 4 indices) or 8 B (fp64: 2 indices) and writes 16 B of vt per
// step, all its gathers issued before the store. Only the gather from v is per
// element, so v needs no more than its element's alignment (a torch slice). A
// grid-stride loop over a grid sized from the CU count; the < W elements past
// the last whole vector go one per lane to the first lanes of workgroup 0.
// Measured beside it and not kept: the same
// vectors with each gather instruction covering consecutive elements (4-B
// index loads, or a transposition through LDS) ran within 3 % either way; one
// element per lane is faster on some matrices and slower on as many.

#include "rsp_kernels.h"

namespace rsp_k {

namespace {

constexpr int kPermThreads = 256;
constexpr int kPermBlocksPerCu = 8;  // 32 waves per CU: the gathers' latency is hidden by waves, not by unrolling

template <typename U, int W>
struct PermVec {
    typedef U vals __attribute__((ext_vector_type(W)));
    typedef int idx __attribute__((ext_vector_type(W)));
};

template <typename U, int W, bool VEC>
__global__ __launch_bounds__(kPermThreads) void permute_kernel(const int *__restrict__ perm, const U *__restrict__ v,
                                                               U *__restrict__ vt, int64_t nnz) {
    typedef typename PermVec<U, W>::vals ValVec;
    typedef typename PermVec<U, W>::idx IdxVec;
    const int64_t tid = (int64_t)blockIdx.x * kPermThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kPermThreads;
    const int64_t nvec = VEC ? nnz / W : 0;
    for (int64_t i = tid; i < nvec; i += stride) {
        const IdxVec p = reinterpret_cast<const IdxVec *>(perm)[i];
        ValVec o;
#pragma unroll
        for (int j = 0; j < W; j++) o[j] = v[p[j]];
        reinterpret_cast<ValVec *>(vt)[i] = o;
    }
    // the tail (every element when the arrays are not 16-B aligned)
    for (int64_t k = nvec * W + tid; k < nnz; k += stride) vt[k] = v[perm[k]];
}

template <typename U, int W>
hipError_t launch_permute(int64_t nnz, const int *perm, const void *v, void *vt, int num_cus, hipStream_t s) {
    const bool vec = ((((uintptr_t)perm) | ((uintptr_t)vt)) & 15) == 0;
    const int64_t per_block = (int64_t)kPermThreads * (vec ? W : 1);
    const int64_t want = (nnz + per_block - 1) / per_block;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * kPermBlocksPerCu;
    const int grid = (int)(want < cap ? want : cap);
    if (vec)
        hipLaunchKernelGGL((permute_kernel<U, W, true>), dim3(grid), dim3(kPermThreads), 0, s, perm, (const U *)v,
                           (U *)vt, nnz);
    else
        hipLaunchKernelGGL((permute_kernel<U, W, false>), dim3(grid), dim3(kPermThreads), 0, s, perm, (const U *)v,
                           (U *)vt, nnz);
    return hipGetLastError();
}

}  // namespace

hipError_t permute_values(int elem_bytes, int64_t nnz, const int *perm, const void *v, void *vt, int num_cus,
                          hipStream_t s) {
    if (nnz <= 0) return hipSuccess;
    return elem_bytes == 8 ? launch_permute<uint64_t, 2>(nnz, perm, v, vt, num_cus, s)
                           : launch_permute<uint32_t, 4>(nnz, perm, v, vt, num_cus, s);
}

void warm_transpose() {
    int o = 0;  // (the use that loads the code object, as warm_spmv)
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, permute_kernel<uint32_t, 4, true>, kPermThreads, 0);
}

}  // namespace rsp_k
