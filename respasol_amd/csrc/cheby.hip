// cheby.hip — the Chebyshev polynomial preconditioner (rsp_cheby_*) for gfx950:
// z = p_k(D^-1 A) D^-1 r, the polynomial of the Chebyshev iteration on
// [lmin, lmax] started from zero. An apply of degree k is
//
//   cheby_first   d = c0 * (dinv * r);  z = d;  w = r
//   j = 1 .. k-1: w = w - A d            -- rsp_spmv(alpha = -1, beta = 1) --
//   cheby_step    t = dinv * w;  d = (a_j * d) + (b_j * t);  z = z + d
//
// with the coefficients of include/rsp.h, computed on the host and rounded once
// to P, the type of the matrix. No dot product, no scalar on the device, no
// synchronisation but the launch boundaries: every product and sum is rounded
// to P (the unit is built with -ffp-contract=off), so an element's result is a
// function of its own inputs and does not depend on the grid, the alignment or
// the tail handling. Without scaling (dinv null) the product with dinv is
// skipped. Traffic per element, in values of P: cheby_first reads 2 (1 without
// scaling) and writes 3 (degree 1: 1); cheby_step reads 4 (3) and writes 2
// (the last: 1).
//
// Element ownership, the 16-byte groups and the scalar path for pointers that
// are only naturally aligned are krylov.hip's (kry_vec.h).
//
// cheby_setup is the whole set-up in one launch, one lane per row in storage
// order (it is not the hot path): the diagonal and its inverse, the row's
// Gershgorin quotient, their maximum and the smallest row without a usable
// diagonal (rsp::ChebySetupArgs).
//
// Compiled twice: namespace rsp_k (fp64 + fp32) and rsp_k_ftz (fp32,
// -fgpu-flush-denormals-to-zero), see rsp_kernels.h.

#include <hip/hip_runtime.h>

#include "rsp_kernels.h"

#ifndef RSP_KNS
#define RSP_KNS rsp_k
#endif

#include "kry_vec.h"

namespace RSP_KNS {

using namespace rsp;

namespace {

template <typename T, bool VEC, bool JAC>
__global__ __launch_bounds__(kKryThreads) void cheby_first(long long n, long long chunk, T c0, int only_z,
                                                           const T *__restrict__ dinv, const T *__restrict__ r,
                                                           T *__restrict__ z, T *__restrict__ d,
                                                           T *__restrict__ w) {
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> gr = ld<T, VEC>(r, j, cnt);
        Grp<T> gd = gr;
        if constexpr (JAC) {
            const Grp<T> gi = ld<T, VEC>(dinv, j, cnt);
#pragma unroll
            for (int k = 0; k < Grp<T>::V; k++) gd.e[k] = gi.e[k] * gr.e[k];
        }
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) gd.e[k] = c0 * gd.e[k];
        st<T, VEC>(z, j, cnt, gd);
        if (!only_z) {
            st<T, VEC>(d, j, cnt, gd);
            st<T, VEC>(w, j, cnt, gr);
        }
    }
}

template <typename T, bool VEC, bool JAC>
__global__ __launch_bounds__(kKryThreads) void cheby_step(long long n, long long chunk, T a, T b, int only_z,
                                                          const T *__restrict__ dinv, const T *__restrict__ w,
                                                          T *__restrict__ z, T *__restrict__ d) {
    KRY_FOR_GROUPS(T, n, chunk) {
        Grp<T> gt = ld<T, VEC>(w, j, cnt);
        Grp<T> gd = ld<T, VEC>(d, j, cnt), gz = ld<T, VEC>(z, j, cnt);
        if constexpr (JAC) {
            const Grp<T> gi = ld<T, VEC>(dinv, j, cnt);
#pragma unroll
            for (int k = 0; k < Grp<T>::V; k++) gt.e[k] = gi.e[k] * gt.e[k];
        }
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) {
            gd.e[k] = (a * gd.e[k]) + (b * gt.e[k]);
            gz.e[k] = gz.e[k] + gd.e[k];
        }
        st<T, VEC>(z, j, cnt, gz);
        if (!only_z) st<T, VEC>(d, j, cnt, gd);
    }
}

template <typename T>
__global__ __launch_bounds__(kKryThreads) void cheby_setup_rows(int n, const int *__restrict__ rowptr,
                                                                const int *__restrict__ colidx,
                                                                const T *__restrict__ vals, T *__restrict__ dinv,
                                                                unsigned long long *state) {
    __shared__ unsigned long long lds[kKryThreads / 64];
    const long long i = (long long)blockIdx.x * kKryThreads + threadIdx.x;
    unsigned long long gbits = 0;  // (a non-negative double's bits order as the values do)
    if (i < n) {
        T diag = T(0);
        double sum = 0.0;
        bool has = false;
        for (int k = rowptr[i], e = rowptr[i + 1]; k < e; k++) {
            const T v = vals[k];
            sum += __builtin_fabs((double)v);
            if (colidx[k] == (int)i) {
                diag = diag + v;
                has = true;
            }
        }
        double g = sum;
        bool bad = false;
        if (dinv) {
            bad = !has || diag == T(0) || !__builtin_isfinite(diag);
            if (bad) {
                atomicMin(&state[1], (unsigned long long)i);
                g = 0.0;
            } else {
                dinv[i] = T(1) / diag;
                g = sum / __builtin_fabs((double)diag);
            }
        }
        if (!__builtin_isfinite(g)) g = __builtin_inf();
        gbits = (unsigned long long)__double_as_longlong(g);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(gbits, off, 64);
        gbits = o > gbits ? o : gbits;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = gbits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = lds[0];
#pragma unroll
        for (int k = 1; k < kKryThreads / 64; k++) m = lds[k] > m ? lds[k] : m;
        if (m) atomicMax(&state[0], m);
    }
}

template <typename T>
hipError_t launch(ChebyOp op, const ChebyArgs &a, hipStream_t s) {
    const KryGrid kg = kry_grid(a.n);
    const dim3 grid(kg.grid), block(kKryThreads);
    const long long n = a.n, ch = kg.chunk;
    const T *dinv = (const T *)a.dinv, *r = (const T *)a.r;
    T *z = (T *)a.z, *d = (T *)a.d, *w = (T *)a.w;
#define CHEBY_LAUNCH(ALIGNED, KERN, ...)                                                     \
    do {                                                                                     \
        if (ALIGNED) {                                                                       \
            if (dinv)                                                                        \
                hipLaunchKernelGGL((KERN<T, true, true>), grid, block, 0, s, __VA_ARGS__);   \
            else                                                                             \
                hipLaunchKernelGGL((KERN<T, true, false>), grid, block, 0, s, __VA_ARGS__);  \
        } else {                                                                             \
            if (dinv)                                                                        \
                hipLaunchKernelGGL((KERN<T, false, true>), grid, block, 0, s, __VA_ARGS__);  \
            else                                                                             \
                hipLaunchKernelGGL((KERN<T, false, false>), grid, block, 0, s, __VA_ARGS__); \
        }                                                                                    \
    } while (0)
    switch (op) {
        case kChebyFirst:
            // (degree 1 touches neither d nor w: they are not part of the alignment test)
            CHEBY_LAUNCH(a.only_z ? aligned16({dinv, r, z}) : aligned16({dinv, r, z, d, w}), cheby_first, n, ch,
                         (T)a.c0, a.only_z, dinv, r, z, d, w);
            break;
        case kChebyStep:
            CHEBY_LAUNCH(aligned16({dinv, w, z, d}), cheby_step, n, ch, (T)a.a, (T)a.b, a.only_z, dinv,
                         (const T *)w, z, d);
            break;
        default:
            return hipErrorInvalidValue;
    }
#undef CHEBY_LAUNCH
    return hipGetLastError();
}

template <typename T>
hipError_t setup_launch(const ChebySetupArgs &a, hipStream_t s) {
    const unsigned grid = (unsigned)(((long long)a.n + kKryThreads - 1) / kKryThreads);
    hipLaunchKernelGGL((cheby_setup_rows<T>), dim3(grid), dim3(kKryThreads), 0, s, a.n, a.rowptr, a.colidx,
                       (const T *)a.vals, (T *)a.dinv, a.state);
    return hipGetLastError();
}

}  // namespace

hipError_t cheby(ChebyOp op, int f32, const ChebyArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (f32) return launch<float>(op, a, s);
#ifndef RSP_FTZ_BUILD
    return launch<double>(op, a, s);
#else
    return hipErrorInvalidValue;
#endif
}

hipError_t cheby_setup(int f32, const ChebySetupArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (f32) return setup_launch<float>(a, s);
#ifndef RSP_FTZ_BUILD
    return setup_launch<double>(a, s);
#else
    return hipErrorInvalidValue;
#endif
}

}  // namespace RSP_KNS
