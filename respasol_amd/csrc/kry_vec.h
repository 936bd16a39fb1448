// kry_vec.h — what the element-wise kernels of krylov.hip and cheby.hip share:
// the 16-byte group a thread moves, its load and store, and the loop over a
// workgroup's range (rsp::kry_grid). Included after RSP_KNS is defined; the
// helpers are private to each translation unit (and to each of its two builds).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "rsp_kernels.h"

namespace RSP_KNS {
namespace {

template <typename T>
struct Grp {
    static constexpr int V = 16 / sizeof(T);
    T e[V];
};

template <typename T, bool VEC>
__device__ __forceinline__ Grp<T> ld(const T *p, long long j, int cnt) {
    Grp<T> g;
    if (VEC && cnt == Grp<T>::V) {
        using V4 = __attribute__((ext_vector_type(4))) unsigned;
        const V4 w = *reinterpret_cast<const V4 *>(p + j);
        __builtin_memcpy(g.e, &w, 16);
    } else {
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) g.e[k] = k < cnt ? p[j + k] : T(0);
    }
    return g;
}

template <typename T, bool VEC>
__device__ __forceinline__ void st(T *p, long long j, int cnt, const Grp<T> &g) {
    if (VEC && cnt == Grp<T>::V) {
        using V4 = __attribute__((ext_vector_type(4))) unsigned;
        V4 w;
        __builtin_memcpy(&w, g.e, 16);
        *reinterpret_cast<V4 *>(p + j) = w;
    } else {
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++)
            if (k < cnt) p[j + k] = g.e[k];
    }
}

// the loop every kernel shares: thread t's groups of the workgroup's range
#define KRY_FOR_GROUPS(T, n, chunk)                                                             \
    const long long c0_ = (long long)blockIdx.x * (chunk);                                      \
    const long long c1_ = c0_ + (chunk) < (n) ? c0_ + (chunk) : (n);                            \
    for (long long j = c0_ + (long long)threadIdx.x * Grp<T>::V; j < c1_;                       \
         j += (long long)rsp::kKryThreads * Grp<T>::V)                                          \
        if (const int cnt = (int)(c1_ - j < Grp<T>::V ? c1_ - j : Grp<T>::V))

inline bool aligned16(std::initializer_list<const void *> ps) {
    uintptr_t m = 0;
    for (const void *p : ps) m |= (uintptr_t)p;
    return (m & 15) == 0;
}

}  // namespace
}  // namespace RSP_KNS
