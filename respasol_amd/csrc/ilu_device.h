// ilu_device.h — per-lane and per-wave arithmetic and LDS primitives shared by
// the ILU(0) factor (ilu0.hip) and the triangular solves (trsv.hip). Every
// helper is inlined into its kernel; compiled in the including unit's kernel
// namespace (rsp_k / rsp_k_ftz).
#pragma once

#include <hip/hip_runtime.h>

#include "rsp_kernels.h"

#ifndef RSP_KNS
#define RSP_KNS rsp_k
#endif

namespace RSP_KNS {

// Fused multiply-add in the working precision: v_fma_f64 / v_fma_f32 (one
// rounding), as the oracle's fma / fmaf. (__builtin_fma on float operands
// would compute in double and round twice.)
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// x / d, the IEEE quotient rounded to T. The FTZ build's float division
// switches the denormal mode on and off around its Newton steps (two
// s_setreg per division: the only difference between ilu0_rounds<float> in
// rsp_k and rsp_k_ftz, found in their ISA), serialising the wave on every
// l_ik = a_ik / u_kk. Here the FTZ build takes a float quotient in double,
// rounded once to float: double has >= 2 * 24 + 2 bits, so that is the
// correctly rounded float quotient for every operand, with fp32 denormals
// flushed by the mode as the oracle's DAZ/FTZ (same bits as the float
// division). Measured on dc1, matrix-new_3, xenon2, ASIC_320ks, crashbasis
// (FTZ factor, ms): float division 25.32, this 24.89; the float Newton
// sequence without the mode switch is 24.06 but loses the correct rounding
// when a residual is denormal (numerators near 2^-103, divisors >= 2^126),
// and guarding it (range checks + rescaling, 26.33; a fallback branch,
// 27.88) costs more than it saves: the division is on the factor's
// dependency chain (profiles/r06_ftz_division_ab.txt).
template <typename T>
__device__ __forceinline__ T qdiv(T x, T d) {
#ifdef RSP_FTZ_BUILD
    if constexpr (sizeof(T) == 4) {
        // (the empty asm keeps the optimiser from folding the widened
        // division back into a float one, a legal rewrite it makes)
        double xd = x, dd = d;
        asm volatile("" : "+v"(xd), "+v"(dd));
        return (float)(xd / dd);
    }
#endif
    return x / d;
}

// Order this wave's LDS stores before its later LDS loads (one wave's LDS
// accesses are performed in order; the fences keep the compiler to it).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// An eight-int plan record (rsp::RndChunk, rsp::LevelChunk) read through the
// constant address space: scalar loads, which the kernels' stores cannot
// alias and which leave vmcnt to the prefetch.
template <typename R>
__device__ __forceinline__ R load_chunk(const R *recs, int c) {
    static_assert(sizeof(R) == 8 * sizeof(int), "an eight-int record");
    typedef const __attribute__((address_space(4))) int *ChunkPtr;
    const ChunkPtr q = (ChunkPtr)recs + (size_t)c * 8;
    return R{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
}

// s - sum_p v_p y_p as a serial fma chain over p = p0 .. p1-1, ascending.
// The operands of B consecutive terms are loaded together (clamped,
// unpredicated) so the loads of a batch overlap instead of serialising
// behind each fma; B is picked per DAG from its mean chain length so short
// rows do not pay for dead loads.
template <typename T, int B, typename FV, typename FY>
__device__ __forceinline__ T fma_chain(T s, int p0, int p1, FV vat, FY yat) {
    const int n = p1 - p0;
    for (int b0 = 0; b0 < n; b0 += B) {
        T v[B], y[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int p = p0 + min(b0 + b, n - 1);
            v[b] = vat(p);
            y[b] = yat(p);
        }
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (b0 + b < n) s = fma_t(-v[b], y[b], s);
    }
    return s;
}

// The same serial fma chain for one long row, by a whole wave: lanes load 64
// terms at once, then the chain runs over them in order on wave-uniform
// registers (readlane), so a hub row pays one load round trip per 64 terms.
__device__ __forceinline__ double wave_read(double v, int j) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, j), hi = __builtin_amdgcn_readlane((int)(b >> 32), j);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ float wave_read(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

template <typename T, typename FV, typename FY>
__device__ __forceinline__ T wave_chain(T s, int k0, int k1, int lane, FV vat, FY yat) {
    for (int base = k0; base < k1; base += 64) {
        const int k = min(base + lane, k1 - 1);
        const T v = vat(k), yv = yat(k);
        const int cnt = min(64, k1 - base);
        for (int j = 0; j < cnt; ++j) s = fma_t(-wave_read(v, j), wave_read(yv, j), s);
    }
    return s;
}

// The same chain for one fat-level row by a wave, on LDS broadcast operands:
// each group of 64 terms is gathered by the lanes (values, then y; the next
// group's loads are issued before this group's chain), parked in the wave's
// LDS rows, and every lane runs the in-order fma chain reading them (reads
// independent of the sum, so they issue ahead of it) — instead of four
// readlanes per term. One fma per term in order: the same bits.
template <typename T>
__device__ __forceinline__ T wave_chain_lds(T s, int k0, int k1, int lane, T *wv, T *wy, const T *sval,
                                           const int *src, const T *y) {
    int k = min(k0 + lane, k1 - 1);
    T v = sval[k];
    int id = src[k];
    T yv = y[id];
    for (int base = k0; base < k1; base += 64) {
        wv[lane] = v;
        wy[lane] = yv;
        wave_sync();
        const int cnt = min(64, k1 - base);
        const bool more = base + 64 < k1;
        if (more) {  // the next group's values and y indices in flight under this chain
            k = min(base + 64 + lane, k1 - 1);
            v = sval[k];
            id = src[k];
        }
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            T p[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                p[u] = wv[j + u];
                q[u] = wy[j + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s = fma_t(-p[u], q[u], s);
        }
        for (; j < cnt; ++j) s = fma_t(-wv[j], wy[j], s);
        wave_sync();  // this group's reads before the next group's stores
        if (more) yv = y[id];
    }
    return s;
}

// LDS-only workgroup barrier (no vmcnt drain).
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Wait until the LDS counter *p >= want (wave-uniform value; bounded: a plan
// bug gives wrong bits in the tests, never a hung GPU): read -> wait ->
// compare, back to back. Every gentler poll (sleeps, a wake-up, two reads in
// flight) measured slower: DESIGN.md §5, "Polls of the narrow-run counters".
// The counter is published by lds_publish (release) and read here with an
// acquire fence after the last poll: the HIP memory model orders a wave's y
// stores before the counter and the waiting wave's y loads after it.
__device__ __forceinline__ void lds_wait_geq(int *p, int want) {
    for (int it = 0; it < (1 << 26) && __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want;
         ++it) {
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Publish an LDS counter of completed levels / rounds (lane 0 of the wave
// that completed them): a workgroup-scope release store, so every LDS store
// of the wave before it (its y / values) is visible to a wave whose
// lds_wait_geq has seen the new value.
__device__ __forceinline__ void lds_publish(int *p, int v, bool leader) {
    if (leader) __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace RSP_KNS
