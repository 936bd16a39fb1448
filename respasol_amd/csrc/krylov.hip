// krylov.hip — the vector side of the ILU(0)-preconditioned BiCGStab iteration
// (rsp_bicgstab_*), of preconditioned CG (rsp_cg_*: the cg_* kernels) and of
// restarted flexible GMRES (rsp_gmres_*, rsp_orthogonalize: the gm_* kernels),
// both described where they start, rsp_dot, and the element-wise kernels of
// mixed-precision iterative refinement (rsp_refine_*, rsp_convert_scaled,
// rsp_refine_update: the ref_* kernels), for gfx950. The SpMVs and triangular solves of an iteration are the library's
// existing entry points; everything between them is here. BiCGStab, five
// launches per iteration:
//
//   p_update   rho' = (rhat,r); beta = (rho'/rho)(alpha/omega); p = r + beta (p - omega v)
//   dot_rhv    (rhat,v)
//   s_update   alpha = rho'/(rhat,v); s = r - alpha v
//   dot_ts     (t,s) and (t,t) in one pass
//   x_update   omega = (t,s)/(t,t); x += alpha phat + omega shat; r = s - omega t;
//              (rhat,r) and (r,r)
//
// Scalars stay on the device (rsp::kKry* slots of one fp64 block). A dot
// leaves one partial per workgroup; the kernel that needs the scalar sums the
// partials in its prologue — the launch boundary is the only synchronisation,
// so there is no counter, no fence and no atomic accumulator, and the result
// depends on n alone. Every workgroup derives the same scalar from the same
// partials in the same order; workgroup 0 also stores it for later kernels,
// into a slot that no workgroup of the same launch reads.
//
// Breakdown: a kernel that would divide by a zero or non-finite rho, omega,
// (rhat,v) or (t,t) stores a code in kKryFlag and returns; every later kernel
// returns on the code, so x, r and p keep their last good values. (t,t) == 0
// with a finite (t,s) is t == 0, i.e. s == 0 up to A's null space: omega = 0
// is taken (x += alpha phat, r = s), and the next iteration's omega check
// reports the breakdown if r is not yet small.
//
// Element ownership: workgroup g owns [g * chunk, (g + 1) * chunk), thread t
// the 16-byte groups t, t + 256, ... of it, in that order. Pointers that are
// all 16-byte aligned move whole groups (double2 / float4); otherwise (an
// 8-byte-aligned base) and in the tail the same elements move one by one, so
// the summation order does not depend on the alignment.
//
// Compiled twice: namespace rsp_k (fp64 + fp32) and rsp_k_ftz (the fp32 and
// fp32-copy forms, -fgpu-flush-denormals-to-zero), see rsp_kernels.h.

#include <hip/hip_runtime.h>

#include "rsp_kernels.h"

#ifndef RSP_KNS
#define RSP_KNS rsp_k
#endif

#include "kry_vec.h"  // Grp, ld, st, KRY_FOR_GROUPS, aligned16 (shared with cheby.hip)

namespace RSP_KNS {

using namespace rsp;

namespace {

// the fp32 copy of a double group (own allocation: 8-byte aligned at even j)
template <bool VEC>
__device__ __forceinline__ void st_copy32(float *p, long long j, int cnt, const Grp<double> &g) {
    if (VEC && cnt == 2) {
        *reinterpret_cast<float2 *>(p + j) = make_float2((float)g.e[0], (float)g.e[1]);
    } else {
        for (int k = 0; k < cnt; k++) p[j + k] = (float)g.e[k];
    }
}

// Sum of one value per thread, the same in every thread: 64-lane down-tree,
// then the four waves in order (rsp::kry_combine_host restates it).
__device__ __forceinline__ double block_sum(double v, double *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // lds free again
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ double combine(const double *blk, int dot, double *lds) {
    const double *part = blk + kKryScalars + (size_t)dot * kKryMaxGrid;
    const int g = (int)gridDim.x;
    double v = 0.0;
    for (int i = threadIdx.x; i < g; i += kKryThreads) v += part[i];
    return block_sum(v, lds);
}

__device__ __forceinline__ void put_partial(double *blk, int dot, double v) {
    if (threadIdx.x == 0) blk[kKryScalars + (size_t)dot * kKryMaxGrid + blockIdx.x] = v;
}

// The breakdown flag, the same for every thread of the workgroup (one thread
// reads it: a workgroup of the launch that sets it may otherwise see it change
// between two of its waves; such a workgroup derives the same breakdown from
// the partials itself, so either value makes it return).
__device__ __forceinline__ bool broken(const double *blk, double *lds) {
    if (threadIdx.x == 0) lds[0] = blk[kKryFlag];
    __syncthreads();
    return lds[0] != 0.0;  // (block_sum synchronises before it writes lds again)
}

__device__ __forceinline__ bool bad_divisor(double d) { return d == 0.0 || !__builtin_isfinite(d); }

__device__ __forceinline__ void set_break(double *blk, int code, int it) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        blk[kKryFlag] = (double)code;
        blk[kKryFlagIt] = (double)it;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void kry_init(long long n, long long chunk, double *blk,
                                                        const T *__restrict__ b, const T *__restrict__ v,
                                                        T *__restrict__ r, T *__restrict__ rhat) {
    __shared__ double lds[kKryThreads / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        blk[kKryRho0] = 1.0;
        blk[kKryRho1] = 1.0;
        blk[kKryAlpha] = 1.0;
        blk[kKryOmega] = 1.0;
        blk[kKryFlag] = 0.0;
        blk[kKryFlagIt] = 0.0;
    }
    double bb = 0.0, rr = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> gb = ld<T, VEC>(b, j, cnt), gv = ld<T, VEC>(v, j, cnt);
        Grp<T> gr;
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) {
            gr.e[k] = gb.e[k] - gv.e[k];
            if (k < cnt) {
                bb += (double)gb.e[k] * (double)gb.e[k];
                rr += (double)gr.e[k] * (double)gr.e[k];
            }
        }
        st<T, VEC>(r, j, cnt, gr);
        st<T, VEC>(rhat, j, cnt, gr);
    }
    bb = block_sum(bb, lds);
    rr = block_sum(rr, lds);
    put_partial(blk, kKryPartBB, bb);
    put_partial(blk, kKryPartRR, rr);
    put_partial(blk, kKryPartRhR, rr);
}

template <typename T, bool VEC, bool COPY>
__global__ __launch_bounds__(kKryThreads) void kry_p_update(long long n, long long chunk, double *blk, int it,
                                                            const T *__restrict__ r, const T *__restrict__ v,
                                                            T *__restrict__ p, float *__restrict__ copy32) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    const double rho = combine(blk, kKryPartRhR, lds);
    double beta = 0.0, omega = 0.0;
    if (bad_divisor(rho)) {  // the next iteration's divisor (and this one's alpha would be 0)
        set_break(blk, kKryBreakRho, it);
        return;
    }
    if (it > 1) {
        const double rho_old = blk[(it & 1) ? kKryRho0 : kKryRho1];
        const double alpha = blk[kKryAlpha];
        omega = blk[kKryOmega];
        if (bad_divisor(rho_old)) {
            set_break(blk, kKryBreakRho, it);
            return;
        }
        if (bad_divisor(omega)) {
            set_break(blk, kKryBreakOmega, it);
            return;
        }
        beta = (rho / rho_old) * (alpha / omega);
        if (!__builtin_isfinite(beta)) {
            set_break(blk, kKryBreakRho, it);
            return;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) blk[(it & 1) ? kKryRho1 : kKryRho0] = rho;
    const T tb = (T)beta, tw = (T)omega;
    KRY_FOR_GROUPS(T, n, chunk) {
        Grp<T> gp = ld<T, VEC>(r, j, cnt);
        if (it > 1) {
            const Grp<T> go = ld<T, VEC>(p, j, cnt), gv = ld<T, VEC>(v, j, cnt);
#pragma unroll
            for (int k = 0; k < Grp<T>::V; k++) gp.e[k] = gp.e[k] + tb * (go.e[k] - tw * gv.e[k]);
        }
        st<T, VEC>(p, j, cnt, gp);
        if constexpr (COPY) st_copy32<VEC>(copy32, j, cnt, gp);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void kry_dot_rhv(long long n, long long chunk, double *blk,
                                                           const T *__restrict__ rhat, const T *__restrict__ v) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    double acc = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> ga = ld<T, VEC>(rhat, j, cnt), gb = ld<T, VEC>(v, j, cnt);
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++)
            if (k < cnt) acc += (double)ga.e[k] * (double)gb.e[k];
    }
    put_partial(blk, kKryPartRhV, block_sum(acc, lds));
}

template <typename T, bool VEC, bool COPY>
__global__ __launch_bounds__(kKryThreads) void kry_s_update(long long n, long long chunk, double *blk, int it,
                                                            const T *__restrict__ r, const T *__restrict__ v,
                                                            T *__restrict__ s, float *__restrict__ copy32) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    const double rhv = combine(blk, kKryPartRhV, lds);
    if (bad_divisor(rhv)) {
        set_break(blk, kKryBreakRhV, it);
        return;
    }
    const double alpha = blk[(it & 1) ? kKryRho1 : kKryRho0] / rhv;
    if (!__builtin_isfinite(alpha)) {
        set_break(blk, kKryBreakRhV, it);
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) blk[kKryAlpha] = alpha;
    const T ta = (T)alpha;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> gr = ld<T, VEC>(r, j, cnt), gv = ld<T, VEC>(v, j, cnt);
        Grp<T> gs;
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) gs.e[k] = gr.e[k] - ta * gv.e[k];
        st<T, VEC>(s, j, cnt, gs);
        if constexpr (COPY) st_copy32<VEC>(copy32, j, cnt, gs);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void kry_dot_ts(long long n, long long chunk, double *blk,
                                                          const T *__restrict__ t, const T *__restrict__ s) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    double ts = 0.0, tt = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> gt = ld<T, VEC>(t, j, cnt), gs = ld<T, VEC>(s, j, cnt);
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++)
            if (k < cnt) {
                ts += (double)gt.e[k] * (double)gs.e[k];
                tt += (double)gt.e[k] * (double)gt.e[k];
            }
    }
    ts = block_sum(ts, lds);
    tt = block_sum(tt, lds);
    put_partial(blk, kKryPartTS, ts);
    put_partial(blk, kKryPartTT, tt);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void kry_x_update(long long n, long long chunk, double *blk, int it,
                                                            T *__restrict__ x, T *__restrict__ r,
                                                            const T *__restrict__ rhat, const T *__restrict__ s,
                                                            const T *__restrict__ t, const T *__restrict__ phat,
                                                            const T *__restrict__ shat) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    const double ts = combine(blk, kKryPartTS, lds);
    const double tt = combine(blk, kKryPartTT, lds);
    if (!__builtin_isfinite(tt) || !__builtin_isfinite(ts)) {
        set_break(blk, kKryBreakTT, it);
        return;
    }
    const double omega = tt == 0.0 ? 0.0 : ts / tt;  // t == 0: the half step was exact (header)
    if (!__builtin_isfinite(omega)) {
        set_break(blk, kKryBreakTT, it);
        return;
    }
    const double alpha = blk[kKryAlpha];
    if (blockIdx.x == 0 && threadIdx.x == 0) blk[kKryOmega] = omega;
    const T ta = (T)alpha, tw = (T)omega;
    double rhr = 0.0, rr = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        Grp<T> gx = ld<T, VEC>(x, j, cnt);
        const Grp<T> gp = ld<T, VEC>(phat, j, cnt), gh = ld<T, VEC>(shat, j, cnt);
        const Grp<T> gs = ld<T, VEC>(s, j, cnt), gt = ld<T, VEC>(t, j, cnt), gq = ld<T, VEC>(rhat, j, cnt);
        Grp<T> gr;
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) {
            gx.e[k] = (gx.e[k] + ta * gp.e[k]) + tw * gh.e[k];
            gr.e[k] = gs.e[k] - tw * gt.e[k];
            if (k < cnt) {
                rhr += (double)gq.e[k] * (double)gr.e[k];
                rr += (double)gr.e[k] * (double)gr.e[k];
            }
        }
        st<T, VEC>(x, j, cnt, gx);
        st<T, VEC>(r, j, cnt, gr);
    }
    rhr = block_sum(rhr, lds);
    rr = block_sum(rr, lds);
    put_partial(blk, kKryPartRhR, rhr);
    put_partial(blk, kKryPartRR, rr);
}

// dst (fp64) = src (fp32); thread t's groups are float4 -> 2 x double2
template <bool VEC>
__global__ __launch_bounds__(kKryThreads) void kry_widen(long long n, long long chunk, const double *blk,
                                                         const float *__restrict__ src, double *__restrict__ dst) {
    __shared__ double lds[1];
    if (broken(blk, lds)) return;
    KRY_FOR_GROUPS(float, n, chunk) {
        const Grp<float> g = ld<float, VEC>(src, j, cnt);
        Grp<double> lo, hi;
        lo.e[0] = g.e[0];
        lo.e[1] = g.e[1];
        hi.e[0] = g.e[2];
        hi.e[1] = g.e[3];
        st<double, VEC>(dst, j, cnt < 2 ? cnt : 2, lo);
        if (cnt > 2) st<double, VEC>(dst, j + 2, cnt - 2, hi);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void kry_zero(long long n, long long chunk, T *__restrict__ x) {
    KRY_FOR_GROUPS(T, n, chunk) {
        Grp<T> g;
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) g.e[k] = T(0);
        st<T, VEC>(x, j, cnt, g);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void kry_dot(long long n, long long chunk, double *blk,
                                                       const T *__restrict__ x, const T *__restrict__ y) {
    __shared__ double lds[kKryThreads / 64];
    double acc = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> ga = ld<T, VEC>(x, j, cnt), gb = ld<T, VEC>(y, j, cnt);
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++)
            if (k < cnt) acc += (double)ga.e[k] * (double)gb.e[k];
    }
    put_partial(blk, kKryPartRR, block_sum(acc, lds));
}

// ------------------------------------------------------------------- CG
//
// Preconditioned conjugate gradients (rsp_cg_*) for a symmetric positive
// definite A, M = L U as above. An iteration is four launches after the apply
// that leaves z = M^-1 r (three when M = I: z is r, and (r,z) is the (r,r) the
// x-update left):
//
//   cg_dot<RZ>   (r,z)
//   cg_p_update  rho' = (r,z); beta = rho'/rho; p = z + beta p     (it = 1: p = z)
//                                                    -- the SpMV: v = A p --
//   cg_dot<PQ>   (p,v)
//   cg_x_update  alpha = rho'/(p,v); x += alpha p; r -= alpha v [+ fp32 copy]; (r,r)
//
// rho lives in the two parity slots as BiCGStab's: cg_p_update reads the other
// parity's and writes its own, cg_x_update reads that one. Breakdown: rho' or
// (p,v) that is <= 0 or not finite (M or A not positive definite; rho' = 0 is
// also r = 0, which the host's rel <= rtol test sees first) stores a code in
// kKryFlag before anything is written, as above.

__device__ __forceinline__ bool not_positive(double d) { return !(d > 0.0) || !__builtin_isfinite(d); }

template <typename T, bool VEC, bool COPY>
__global__ __launch_bounds__(kKryThreads) void cg_init(long long n, long long chunk, double *blk,
                                                       const T *__restrict__ b, const T *__restrict__ v,
                                                       T *__restrict__ r, float *__restrict__ copy32) {
    __shared__ double lds[kKryThreads / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        blk[kKryRho0] = 1.0;
        blk[kKryRho1] = 1.0;
        blk[kKryAlpha] = 1.0;
        blk[kKryOmega] = 1.0;
        blk[kKryFlag] = 0.0;
        blk[kKryFlagIt] = 0.0;
    }
    double bb = 0.0, rr = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> gb = ld<T, VEC>(b, j, cnt), gv = ld<T, VEC>(v, j, cnt);
        Grp<T> gr;
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) {
            gr.e[k] = gb.e[k] - gv.e[k];
            if (k < cnt) {
                bb += (double)gb.e[k] * (double)gb.e[k];
                rr += (double)gr.e[k] * (double)gr.e[k];
            }
        }
        st<T, VEC>(r, j, cnt, gr);
        if constexpr (COPY) st_copy32<VEC>(copy32, j, cnt, gr);
    }
    bb = block_sum(bb, lds);
    rr = block_sum(rr, lds);
    put_partial(blk, kKryPartBB, bb);
    put_partial(blk, kKryPartRR, rr);
}

template <typename T, bool VEC, int PART>
__global__ __launch_bounds__(kKryThreads) void cg_dot(long long n, long long chunk, double *blk,
                                                      const T *__restrict__ x, const T *__restrict__ y) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    double acc = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> ga = ld<T, VEC>(x, j, cnt), gb = ld<T, VEC>(y, j, cnt);
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++)
            if (k < cnt) acc += (double)ga.e[k] * (double)gb.e[k];
    }
    put_partial(blk, PART, block_sum(acc, lds));
}

// z and p may not alias; z == r (M = I) is read only here. part: where rho' is.
template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void cg_p_update(long long n, long long chunk, double *blk, int it,
                                                           int part, const T *__restrict__ z, T *__restrict__ p) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    const double rho = combine(blk, part, lds);
    if (not_positive(rho)) {
        set_break(blk, kKryBreakCgRZ, it);
        return;
    }
    double beta = 0.0;
    if (it > 1) {
        beta = rho / blk[(it & 1) ? kKryRho0 : kKryRho1];  // (the old rho passed this test an iteration ago)
        if (!__builtin_isfinite(beta)) {
            set_break(blk, kKryBreakCgRZ, it);
            return;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) blk[(it & 1) ? kKryRho1 : kKryRho0] = rho;
    const T tb = (T)beta;
    KRY_FOR_GROUPS(T, n, chunk) {
        Grp<T> gp = ld<T, VEC>(z, j, cnt);
        if (it > 1) {
            const Grp<T> go = ld<T, VEC>(p, j, cnt);
#pragma unroll
            for (int k = 0; k < Grp<T>::V; k++) gp.e[k] = gp.e[k] + tb * go.e[k];
        }
        st<T, VEC>(p, j, cnt, gp);
    }
}

template <typename T, bool VEC, bool COPY>
__global__ __launch_bounds__(kKryThreads) void cg_x_update(long long n, long long chunk, double *blk, int it,
                                                           T *__restrict__ x, T *__restrict__ r,
                                                           const T *__restrict__ p, const T *__restrict__ q,
                                                           float *__restrict__ copy32) {
    __shared__ double lds[kKryThreads / 64];
    if (broken(blk, lds)) return;
    const double pq = combine(blk, kKryPartPQ, lds);
    if (not_positive(pq)) {
        set_break(blk, kKryBreakCgPQ, it);
        return;
    }
    const double alpha = blk[(it & 1) ? kKryRho1 : kKryRho0] / pq;
    if (!__builtin_isfinite(alpha)) {
        set_break(blk, kKryBreakCgPQ, it);
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) blk[kKryAlpha] = alpha;
    const T ta = (T)alpha;
    double rr = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        Grp<T> gx = ld<T, VEC>(x, j, cnt), gr = ld<T, VEC>(r, j, cnt);
        const Grp<T> gp = ld<T, VEC>(p, j, cnt), gq = ld<T, VEC>(q, j, cnt);
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) {
            gx.e[k] = gx.e[k] + ta * gp.e[k];
            gr.e[k] = gr.e[k] - ta * gq.e[k];
            if (k < cnt) rr += (double)gr.e[k] * (double)gr.e[k];
        }
        st<T, VEC>(x, j, cnt, gx);
        st<T, VEC>(r, j, cnt, gr);
        if constexpr (COPY) st_copy32<VEC>(copy32, j, cnt, gr);
    }
    put_partial(blk, kKryPartRR, block_sum(rr, lds));
}

// ---------------------------------------------------------------- GMRES
//
// Restarted flexible GMRES (rsp_gmres_*) and rsp_orthogonalize. Column j of a
// cycle is four launches after the apply and the SpMV that leave w = A z_j:
//
//   gm_multidot   partials of (v_i, w), i <= j
//   gm_update<0>  h = their sums; w -= V h; partials of (v_i, w) again
//   gm_update<1>  h' = their sums; w -= V h'; partial of (w, w)
//   gm_normalise  v_{j+1} = w / ||w|| [+ fp32 copy]; workgroup 0: column h + h',
//                 the rotations, est (rsp::gmres_lsq)
//
// and a cycle ends with gm_combine (x += Z y), the SpMV, gm_resid (w = b - A x)
// and gm_normalise at j = -1 (v_0 = w / ||w||, g = (||w||, 0, ..)).
//
// A workgroup walks its range in sub-chunks of kKryChunk elements: thread t
// keeps its kKryChunk / kKryThreads elements of w in registers (as fp64), so w
// is read once whatever the number of columns, and the columns pass in batches
// of kGmBatch accumulators. A batch is reduced over the workgroup as block_sum
// reduces one value and added to the workgroup's running sums in LDS, one
// thread per column; with the usual single sub-chunk that is the whole dot.
// Updates are accumulated in fp64 and rounded once to T; the second dots read
// the rounded values, i.e. the w that is stored.

constexpr int kGmBatch = 8;
constexpr int kGmElems = kKryChunk / kKryThreads;  // per thread and sub-chunk

// Flag or stop word set: the same for every thread (see broken()).
__device__ __forceinline__ bool halted(const double *blk, double *lds) {
    if (threadIdx.x == 0) lds[0] = (blk[kGmFlag] != 0.0 || blk[kGmStop] != 0.0) ? 1.0 : 0.0;
    __syncthreads();
    const bool h = lds[0] != 0.0;
    __syncthreads();
    return h;
}

__device__ __forceinline__ double *gm_part(double *blk, int arr) {
    return blk + kGmSmall + (size_t)arr * kKryMaxGrid;
}

// Thread t's groups of sub-chunk [s0, s1): q * kKryThreads + t, q < Q.
template <typename T>
struct Sub {
    static constexpr int V = Grp<T>::V, Q = kGmElems / V;
    long long j[Q];
    int cnt[Q];
    __device__ __forceinline__ Sub(long long s0, long long s1) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            j[q] = s0 + ((long long)q * kKryThreads + threadIdx.x) * V;
            const long long left = s1 - j[q];
            cnt[q] = left >= V ? V : (left > 0 ? (int)left : 0);
        }
    }
};

template <typename T, bool VEC>
__device__ __forceinline__ void sub_load(const T *p, const Sub<T> &sb, double (&d)[kGmElems]) {
#pragma unroll
    for (int q = 0; q < Sub<T>::Q; q++) {
        const Grp<T> g = ld<T, VEC>(p, sb.j[q], sb.cnt[q]);  // (cnt 0: zeros, nothing read)
#pragma unroll
        for (int k = 0; k < Sub<T>::V; k++) d[q * Sub<T>::V + k] = (double)g.e[k];
    }
}

// d rounded to T and stored; d becomes the stored values
template <typename T, bool VEC>
__device__ __forceinline__ void sub_store(T *p, const Sub<T> &sb, double (&d)[kGmElems]) {
#pragma unroll
    for (int q = 0; q < Sub<T>::Q; q++) {
        Grp<T> g;
#pragma unroll
        for (int k = 0; k < Sub<T>::V; k++) {
            g.e[k] = (T)d[q * Sub<T>::V + k];
            d[q * Sub<T>::V + k] = (double)g.e[k];
        }
        st<T, VEC>(p, sb.j[q], sb.cnt[q], g);
    }
}

// tot[i] += (v_i, d) over the sub-chunk, i < ncol (elements past the range are
// zero in both). red: 4 * kGmBatch doubles of LDS.
template <typename T, bool VEC>
__device__ __forceinline__ void sub_multidot(const T *V, long long ldv, int ncol, const Sub<T> &sb,
                                             const double (&d)[kGmElems], double *tot, double *red) {
    for (int c0 = 0; c0 < ncol; c0 += kGmBatch) {
        const int nb = ncol - c0 < kGmBatch ? ncol - c0 : kGmBatch;
        double acc[kGmBatch];
#pragma unroll
        for (int b = 0; b < kGmBatch; b++) {
            acc[b] = 0.0;
            if (b < nb) {
                const T *v = V + (long long)(c0 + b) * ldv;
#pragma unroll
                for (int q = 0; q < Sub<T>::Q; q++) {
                    const Grp<T> g = ld<T, VEC>(v, sb.j[q], sb.cnt[q]);
#pragma unroll
                    for (int k = 0; k < Sub<T>::V; k++) acc[b] += (double)g.e[k] * d[q * Sub<T>::V + k];
                }
            }
        }
#pragma unroll
        for (int b = 0; b < kGmBatch; b++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[b] += __shfl_down(acc[b], off, 64);
            if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * kGmBatch + b] = acc[b];
        }
        __syncthreads();
        if ((int)threadIdx.x < nb)
            tot[c0 + threadIdx.x] += ((red[threadIdx.x] + red[kGmBatch + threadIdx.x]) +
                                      red[2 * kGmBatch + threadIdx.x]) + red[3 * kGmBatch + threadIdx.x];
        __syncthreads();
    }
}

// d -= sum_i hs[i] v_i over the sub-chunk, i < ncol, in fp64, i ascending
template <typename T, bool VEC>
__device__ __forceinline__ void sub_update(const T *V, long long ldv, int ncol, const Sub<T> &sb,
                                           double (&d)[kGmElems], const double *hs) {
#pragma unroll 4
    for (int i = 0; i < ncol; i++) {
        const T *v = V + (long long)i * ldv;
        const double h = hs[i];
#pragma unroll
        for (int q = 0; q < Sub<T>::Q; q++) {
            const Grp<T> g = ld<T, VEC>(v, sb.j[q], sb.cnt[q]);
#pragma unroll
            for (int k = 0; k < Sub<T>::V; k++) d[q * Sub<T>::V + k] -= h * (double)g.e[k];
        }
    }
}

// hs[i] = the sum of column i's partials, i < ncol: wave w takes the columns
// w, w + 4, ..; lane l adds part[l], part[l + 64], .. in that order, then the
// 64-lane down-tree. The same in every workgroup.
__device__ __forceinline__ void multi_combine(const double *part0, int ncol, double *hs) {
    const int lane = threadIdx.x & 63, g = (int)gridDim.x;
    for (int i = threadIdx.x >> 6; i < ncol; i += kKryThreads / 64) {
        const double *part = part0 + (size_t)i * kKryMaxGrid;
        double v = 0.0;
        for (int p = lane; p < g; p += 64) v += part[p];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) hs[i] = v;
    }
    __syncthreads();
}

#define GM_RANGE(n, chunk)                                        \
    const long long c0_ = (long long)blockIdx.x * (chunk);        \
    const long long c1_ = c0_ + (chunk) < (n) ? c0_ + (chunk) : (n)
#define GM_FOR_SUBS(T)                                                       \
    for (long long s0_ = c0_; s0_ < c1_; s0_ += kKryChunk)                   \
        if (const Sub<T> sb(s0_, s0_ + kKryChunk < c1_ ? s0_ + kKryChunk : c1_); true)

template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void gm_multidot(long long n, long long chunk, double *blk, int ncol,
                                                           const T *__restrict__ V, long long ldv,
                                                           const T *__restrict__ w) {
    __shared__ double lds[1], tot[kGmLd], red[4 * kGmBatch];
    if (halted(blk, lds)) return;
    if ((int)threadIdx.x < ncol) tot[threadIdx.x] = 0.0;
    __syncthreads();
    GM_RANGE(n, chunk);
    GM_FOR_SUBS(T) {
        double d[kGmElems];
        sub_load<T, VEC>(w, sb, d);
        sub_multidot<T, VEC>(V, ldv, ncol, sb, d, tot, red);
    }
    if ((int)threadIdx.x < ncol) gm_part(blk, kGmPartD1 + threadIdx.x)[blockIdx.x] = tot[threadIdx.x];
}

template <typename T, bool VEC, bool SECOND>
__global__ __launch_bounds__(kKryThreads) void gm_update(long long n, long long chunk, double *blk, int ncol,
                                                         const T *__restrict__ V, long long ldv,
                                                         T *__restrict__ w) {
    __shared__ double lds[kKryThreads / 64], hs[kGmLd], tot[kGmLd], red[4 * kGmBatch];
    if (halted(blk, lds)) return;
    multi_combine(gm_part(blk, SECOND ? kGmPartD2 : kGmPartD1), ncol, hs);
    if ((int)threadIdx.x < ncol) {
        tot[threadIdx.x] = 0.0;
        if (blockIdx.x == 0) blk[(SECOND ? kGmH2 : kGmH1) + threadIdx.x] = hs[threadIdx.x];
    }
    __syncthreads();
    double ww = 0.0;
    GM_RANGE(n, chunk);
    GM_FOR_SUBS(T) {
        double d[kGmElems];
        sub_load<T, VEC>(w, sb, d);
        sub_update<T, VEC>(V, ldv, ncol, sb, d, hs);
        sub_store<T, VEC>(w, sb, d);
        if constexpr (SECOND) {
#pragma unroll
            for (int k = 0; k < kGmElems; k++) ww += d[k] * d[k];
        } else {
            sub_multidot<T, VEC>(V, ldv, ncol, sb, d, tot, red);
        }
    }
    if constexpr (SECOND) {
        ww = block_sum(ww, lds);
        if (threadIdx.x == 0) gm_part(blk, kGmPartNrm)[blockIdx.x] = ww;
    } else {
        if ((int)threadIdx.x < ncol) gm_part(blk, kGmPartD2 + threadIdx.x)[blockIdx.x] = tot[threadIdx.x];
    }
}

// w = b - w, partials of (w, w) and, if FIRST, of (b, b)
template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void gm_resid(long long n, long long chunk, double *blk, int first,
                                                        const T *__restrict__ b, T *__restrict__ w) {
    __shared__ double lds[kKryThreads / 64];
    double bb = 0.0, rr = 0.0;
    KRY_FOR_GROUPS(T, n, chunk) {
        const Grp<T> gb = ld<T, VEC>(b, j, cnt), gv = ld<T, VEC>(w, j, cnt);
        Grp<T> gr;
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) {
            gr.e[k] = gb.e[k] - gv.e[k];
            if (k < cnt) {
                bb += (double)gb.e[k] * (double)gb.e[k];
                rr += (double)gr.e[k] * (double)gr.e[k];
            }
        }
        st<T, VEC>(w, j, cnt, gr);
    }
    rr = block_sum(rr, lds);
    if (threadIdx.x == 0) gm_part(blk, kGmPartRR)[blockIdx.x] = rr;
    if (first) {
        bb = block_sum(bb, lds);
        if (threadIdx.x == 0) gm_part(blk, kGmPartBB)[blockIdx.x] = bb;
    }
}

__device__ __forceinline__ double gm_combine_one(double *blk, int arr, double *lds) {
    const double *part = gm_part(blk, arr);
    const int g = (int)gridDim.x;
    double v = 0.0;
    for (int i = threadIdx.x; i < g; i += kKryThreads) v += part[i];
    return block_sum(v, lds);
}

template <typename T, bool VEC, bool COPY>
__global__ __launch_bounds__(kKryThreads) void gm_normalise(long long n, long long chunk, double *blk, int j,
                                                            int reset, const T *__restrict__ w,
                                                            T *__restrict__ dst, float *__restrict__ copy32) {
    __shared__ double lds[kKryThreads / 64], col[kGmLd + 1], scs[kGmMax], ssn[kGmMax], sg[kGmLd + 1];
    __shared__ int code;
    if (!reset && halted(blk, lds)) return;
    const double nrm = sqrt(gm_combine_one(blk, j < 0 ? kGmPartRR : kGmPartNrm, lds));
    if (j < 0) {
        // cycle start: g = (||r||, 0, ..); a zero or non-finite ||r|| is the host's to see first
        const double bn = sqrt(gm_combine_one(blk, kGmPartBB, lds));
        const bool bad = bad_divisor(nrm);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (reset || bad) {
                blk[kGmFlag] = bad ? (double)kGmBreakNorm : 0.0;
                blk[kGmFlagIt] = 0.0;
            }
            blk[kGmStop] = 0.0;
            blk[kGmDone] = 0.0;
            blk[kGmBeta] = nrm;
            blk[kGmBn] = bn;
            blk[kGmG] = nrm;
        }
        if (bad) return;
    } else if (blockIdx.x == 0) {
        // column j = h + h' with h_{j+1,j} = ||w||: the small step
        const int t = threadIdx.x;
        if (t <= j) {
            col[t] = blk[kGmH1 + t] + blk[kGmH2 + t];
            scs[t] = blk[kGmCs + t];
            ssn[t] = blk[kGmSn + t];
        }
        if (t == j + 1) col[t] = nrm;
        if (t == 0) sg[j] = blk[kGmG + j];
        __syncthreads();
        if (t == 0) {
            code = gmres_lsq(col, j, scs, ssn, sg, nullptr, 0, 0, nullptr);
            if (code) {
                blk[kGmFlag] = (double)code;
                blk[kGmFlagIt] = (double)j;
            } else {
                blk[kGmG + j] = sg[j];
                blk[kGmG + j + 1] = sg[j + 1];
                blk[kGmCs + j] = scs[j];
                blk[kGmSn + j] = ssn[j];
                blk[kGmEst + j] = fabs(sg[j + 1]) / blk[kGmBn];
                blk[kGmDone] = (double)(j + 1);
                if (nrm == 0.0) blk[kGmStop] = 1.0;
            }
        }
        __syncthreads();
        if (code == 0 && t <= j) blk[kGmR + (size_t)j * kGmLd + t] = col[t];
    }
    if (j >= 0 && bad_divisor(nrm)) return;  // nothing to normalise: the exact solve, or a breakdown
    KRY_FOR_GROUPS(T, n, chunk) {
        Grp<T> g = ld<T, VEC>(w, j, cnt);
#pragma unroll
        for (int k = 0; k < Grp<T>::V; k++) g.e[k] = (T)((double)g.e[k] / nrm);
        st<T, VEC>(dst, j, cnt, g);
        if constexpr (COPY) st_copy32<VEC>(copy32, j, cnt, g);
    }
}

// x += sum_i y_i z_i over the completed columns (kGmDone), y from R y = g.
// Runs whatever the flag says: a breakdown at column j leaves the j columns
// before it to be added. A non-finite y adds nothing.
template <typename T, bool VEC>
__global__ __launch_bounds__(kKryThreads) void gm_combine(long long n, long long chunk, double *blk,
                                                          const T *__restrict__ Z, long long ldz,
                                                          T *__restrict__ x) {
    __shared__ double R[kGmLd * kGmMax], g[kGmLd], y[kGmMax];
    __shared__ int ok;
    const int k = (int)blk[kGmDone];
    if (k <= 0 || k > kGmMax) return;
    for (int i = threadIdx.x; i < k * kGmLd; i += kKryThreads) R[i] = blk[kGmR + i];
    if ((int)threadIdx.x < k) g[threadIdx.x] = blk[kGmG + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        gmres_lsq(nullptr, 0, nullptr, nullptr, g, R, kGmLd, k, y);
        bool fin = true;
        for (int i = 0; i < k; i++) fin = fin && __builtin_isfinite(y[i]);
        ok = fin;
        if (blockIdx.x == 0) {
            if (fin) {
                for (int i = 0; i < k; i++) blk[kGmY + i] = y[i];
            } else if (blk[kGmFlag] == 0.0) {
                blk[kGmFlag] = (double)kGmBreakY;
                blk[kGmFlagIt] = 0.0;
                blk[kGmDone] = 0.0;
            }
        }
    }
    __syncthreads();
    if (!ok) return;
    GM_RANGE(n, chunk);
    GM_FOR_SUBS(T) {
        double d[kGmElems];
        sub_load<T, VEC>(x, sb, d);
#pragma unroll 4
        for (int i = 0; i < k; i++) {
            const T *z = Z + (long long)i * ldz;
            const double yi = y[i];
#pragma unroll
            for (int q = 0; q < Sub<T>::Q; q++) {
                const Grp<T> gz = ld<T, VEC>(z, sb.j[q], sb.cnt[q]);
#pragma unroll
                for (int e = 0; e < Sub<T>::V; e++) d[q * Sub<T>::V + e] += yi * (double)gz.e[e];
            }
        }
        sub_store<T, VEC>(x, sb, d);
    }
}

// -------------------------------------------------- iterative refinement
//
// Mixed-precision refinement (rsp_refine_*) and its building blocks
// (rsp_convert_scaled, rsp_refine_update). A step's residual r = b - A x is
// cg_init at fp64; the two kernels between it and the fp32 inner solve are
//
//   ref_convert<double, float, ZERO>  r32 = fp32(r * 2^-e), d = 0   (8n read, 8n written)
//   ref_update                        x_old = x; x = x + 2^e * double(d)
//
// scale = 2^exp2 is an fp64 value and every product with it is exact short of
// fp64's range, so an element is rounded once, to its destination type (to
// nearest even: the conversion's and the addition's own rounding). A thread
// moves four elements per step whatever the types: one float4, or two double2.
// In the FTZ build an fp32 denormal read counts as a zero of its sign and an
// fp32 result that is denormal after rounding becomes one, decided on the fp64
// value, so no conversion instruction's own denormal mode is relied on.

__device__ __forceinline__ double ref_widen(float s) {
#ifdef RSP_FTZ_BUILD
    if (__builtin_fabsf(s) < 0x1p-126f) s = __builtin_copysignf(0.0f, s);
#endif
    return (double)s;
}

template <typename D>
__device__ __forceinline__ D ref_narrow(double v);
template <>
__device__ __forceinline__ double ref_narrow<double>(double v) {
    return v;
}
template <>
__device__ __forceinline__ float ref_narrow<float>(double v) {
    float f = (float)v;
#ifdef RSP_FTZ_BUILD
    // below 2^-126 - 2^-150 the rounded value is denormal (the tie rounds to the even 2^-126)
    const double a = __builtin_fabs(v);
    if (a < 0x1p-126) f = __builtin_copysignf(a >= 0x1p-126 - 0x1p-150 ? 0x1p-126f : 0.0f, f);
#endif
    return f;
}

// four elements at j (cnt of them in range) as fp64, and back
template <typename T, bool VEC>
__device__ __forceinline__ void ref_ld4(const T *p, long long j, int cnt, double (&out)[4]) {
    if constexpr (sizeof(T) == 4) {
        const Grp<T> g = ld<T, VEC>(p, j, cnt);
#pragma unroll
        for (int k = 0; k < 4; k++) out[k] = ref_widen(g.e[k]);
    } else {
        const Grp<T> lo = ld<T, VEC>(p, j, cnt < 2 ? cnt : 2);
        Grp<T> hi;
        hi.e[0] = hi.e[1] = T(0);
        if (cnt > 2) hi = ld<T, VEC>(p, j + 2, cnt - 2);
        out[0] = lo.e[0];
        out[1] = lo.e[1];
        out[2] = hi.e[0];
        out[3] = hi.e[1];
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void ref_st4(T *p, long long j, int cnt, const T (&v)[4]) {
    if constexpr (sizeof(T) == 4) {
        Grp<T> g;
#pragma unroll
        for (int k = 0; k < 4; k++) g.e[k] = v[k];
        st<T, VEC>(p, j, cnt, g);
    } else {
        Grp<T> lo, hi;
        lo.e[0] = v[0];
        lo.e[1] = v[1];
        hi.e[0] = v[2];
        hi.e[1] = v[3];
        st<T, VEC>(p, j, cnt < 2 ? cnt : 2, lo);
        if (cnt > 2) st<T, VEC>(p, j + 2, cnt - 2, hi);
    }
}

// dst = D(src * scale) [ZERO: and zero = 0]. src == dst is allowed (S == D): a
// thread reads its four elements before it writes them, so no __restrict__.
template <typename S, typename D, bool VEC, bool ZERO>
__global__ __launch_bounds__(kKryThreads) void ref_convert(long long n, long long chunk, double scale, const S *src,
                                                           D *dst, float *zero) {
    KRY_FOR_GROUPS(float, n, chunk) {
        double w[4];
        ref_ld4<S, VEC>(src, j, cnt, w);
        D o[4];
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = ref_narrow<D>(w[k] * scale);
        ref_st4<D, VEC>(dst, j, cnt, o);
        if constexpr (ZERO) {
            const float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            ref_st4<float, VEC>(zero, j, cnt, z);
        }
    }
}

// x_old = x (SAVE); x = x + scale * double(d)
template <bool VEC, bool SAVE>
__global__ __launch_bounds__(kKryThreads) void ref_update(long long n, long long chunk, double scale,
                                                          const float *__restrict__ d, double *__restrict__ x,
                                                          double *__restrict__ x_old) {
    KRY_FOR_GROUPS(float, n, chunk) {
        double dd[4], xx[4];
        ref_ld4<float, VEC>(d, j, cnt, dd);
        ref_ld4<double, VEC>(x, j, cnt, xx);
        if constexpr (SAVE) ref_st4<double, VEC>(x_old, j, cnt, xx);
#pragma unroll
        for (int k = 0; k < 4; k++) xx[k] = xx[k] + scale * dd[k];
        ref_st4<double, VEC>(x, j, cnt, xx);
    }
}

template <typename T, bool COPY>
hipError_t launch(KryOp op, const KryArgs &a, hipStream_t s) {
    const KryGrid kg = kry_grid(a.n);
    const dim3 grid(kg.grid), block(kKryThreads);
    const long long n = a.n, ch = kg.chunk;
    const T *b = (const T *)a.b, *c = (const T *)a.c, *phat = (const T *)a.phat, *shat = (const T *)a.shat,
            *z = (const T *)a.z;
    T *x = (T *)a.x, *r = (T *)a.r, *rhat = (T *)a.rhat, *p = (T *)a.p, *v = (T *)a.v, *sv = (T *)a.s,
      *t = (T *)a.t;
    float *c32 = (float *)a.copy32;
#define KRY_LAUNCH(ALIGNED, KERN, KERN_U, ...)                                           \
    do {                                                                                 \
        if (ALIGNED)                                                                     \
            hipLaunchKernelGGL(KERN, grid, block, 0, s, __VA_ARGS__);                    \
        else                                                                             \
            hipLaunchKernelGGL(KERN_U, grid, block, 0, s, __VA_ARGS__);                  \
    } while (0)
    switch (op) {
        case kKryInit:
            KRY_LAUNCH(aligned16({b, v, r, rhat}), (kry_init<T, true>), (kry_init<T, false>), n, ch, a.blk, b,
                       (const T *)v, r, rhat);
            break;
        case kKryPUpdate:
            KRY_LAUNCH(aligned16({r, v, p, c32}), (kry_p_update<T, true, COPY>), (kry_p_update<T, false, COPY>), n,
                       ch, a.blk, a.it, (const T *)r, (const T *)v, p, c32);
            break;
        case kKryDotRhV:
            KRY_LAUNCH(aligned16({rhat, v}), (kry_dot_rhv<T, true>), (kry_dot_rhv<T, false>), n, ch, a.blk,
                       (const T *)rhat, (const T *)v);
            break;
        case kKrySUpdate:
            KRY_LAUNCH(aligned16({r, v, sv, c32}), (kry_s_update<T, true, COPY>), (kry_s_update<T, false, COPY>), n,
                       ch, a.blk, a.it, (const T *)r, (const T *)v, sv, c32);
            break;
        case kKryDotTS:
            KRY_LAUNCH(aligned16({t, sv}), (kry_dot_ts<T, true>), (kry_dot_ts<T, false>), n, ch, a.blk,
                       (const T *)t, (const T *)sv);
            break;
        case kKryXUpdate:
            KRY_LAUNCH(aligned16({x, r, rhat, sv, t, phat, shat}), (kry_x_update<T, true>),
                       (kry_x_update<T, false>), n, ch, a.blk, a.it, x, r, (const T *)rhat, (const T *)sv,
                       (const T *)t, phat, shat);
            break;
        case kKryZero:
            KRY_LAUNCH(aligned16({x}), (kry_zero<T, true>), (kry_zero<T, false>), n, ch, x);
            break;
        case kKryDot:
            KRY_LAUNCH(aligned16({b, c}), (kry_dot<T, true>), (kry_dot<T, false>), n, ch, a.blk, b, c);
            break;
        case kKryCgInit:
            KRY_LAUNCH(aligned16({b, v, r, c32}), (cg_init<T, true, COPY>), (cg_init<T, false, COPY>), n, ch, a.blk,
                       b, (const T *)v, r, c32);
            break;
        case kKryCgDotRZ:
            KRY_LAUNCH(aligned16({r, z}), (cg_dot<T, true, kKryPartRZ>), (cg_dot<T, false, kKryPartRZ>), n, ch,
                       a.blk, (const T *)r, z);
            break;
        case kKryCgPUpdate:
            KRY_LAUNCH(aligned16({z, p}), (cg_p_update<T, true>), (cg_p_update<T, false>), n, ch, a.blk, a.it,
                       (int)(z == r ? kKryPartRR : kKryPartRZ), z, p);
            break;
        case kKryCgDotPQ:
            KRY_LAUNCH(aligned16({p, v}), (cg_dot<T, true, kKryPartPQ>), (cg_dot<T, false, kKryPartPQ>), n, ch,
                       a.blk, (const T *)p, (const T *)v);
            break;
        case kKryCgXUpdate:
            KRY_LAUNCH(aligned16({x, r, p, v, c32}), (cg_x_update<T, true, COPY>), (cg_x_update<T, false, COPY>), n,
                       ch, a.blk, a.it, x, r, (const T *)p, (const T *)v, c32);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename T, bool COPY>
hipError_t gm_launch(GmOp op, const GmArgs &a, hipStream_t s) {
    const KryGrid kg = kry_grid(a.n);
    const dim3 grid(kg.grid), block(kKryThreads);
    const long long n = a.n, ch = kg.chunk;
    const T *V = (const T *)a.V, *Z = (const T *)a.Z, *b = (const T *)a.b;
    T *w = (T *)a.w, *x = (T *)a.x;
    float *c32 = (float *)a.copy32;
    const int ncol = a.j + 1;
    // a column base is 16-byte aligned when the first is and the stride is whole groups
    const bool vstride = (a.ldv * (long long)sizeof(T)) % 16 == 0, zstride = (a.ldz * (long long)sizeof(T)) % 16 == 0;
    switch (op) {
        case kGmResid:
            KRY_LAUNCH(aligned16({b, w}), (gm_resid<T, true>), (gm_resid<T, false>), n, ch, a.blk, a.first, b, w);
            break;
        case kGmNormalise: {
            if (a.j < -1 || a.j >= kGmMax) return hipErrorInvalidValue;
            T *dst = (T *)a.V + (long long)(a.j + 1) * a.ldv;
            KRY_LAUNCH(aligned16({w, dst, c32}), (gm_normalise<T, true, COPY>), (gm_normalise<T, false, COPY>), n,
                       ch, a.blk, a.j, a.first, (const T *)w, dst, c32);
            break;
        }
        case kGmMultiDot:
            if (ncol < 1 || ncol > kGmLd) return hipErrorInvalidValue;
            KRY_LAUNCH(vstride && aligned16({V, w}), (gm_multidot<T, true>), (gm_multidot<T, false>), n, ch, a.blk,
                       ncol, V, a.ldv, (const T *)w);
            break;
        case kGmUpdate1:
            if (ncol < 1 || ncol > kGmLd) return hipErrorInvalidValue;
            KRY_LAUNCH(vstride && aligned16({V, w}), (gm_update<T, true, false>), (gm_update<T, false, false>), n,
                       ch, a.blk, ncol, V, a.ldv, w);
            break;
        case kGmUpdate2:
            if (ncol < 1 || ncol > kGmLd) return hipErrorInvalidValue;
            KRY_LAUNCH(vstride && aligned16({V, w}), (gm_update<T, true, true>), (gm_update<T, false, true>), n, ch,
                       a.blk, ncol, V, a.ldv, w);
            break;
        case kGmCombine:
            KRY_LAUNCH(zstride && aligned16({Z, x}), (gm_combine<T, true>), (gm_combine<T, false>), n, ch, a.blk, Z,
                       a.ldz, x);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename S, typename D>
hipError_t ref_convert_launch(const RefArgs &a, bool zero, hipStream_t s) {
    const KryGrid kg = kry_grid(a.n);
    const dim3 grid(kg.grid), block(kKryThreads);
    const S *src = (const S *)a.src;
    D *dst = (D *)a.dst;
    if (zero) {
        if constexpr (sizeof(S) == 8 && sizeof(D) == 4)
            KRY_LAUNCH(aligned16({src, dst, a.zero}), (ref_convert<S, D, true, true>),
                       (ref_convert<S, D, false, true>), a.n, kg.chunk, a.scale, src, dst, a.zero);
        else
            return hipErrorInvalidValue;
    } else {
        KRY_LAUNCH(aligned16({src, dst}), (ref_convert<S, D, true, false>), (ref_convert<S, D, false, false>), a.n,
                   kg.chunk, a.scale, src, dst, (float *)nullptr);
    }
    return hipGetLastError();
}

hipError_t ref_launch(RefOp op, const RefArgs &a, hipStream_t s) {
    switch (op) {
        case kRefConvert:
            if (a.src_f32)
                return a.dst_f32 ? ref_convert_launch<float, float>(a, false, s)
                                 : ref_convert_launch<float, double>(a, false, s);
            return a.dst_f32 ? ref_convert_launch<double, float>(a, false, s)
                             : ref_convert_launch<double, double>(a, false, s);
        case kRefNarrowZero:
            return ref_convert_launch<double, float>(a, true, s);
        case kRefUpdate: {
            const KryGrid kg = kry_grid(a.n);
            const dim3 grid(kg.grid), block(kKryThreads);
            const float *d = (const float *)a.src;
            double *x = (double *)a.dst;
            if (a.x_old)
                KRY_LAUNCH(aligned16({d, x, a.x_old}), (ref_update<true, true>), (ref_update<false, true>), a.n,
                           kg.chunk, a.scale, d, x, a.x_old);
            else
                KRY_LAUNCH(aligned16({d, x}), (ref_update<true, false>), (ref_update<false, false>), a.n, kg.chunk,
                           a.scale, d, x, (double *)nullptr);
            return hipGetLastError();
        }
        default:
            return hipErrorInvalidValue;
    }
}
#undef KRY_LAUNCH

}  // namespace

hipError_t refine(RefOp op, const RefArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    return ref_launch(op, a, s);
}

hipError_t gmres(GmOp op, int type, const GmArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    switch (type) {
        case kKryF32: return gm_launch<float, false>(op, a, s);
        case kKryF64Copy32: return gm_launch<double, true>(op, a, s);
#ifndef RSP_FTZ_BUILD
        case kKryF64: return gm_launch<double, false>(op, a, s);
#endif
        default: return hipErrorInvalidValue;
    }
}

hipError_t krylov(KryOp op, int type, const KryArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (op == kKryWiden) {
        const KryGrid kg = kry_grid(a.n);
        if (aligned16({a.b, a.copy32}))
            hipLaunchKernelGGL((kry_widen<true>), dim3(kg.grid), dim3(kKryThreads), 0, s, a.n, kg.chunk,
                               (const double *)a.blk, (const float *)a.b, (double *)a.copy32);
        else
            hipLaunchKernelGGL((kry_widen<false>), dim3(kg.grid), dim3(kKryThreads), 0, s, a.n, kg.chunk,
                               (const double *)a.blk, (const float *)a.b, (double *)a.copy32);
        return hipGetLastError();
    }
    switch (type) {
        case kKryF32: return launch<float, false>(op, a, s);
        case kKryF64Copy32: return launch<double, true>(op, a, s);
#ifndef RSP_FTZ_BUILD
        case kKryF64: return launch<double, false>(op, a, s);
#endif
        default: return hipErrorInvalidValue;
    }
}

void warm_krylov() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(kry_dot<float, true>));
    int o = 0;  // (the use that loads the code object, as warm_spmv)
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kry_dot<float, true>, kKryThreads, 0);
}

}  // namespace RSP_KNS
