// spmv.hip — CSR SpMV y = alpha*A*x + beta*y for gfx950 (MI355X), fp64 and
// fp32 (fp32 storage AND accumulation, as cusparseSpMV with CUDA_R_32F,
// GPU/spmv.cu:131-145,179-181). Replaces cusparseSpMV (GPU/spmv.cu:148-186).
//
// Schedule ("row-block" tiles, built once per matrix by rsp_spmv_buffer_size /
// rsp_spmv_preprocess into the matrix's own device memory):
// consecutive rows are packed into tiles of at most SpmvTile<T>::kMaxNnz
// entries (<= SpmvTile<T>::kMaxRows rows); one 256-thread workgroup per tile.
//   1. stream: each thread issues all of its 16-byte colidx/vals loads for
//      the tile back to back (predicated, no per-element branches, so every
//      load is in flight before the first wait), then all its x[col] gathers,
//      then writes the products into LDS (16 KiB per tile);
//   2. reduce: L = 1, 2, 4 or 8 lanes per row sum the row's products from
//      LDS in the CANONICAL 8-WAY ORDER — partial p_j adds the products
//      e = j, j+8, ... (e counted from the row start) in order, then
//      y = ((p0+p4)+(p2+p6)) + ((p1+p5)+(p3+p7)) — which every L realises
//      exactly (local tree stages for offsets >= L, shuffles below). So y is
//      bitwise independent of how rows are packed into tiles or split over
//      GPUs, and equal to the oracle's oracle_spmv_canon_* bit for bit.
// Rows longer than a tile are cut into tile-sized chunks (relative to the row
// start); each chunk is reduced by all 256 threads in a fixed tree, and the
// chunk that arrives last adds the chunk partials in order (longrow_arrive;
// RSP_SPMV_VARIANT bit 8 uses a separate fixup launch instead). Everything is
// deterministic.
//
// Roofline: HBM-bound, no MFMA (no dense contraction). Algorithmic bytes per
// call: (sizeof(T)+4)*nnz_s + 4*(m+1) + sizeof(T)*(n + m) (+ sizeof(T)*m if
// beta != 0); see DESIGN.md.
//
// Compiled twice: namespace rsp_k (fp64 + fp32) and rsp_k_ftz (fp32 only,
// -fgpu-flush-denormals-to-zero), see rsp_kernels.h.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rsp_kernels.h"
#include "spmv_pack.h"

#ifndef RSP_KNS
#define RSP_KNS rsp_k
#endif

#ifndef RSP_NT_Y
#define RSP_NT_Y -1  // y stores: 1 non-temporal, 0 plain, -1 (shipped) non-temporal for fp64 only (A/B)
#endif

namespace RSP_KNS {

using rsp::kSpmvThreads;
using rsp::kSpmvHeavyMax;
using rsp::SpmvArgs;
using rsp::SpmvBlock;
using rsp::SpmvLongRow;
using rsp::SpmvTile;
using rsp::kSpmvBatchMax;
using rsp::SpmvBatchArgs;
using rsp::SpmvBatchEntry;
using rsp::SpmvBatchTable;

template <typename T, int N>
struct VecT;
template <>
struct VecT<double, 2> {
    typedef double __attribute__((ext_vector_type(2))) V;
    typedef int __attribute__((ext_vector_type(2))) I;
    typedef unsigned short __attribute__((ext_vector_type(2))) H;
};
template <>
struct VecT<float, 4> {
    typedef float __attribute__((ext_vector_type(4))) V;
    typedef int __attribute__((ext_vector_type(4))) I;
    typedef unsigned short __attribute__((ext_vector_type(4))) H;
};

// Logical tile for workgroup `bid`: each of the 8 XCDs (round-robin dispatch)
// gets a contiguous run of tiles, so neighbouring row blocks — which gather
// overlapping parts of x — share one L2 (guide T1, bijective form).
__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

template <bool NT, typename P>
__device__ __forceinline__ P ld(const P *p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

// Products of entries [k0, k1) into lds[e - kb], kb = k0 rounded down to the
// vector width. Every load is unpredicated: a vector past k1 re-reads the
// tile's last vector (an L1 hit), so the loads, then the gathers, issue back
// to back with no exec-masked blocks between them (a predicated load makes
// hipcc drain vmcnt before each later gather). Partial vectors at either end
// touch in-bounds neighbours whose LDS slots are never read. Requires a
// non-empty tile whose last vector does not straddle the end of the arrays
// (the caller takes stream_products_scalar otherwise).
// C16: the column indices come from the schedule's 16-bit copy, col = cbase
// + off (the tile's columns span < 65536; rsp_spmv_preprocess): 2 B instead
// of 4 B per entry. A partial vector's neighbour entries belong to another
// tile and another base, so their decoded column is clamped to cmax = n - 1
// (in bounds; their products are never read).
template <typename T, bool NT, bool C16 = false, int NTH = kSpmvThreads,
          int IT = SpmvTile<T>::kSlots / (kSpmvThreads * (16 / sizeof(T)))>
__device__ __forceinline__ void stream_products(const int *__restrict__ colidx,
                                                const unsigned short *__restrict__ cidx, int cbase,
                                                int cmax, const T *__restrict__ vals,
                                                const T *__restrict__ x, int kb, int k1,
                                                T *__restrict__ lds) {
    constexpr int VW = 16 / sizeof(T);
    typedef typename VecT<T, VW>::V V;
    typedef typename VecT<T, VW>::I I;
    typedef typename VecT<T, VW>::H H;
    const int tid = threadIdx.x;
    const int last = (k1 - 1) & ~(VW - 1);
    I ci[IT];
    H ch[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int e = min(kb + (it * NTH + tid) * VW, last);
        if constexpr (C16)
            ch[it] = ld<NT>(reinterpret_cast<const H *>(cidx + e));
        else
            ci[it] = ld<NT>(reinterpret_cast<const I *>(colidx + e));
    }
    V vv[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int e = min(kb + (it * NTH + tid) * VW, last);
        vv[it] = ld<NT>(reinterpret_cast<const V *>(vals + e));
    }
    // keep the scheduler from splitting the load and gather bursts: two
    // memory round trips per tile, not one per vector
    __builtin_amdgcn_sched_barrier(0);
    T xv[IT][VW];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            int c;
            if constexpr (C16)
                c = min(cbase + (int)ch[it][j], cmax);
            else
                c = ci[it][j];
            xv[it][j] = x[c];
        }
    __builtin_amdgcn_sched_barrier(0);
    // every slot (it*256 + tid)*VW lies inside the tile's LDS image, so the
    // stores are unpredicated too; slots at or past k1 - kb are never read
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        V p;
#pragma unroll
        for (int j = 0; j < VW; ++j) p[j] = vv[it][j] * xv[it][j];
        *reinterpret_cast<V *>(lds + (it * NTH + tid) * VW) = p;
    }
}

// LDS-only workgroup barrier: orders LDS traffic and leaves global stores in
// flight (__syncthreads() waits vmcnt(0), i.e. for the previous tile's y
// stores to be acknowledged).
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// A STAGED tile (round 4; plan: spmv_plan.cpp encode_columns). Gathering x
// lane by lane costs the vector-memory path about one TA cycle per lane —
// the bound of the plain tile (counters) — while a mesh tile's
// 2-4 k entries read only ~900-1600 distinct columns, in a few contiguous
// runs. So the tile's distinct columns are loaded once into its LDS image
// (coalesced loads along each run), and every entry reads its x from there
// by a 16-bit slot index (stored where the C16 tiles keep column offsets).
// Sequence: the run descriptors (loaded first, by the caller) go to a table
// at the END of the LDS image; each thread finds the run of its slots
// u = tid + 256 k by a binary search in that table (all k together, one LDS
// round trip per step) and loads x of those columns — while the tile's
// stream loads are still in flight; x goes to LDS slots [0, U); then the
// entries' x are read from LDS (slot clamped to U - 1: a partial vector's
// neighbour entries carry another tile's indices; their products are never
// read), and after a barrier the products overwrite the image as usual.
// Same products, same order: the same bits as the gathered tile.
// PACKED tiles (PK; spmv_pack.h): the slot indices
// are 12-bit fields of the tile's own record, NW words per thread (one 12-byte
// load for fp64, 16 + 8 bytes for fp32) instead of IT 16-bit vectors from
// cidx: 1.5 B per slot of the image instead of 2 B per entry. The words are
// loaded ahead of the values like the 16-bit vectors and decoded after the
// loads' burst; fields of slots outside [k0, k1) are 0. PKM 1 / 0: the packed
// / unpacked form as an instantiation of its own, chosen by the caller's
// workgroup-uniform branch (fp64), so neither form's loads meet the other's
// registers at a join — which makes hipcc drain vmcnt in front of the later
// form's loads, 5 % of the big set's launch. PKM 2: one instantiation that
// tests pk (fp32, where two cost 73 VGPRs and a wave per SIMD; its unpacked
// staged tiles are the few short ones).
template <typename T, bool NT, int PKM, int NTH = kSpmvThreads,
          int IT = SpmvTile<T>::kSlots / (kSpmvThreads * (16 / sizeof(T)))>
__device__ __forceinline__ void stream_products_staged(const unsigned short *__restrict__ cidx,
                                                       const unsigned int *__restrict__ pk, int2 rd,
                                                       int nr, const int (&lsl)[SpmvTile<T>::kStageSlots / NTH],
                                                       const T *__restrict__ vals,
                                                       const T *__restrict__ x, int kb, int k1,
                                                       T *__restrict__ lds) {
    constexpr int VW = 16 / sizeof(T);
    constexpr int SMAX = SpmvTile<T>::kStageSlots / NTH;
    typedef typename VecT<T, VW>::V V;
    const int tid = threadIdx.x;
    const int last = (k1 - 1) & ~(VW - 1);
    // the tile's index words: IT 16-bit vectors (two slots per word), or the
    // NW words of the packed record — one register array for both forms
    constexpr int NW = rsp_pack::words_per_thread(IT * VW);
    constexpr int HW = VW / 2;  // words per 16-bit vector
    static_assert(NW <= IT * HW, "the packed words fit the unpacked ones' registers");
    const bool pkd = PKM == 2 ? pk != nullptr : PKM == 1;
    unsigned int iw[PKM == 1 ? NW : IT * HW];
    V vv[IT];
    if (pkd) {
        const unsigned int *w = pk + tid * NW;
#pragma unroll
        for (int q = 0; q < NW; ++q) iw[q] = ld<NT>(w + q);
    } else {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int e = min(kb + (it * NTH + tid) * VW, last);
            const unsigned int *w = reinterpret_cast<const unsigned int *>(cidx + e);
#pragma unroll
            for (int q = 0; q < HW; ++q) iw[it * HW + q] = ld<NT>(w + q);
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int e = min(kb + (it * NTH + tid) * VW, last);
        vv[it] = ld<NT>(reinterpret_cast<const V *>(vals + e));
    }
    __builtin_amdgcn_sched_barrier(0);
    // x through a buffer resource: 32-bit byte offsets instead of 64-bit
    // addresses (fewer VGPRs; num_records covers the whole of x)
    const __amdgpu_buffer_rsrc_t xr =
        __builtin_amdgcn_make_buffer_rsrc((void *)x, (short)0, 0x7ffffffc, 0x00020000);
    auto xload = [&](int col) {
        if constexpr (sizeof(T) == 8)
            return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(xr, col * 8, 0, 0));
        else
            return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(xr, col * 4, 0, 0));
    };
    T xs[SMAX];
    int U;
    if (SpmvTile<T>::kStageList && nr == 255) {  // list mode (workgroup-uniform): the slots' columns came with the tile
        U = rd.y;
#pragma unroll
        for (int k = 0; k < SMAX; ++k)
            if (k * NTH < U) xs[k] = xload(rd.x + lsl[k]);
    } else {  // runs mode: the run table at the end of the LDS image, a search per slot
        // The table (nr <= kStageRuns descriptors and the sentinel, 8 B each)
        // ends with the image and starts at element kSlots - 255 = 1793 (fp64)
        // or kSlots - 2 * 255 = 3586 (fp32) at the lowest; the x staged below
        // fills elements [0, U), U <= kStageSlots = 1536 / 2048: they never meet.
        static_assert(SpmvTile<T>::kStageSlots * sizeof(T) + (rsp::kStageRuns + 1) * sizeof(int2) <=
                          SpmvTile<T>::kSlots * sizeof(T),
                      "the run table lies past the staged x in the LDS image");
        static_assert(rsp::kStageRuns + 1 <= NTH, "one thread per run descriptor and the sentinel");
        int2 *tab = reinterpret_cast<int2 *>(lds + SpmvTile<T>::kSlots) - (nr + 1);
        if (tid <= nr) tab[tid] = rd;
        lds_barrier();
        U = tab[nr].y;
        int us[SMAX], lo[SMAX];
#pragma unroll
        for (int k = 0; k < SMAX; ++k) {
            us[k] = min(k * NTH + tid, U - 1);
            lo[k] = 0;
        }
        for (int n = nr; n > 1;) {  // largest r with tab[r].y <= u (tab[0].y = 0); nr is uniform
            const int h = n >> 1;
#pragma unroll
            for (int k = 0; k < SMAX; ++k)
                if (tab[lo[k] + h].y <= us[k]) lo[k] += h;
            n -= h;
        }
#pragma unroll
        for (int k = 0; k < SMAX; ++k)
            if (k * NTH < U) {  // workgroup-uniform
                const int2 r = tab[lo[k]];
                xs[k] = xload(r.x + (us[k] - r.y));
            }
    }
#pragma unroll
    for (int k = 0; k < SMAX; ++k)
        if (k * NTH < U && k * NTH + tid < U) lds[k * NTH + tid] = xs[k];
    lds_barrier();
    T xv[IT][VW];
    if (pkd) {
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int j = 0; j < VW; ++j) xv[it][j] = lds[min((int)rsp_pack::get_field(iw, it * VW + j), U - 1)];
    } else {
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int j = 0; j < VW; ++j)
                xv[it][j] = lds[min((int)((iw[(it * VW + j) >> 1] >> (16 * (j & 1))) & 0xffffu), U - 1)];
    }
    lds_barrier();  // every x read before the products overwrite the image
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        V p;
#pragma unroll
        for (int j = 0; j < VW; ++j) p[j] = vv[it][j] * xv[it][j];
        *reinterpret_cast<V *>(lds + (it * NTH + tid) * VW) = p;
    }
}

// Element-wise variant for a tile that touches the end of the arrays (at
// most one per call) or unaligned arrays.
template <typename T, int NTH = kSpmvThreads>
__device__ __forceinline__ void stream_products_scalar(const int *__restrict__ colidx,
                                                       const T *__restrict__ vals,
                                                       const T *__restrict__ x, int k0, int kb,
                                                       int k1, T *lds) {
    for (int e = kb + (int)threadIdx.x; e < k1; e += NTH)
        if (e >= k0) lds[e - kb] = vals[e] * x[colidx[e]];
}

// Rows [0, nrows) of a tile, L lanes per row, canonical 8-way order; the
// row sum goes to sink(row, sum) (lane 0 of the row's group). A row longer
// than `heavy` entries (heavy > 0) is not summed here but listed in
// hl[0 .. *hn) for reduce_heavy_rows.
template <typename T, int L, int NTH, typename Sink>
__device__ __forceinline__ void reduce_rows(const T *lds, const unsigned short *rp_lds, int nrows, int kb,
                                            int heavy, int *hl, int *hn, Sink sink) {
    constexpr int NA = 8 / L;                  // partials held per lane
    constexpr int NG = NTH / L;                // row groups per pass
    const int tid = threadIdx.x;
    const int g = tid / L, lane = tid & (L - 1);
    for (int rr = g; rr - g < nrows; rr += NG) {  // same trip count for all groups
        bool active = rr < nrows;
        T acc[NA];
#pragma unroll
        for (int t = 0; t < NA; ++t) acc[t] = T(0);
        if (active) {
            const int a0 = rp_lds[rr] - kb, a1 = rp_lds[rr + 1] - kb, last = a1 - 1;
            if (heavy > 0 && a1 - a0 > heavy) {
                active = false;
                if (lane == 0) hl[atomicAdd(hn, 1)] = rr;
            } else {
                // branch-free: every step issues its NA loads together
                // (clamped into the row) and a slot past the row keeps its
                // partial by a select (one v_cndmask), not by adding +0: under
                // FTZ a partial can be -0 (a negative denormal sum flushed),
                // and -0 + +0 is +0 where the canonical order has no add. A
                // predicated load per product made the compiler wait on each
                // one, so a 256-entry row in a tile of short rows held its
                // workgroup ~8 us (scripts/percall_probe.py).
                for (int base = a0 + lane; base < a1; base += 8) {
                    T v[NA];
#pragma unroll
                    for (int t = 0; t < NA; ++t) v[t] = lds[min(base + t * L, last)];
#pragma unroll
                    for (int t = 0; t < NA; ++t)  // partial (lane + t*L) of the row
                        acc[t] = base + t * L < a1 ? acc[t] + v[t] : acc[t];
                }
            }
        }
        // tree stages whose pair offset (4, 2, 1) is a multiple of L: local
#pragma unroll
        for (int h = NA / 2; h >= 1; h >>= 1)
#pragma unroll
            for (int t = 0; t < h; ++t) acc[t] = acc[t] + acc[t + h];
        T s = acc[0];
        // remaining stages across the L lanes of the group
#pragma unroll
        for (int off = L / 2; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
        if (active && lane == 0) sink(rr, s);
    }
}

// The rows listed by reduce_rows (hl[0 .. hn)): eight lanes per row, lane j
// summing partial j (products j, j+8, ... in order) four steps per round
// (32 products, loads issued together), then the canonical tree over the
// eight lanes — the same bits as any L. A tile's few 33–256-entry rows no
// longer run one lane's 8-partial loop each while the rest of the tile idles.
template <typename T, int NTH, typename Sink>
__device__ __forceinline__ void reduce_heavy_rows(const T *lds, const unsigned short *rp_lds, int kb,
                                                  const int *hl, int hn, Sink sink) {
    constexpr int NG = NTH / 8;
    const int tid = threadIdx.x;
    const int g = tid >> 3, lane = tid & 7;
    for (int h = g; h - g < hn; h += NG) {  // same trip count for all groups
        const bool active = h < hn;
        T acc = T(0);
        const int rr = active ? hl[h] : 0;
        if (active) {
            const int a1 = rp_lds[rr + 1] - kb, last = a1 - 1;
            for (int base = rp_lds[rr] - kb + lane; base < a1; base += 32) {
                T v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = lds[min(base + 8 * t, last)];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc = base + 8 * t < a1 ? acc + v[t] : acc;  // (select: see reduce_rows)
            }
        }
#pragma unroll
        for (int off = 4; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        if (active && lane == 0) sink(rr, acc);
    }
}

// lanes per row: power of two <= 8 such that each lane still sums >= 4
// products of an average row and the groups fit the workgroup; with L < 8,
// rows longer than 32 L entries go to reduce_heavy_rows after a barrier
// (hl: kSpmvHeavyMax ints of LDS, *hn zeroed before the tile's first barrier)
template <typename T, int NTH = kSpmvThreads, typename Sink>
__device__ __forceinline__ void reduce_tile_rows(const T *lds, const unsigned short *rp_lds, int nrows,
                                                 int nnzt, int kb, int *hl, int *hn, Sink sink) {
    int L = 1;
    while (L < 8 && 2 * L * nrows <= NTH && 8 * L * nrows <= nnzt) L <<= 1;
    switch (L) {
        case 1: reduce_rows<T, 1, NTH>(lds, rp_lds, nrows, kb, 32, hl, hn, sink); break;
        case 2: reduce_rows<T, 2, NTH>(lds, rp_lds, nrows, kb, 64, hl, hn, sink); break;
        case 4: reduce_rows<T, 4, NTH>(lds, rp_lds, nrows, kb, 128, hl, hn, sink); break;
        default: reduce_rows<T, 8, NTH>(lds, rp_lds, nrows, kb, 0, hl, hn, sink); return;
    }
    lds_barrier();
    const int n = *hn;  // workgroup-uniform
    if (n > 0) reduce_heavy_rows<T, NTH>(lds, rp_lds, kb, hl, n, sink);
}

// A long row (or one tile-sized chunk of it) in LDS slots [a, e): thread t
// sums slots a+t, a+t+256, ... in order, each wave combines its 64 sums with
// a xor-butterfly (32, 16, ..., 1), and the four wave sums are added as
// (w0+w1)+(w2+w3) — the canonical order for rows longer than kSpmvLongRow
// (oracle_spmv_canon_*). The total is valid in thread 0.
template <typename T>
__device__ __forceinline__ T reduce_long(const T *lds, int a, int e, T *wsum) {
    const int tid = threadIdx.x;
    T s = T(0);
    for (int k = a + tid; k < e; k += kSpmvThreads) s += lds[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    lds_barrier();
    return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

#ifdef RSP_SPMV_PROBE_LOADS
#include "spmv_probe.h"
#endif

// One tile: stream -> gathers -> products in LDS -> canonical reduce -> y.
// BETA: beta != 0 (y is read); the beta == 0 form issues no y loads, so its
// y stores never wait on anything.
// A chunk of a long row (wave 0 of its tile): publish the chunk's partial,
// take a ticket; the chunk that arrives last adds the row's partials in chunk
// order (the fixup kernel's order: 0 + p0 + p1 + ...) and writes y. No wait,
// no spin: the last arriver is told by the value its own add returned; it
// resets the ticket. The hand-off is the write-through form of
// MI355X_MICROARCH.md §Workgroup dispatch (valid forms; cdna_hip_programming.md
// split-K recipe, "equally valid and cheaper"): the partial is an agent-scope
// (sc1, write-through) store, drained by the storing lane's s_waitcnt vmcnt(0)
// before its relaxed agent-scope ticket add, and the last arriver reads EVERY
// partial with agent-scope (sc1) loads — so neither an L2 write-back
// (release) nor an L1 invalidate (acquire) is on the row's path (round 5;
// they were ~1.7 us each). The last arriver's lanes load the partials in
// parallel (lane c: partial c), one memory round trip instead of one per
// chunk, and the in-order sum runs on shuffles.
// The relaxed form above relies on gfx9-family ordering (LLVM AMDGPU memory
// model, GFX942/GFX950 rows: stores are counted by vmcnt, and agent-scope
// (sc1) stores write through and sc1 loads bypass the non-coherent caches).
// gfx10+ counts stores in a separate vscnt, so this file builds for gfx950
// only (the library's one target).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "longrow_arrive's relaxed hand-off is only valid on gfx942 / gfx950"
#endif
template <typename T>
__device__ __forceinline__ void longrow_arrive(const SpmvBlock blk, const int *__restrict__ rowptr,
                                               T *partials, T *__restrict__ y, T t, T alpha, T beta,
                                               bool beta_nz) {
    typedef typename std::conditional<sizeof(T) == 8, unsigned long long, unsigned int>::type U;
    constexpr int C = SpmvTile<T>::kChunk;
    const int lane = threadIdx.x & 63;
    const int slot = -(blk.r1 + 1);
    const int rs = rowptr[blk.r0], re = rowptr[blk.r0 + 1];
    const int first = slot - (blk.k0 - rs) / C;
    const int n = (re - rs + C - 1) / C;
    // global-address-space pointers: global_ (not flat_) instructions, the
    // form the hand-off is measured for (the batched kernel's entry pointers
    // are generic)
    typedef __attribute__((address_space(1))) U GU;
    typedef __attribute__((address_space(1))) unsigned int GI;
    GU *pv = (GU *)reinterpret_cast<U *>(partials);
    GI *ticket = (GI *)reinterpret_cast<unsigned int *>(partials + 2 * first + 1);
    unsigned int arrived = 0;
    if (lane == 0) {
        __hip_atomic_store(pv + 2 * slot, __builtin_bit_cast(U, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial has left this CU before the ticket moves
        arrived = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    arrived = (unsigned int)__builtin_amdgcn_readfirstlane((int)arrived);
    if (arrived != (unsigned int)(n - 1)) return;  // wave-uniform
    T s = T(0);
    for (int c0 = 0; c0 < n; c0 += 64) {
        const T p = c0 + lane < n ? __builtin_bit_cast(T, __hip_atomic_load(pv + 2 * (first + c0 + lane),
                                                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                  : T(0);
        const int cn = min(64, n - c0);
        for (int c = 0; c < cn; ++c) s += __shfl(p, c, 64);
    }
    if (lane == 0) {
        T out = alpha * s;
        if (beta_nz) out += beta * y[blk.r0];
        y[blk.r0] = out;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename T, bool NT, bool BETA>
__device__ __forceinline__ void spmv_tile(
    const SpmvBlock blk, const int *__restrict__ rowptr, const int *__restrict__ colidx,
    const unsigned short *__restrict__ cidx, const int *__restrict__ runs, int cbase, int poff, int cmax,
    const T *__restrict__ vals, const T *__restrict__ x, T *__restrict__ y,
    T *partials, T alpha, T beta, int beta_nonzero, int nnz, int vector_ok, T *lds,
    T *wsum, unsigned short *rp_lds, int *hl, int fuse) {
    constexpr int VW = 16 / sizeof(T);
    constexpr int RPQ = (SpmvTile<T>::kMaxRows + kSpmvThreads) / kSpmvThreads;
    // packed row offsets: two per word
    constexpr int RPW = (SpmvTile<T>::kMaxRows / 2 + kSpmvThreads) / kSpmvThreads;
    static_assert(RPW <= RPQ, "the packed row words fit the row offsets' registers");
    const int tid = threadIdx.x;
    const int k0 = blk.k0, k1 = blk.k1;
    // a staged tile's run descriptors: the first load of the tile, so the x
    // loads they lead to need not wait for the stream (vmcnt is in order)
    const bool staged = cbase <= -2;
    constexpr int SMAX = SpmvTile<T>::kStageSlots / kSpmvThreads;
    int2 rd = make_int2(0, 0);
    int nr = 0;
    int lsl[SMAX];  // list mode: this thread's slots' column offsets
    if (staged) {  // workgroup-uniform
        const int code = -2 - cbase;
        nr = code & 255;
        if (SpmvTile<T>::kStageList && nr == 255) {  // list mode: {base, U}, then U uint16 column offsets
            rd = reinterpret_cast<const int2 *>(runs)[code >> 8];
            const unsigned short *lst = reinterpret_cast<const unsigned short *>(runs + 2 * (code >> 8) + 2);
#pragma unroll
            for (int k = 0; k < SMAX; ++k)
                if (k * kSpmvThreads < rd.y) lsl[k] = lst[min(k * kSpmvThreads + tid, rd.y - 1)];
        } else if (tid <= nr) {
            rd = reinterpret_cast<const int2 *>(runs)[(code >> 8) + tid];
        }
    }
    // the tile's row offsets, loaded ahead of the stream and parked in LDS
    // after it, so the reduce never waits on global memory
    const int nrows = blk.r1 - blk.r0;
    const int nrows_ld = nrows > 0 ? nrows : 0;  // long-row chunks: r1 < 0
    // vectors may be used unless the tile reaches the last, partial vector
    const bool vec = vector_ok && k1 > k0 && k1 <= (nnz & ~(VW - 1));
    const int kb = vec ? (k0 & ~(VW - 1)) : k0;
    // a packed staged tile (workgroup-uniform): its record holds the slot
    // fields and (bit 0 of poff) the row offsets relative to the vector path's
    // kb, so only that path reads it; the scalar path keeps cidx / rowptr
    const unsigned int *rec =
        vec && staged && poff >= 0 ? reinterpret_cast<const unsigned int *>(runs) + (poff >> 1) : nullptr;
    const bool prow = rec && (poff & 1);
    const int nrw = (nrows_ld + 2) >> 1;  // packed row words
    // one branch-free sequence for both sources (the record's words, or
    // rowptr): only the base and the clamp differ, so nothing waits here
    const int *rsrc = prow ? reinterpret_cast<const int *>(rec) +
                                 kSpmvThreads * rsp_pack::words_per_thread(SpmvTile<T>::kSlots / kSpmvThreads)
                           : rowptr + blk.r0;
    const int rlim = prow ? nrw - 1 : nrows_ld;
    int rpv[RPQ];
#pragma unroll
    for (int q = 0; q < RPQ; ++q)  // unpredicated (clamped)
        rpv[q] = rsrc[min(tid + q * kSpmvThreads, rlim)];
#ifdef RSP_SPMV_PROBE_LOADS  // diagnostic builds only (make probe; scripts/spmv_probe.py loadsonly)
    if (vec) {
        probe_tile_loads<T, NT>(colidx, vals, y, blk, kb, k1, rpv[0]);
        return;
    }
#endif
    if (vec && cbase >= 0)
        stream_products<T, NT, true>(colidx, cidx, cbase, cmax, vals, x, kb, k1, lds);
    else if (vec && staged && sizeof(T) == 4)
        stream_products_staged<T, NT, 2>(cidx, rec, rd, nr, lsl, vals, x, kb, k1, lds);
    else if (vec && rec)
        stream_products_staged<T, NT, 1>(cidx, rec, rd, nr, lsl, vals, x, kb, k1, lds);
    else if (vec && staged)
        stream_products_staged<T, NT, 0>(cidx, rec, rd, nr, lsl, vals, x, kb, k1, lds);
    else if (vec)
        stream_products<T, NT>(colidx, cidx, 0, 0, vals, x, kb, k1, lds);
    else
        stream_products_scalar<T>(colidx, vals, x, k0, kb, k1, lds);
    if (prow) {  // already relative to kb, two per word
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const int i = tid + q * kSpmvThreads;
            if (i < nrw) reinterpret_cast<unsigned int *>(rp_lds)[i] = (unsigned int)rpv[q];
        }
    } else {
#pragma unroll
        for (int q = 0; q < RPQ; ++q) {
            const int i = tid + q * kSpmvThreads;
            if (i <= nrows) rp_lds[i] = (unsigned short)(rpv[q] - kb);  // < kSlots + kVec
        }
    }
    if (tid == 0) hl[0] = 0;  // the tile's heavy-row count (reduce_tile_rows)
    lds_barrier();

    if (blk.r1 < 0) {  // a long row: written whole, or a chunk partial for the fixup
        const T t = reduce_long(lds, k0 - kb, k1 - kb, wsum);
        if (blk.r1 != rsp::kSpmvWholeRow && fuse) {
            if (tid < 64) longrow_arrive<T>(blk, rowptr, partials, y, t, alpha, beta, BETA);
        } else if (tid == 0) {
            if (blk.r1 == rsp::kSpmvWholeRow) {
                T out = alpha * t;
                if (BETA) out += beta * y[blk.r0];
                y[blk.r0] = out;
            } else {
                partials[2 * -(blk.r1 + 1)] = t;
            }
        }
        return;
    }

    const int r0 = blk.r0;
    reduce_tile_rows<T>(lds, rp_lds, nrows, k1 - k0, 0, hl + 1, hl, [&](int rr, T sum) {
        T out = alpha * sum;
        if (BETA) out += beta * y[r0 + rr];
        // fp64: non-temporal y stores (the y lines leave L2 as a stream;
        // -3 % per pass on the big set, where plain y write-back costs ~16 %
        // of the time for ~4 % of the bytes); fp32: plain stores (nt +2 %)
        constexpr bool kNtY = RSP_NT_Y > 0 || (RSP_NT_Y < 0 && sizeof(T) == 8);
        if constexpr (kNtY)
            __builtin_nontemporal_store(out, y + r0 + rr);
        else
            y[r0 + rr] = out;
    });
}

// One workgroup per tile (XCD-swizzled). Measured alternatives, all slower
// on the big set: 2/4/8 tiles walked per workgroup (-5/-10/
// -18 %), all of a workgroup's tiles loaded up front (-4 %), a software-
// pipelined persistent kernel (-29 %), one-wave tiles (-1 %).
template <typename T, bool NT, bool BETA>
__global__ __launch_bounds__(kSpmvThreads) void spmv_tiles(
    const int *__restrict__ rowptr, const int *__restrict__ colidx, const T *__restrict__ vals,
    const T *__restrict__ x, T *__restrict__ y, const SpmvBlock *__restrict__ blocks, int nblocks,
    const int *__restrict__ cbases, const int *__restrict__ poffs, const unsigned short *__restrict__ cidx,
    const int *__restrict__ runs, int cmax, T *partials, T alpha, T beta, int beta_nonzero, int nnz,
    int vector_ok, int fuse) {
    __shared__ __attribute__((aligned(16))) T lds[SpmvTile<T>::kSlots];
    __shared__ T wsum[kSpmvThreads / 64];
    __shared__ int hl[1 + kSpmvHeavyMax];  // heavy rows of the tile: count, list
    __shared__ __attribute__((aligned(4))) unsigned short rp_lds[SpmvTile<T>::kMaxRows + 2];  // row offsets - kb
    const int b = xcd_swizzle(blockIdx.x, nblocks);
    spmv_tile<T, NT, BETA>(blocks[b], rowptr, colidx, cidx, runs, cbases[b], poffs[b], cmax, vals, x, y,
                           partials, alpha, beta, beta_nonzero, nnz, vector_ok, lds, wsum, rp_lds, hl,
                           fuse);
}

// One long row per wave: y[row] = alpha * (0 + p0 + p1 + ...) (+ beta*y[row]),
// the chunk partials added in chunk order. Lane c loads partial c, so a row
// costs one memory round trip instead of one per chunk (the loads of a
// serial loop each waited for the add before them); the in-order sum runs
// on shuffles, every lane computing it.
template <typename T>
__device__ __forceinline__ void fixup_row(const SpmvLongRow r, const T *__restrict__ partials,
                                          T *__restrict__ y, T alpha, T beta, int beta_nonzero) {
    const int lane = threadIdx.x;
    const T yv = (beta_nonzero && lane == 0) ? y[r.row] : T(0);
    T s = T(0);
    for (int c0 = 0; c0 < r.nchunks; c0 += 64) {
        const T p = c0 + lane < r.nchunks ? partials[2 * (r.first + c0 + lane)] : T(0);
        const int cn = min(64, r.nchunks - c0);
        for (int c = 0; c < cn; ++c) s += __shfl(p, c, 64);
    }
    if (lane == 0) {
        T out = alpha * s;
        if (beta_nonzero) out += beta * yv;
        y[r.row] = out;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void spmv_longrow_fixup(const SpmvLongRow *__restrict__ lr,
                                                          int nlong, const T *__restrict__ partials,
                                                          T *__restrict__ y, T alpha, T beta,
                                                          int beta_nonzero) {
    fixup_row<T>(lr[blockIdx.x], partials, y, alpha, beta, beta_nonzero);
}

// Batched form: several independent matrices' tiles in one grid (one
// workgroup per tile, as spmv_tiles). Matrix j owns workgroups
// [begin[j], begin[j+1]); within it the tiles are XCD-swizzled as in
// spmv_tiles, so every matrix spreads over all XCDs (a swizzle over the
// whole grid would give each XCD a different matrix and unbalance them).
// One launch instead of one per matrix removes the per-kernel ramp and drain
// (~5 us each on the big set, more than the whole SpMV of a small slice).
template <typename T, bool NT, bool BETA, bool SWZ>
__global__ __launch_bounds__(kSpmvThreads) void spmv_tiles_batch(
    const SpmvBatchEntry *__restrict__ entries, const SpmvBlock *__restrict__ tiles,
    const int *__restrict__ cbases, const int *__restrict__ poffs, SpmvBatchTable at, T alpha, T beta,
    int fuse) {
    __shared__ __attribute__((aligned(16))) T lds[SpmvTile<T>::kSlots];
    __shared__ T wsum[kSpmvThreads / 64];
    __shared__ int hl[1 + kSpmvHeavyMax];  // heavy rows of the tile: count, list
    __shared__ __attribute__((aligned(4))) unsigned short rp_lds[SpmvTile<T>::kMaxRows + 2];  // row offsets - kb
    const int b = blockIdx.x;
    // lo / hi selected inside the compare chain on the kernel arguments
    // (preloaded into SGPRs, so no memory latency in front of the tile
    // record load). 84 SGPRs with the swizzle = 7 rather than 8 workgroups
    // per CU by the residency rule, which measured equal to 8 on the
    // one-matrix kernel; both lookups that needed fewer SGPRs (begin[j] read
    // by index after counting j: 76; a ballot over begin[lane]: 42) put a
    // load in front of the tile and measured 1-2 % slower.
    int j = 0, lo = 0, hi = at.begin[1];
#pragma unroll
    for (int q = 1; q < kSpmvBatchMax; ++q)  // scalar compares, no loads
        if (b >= at.begin[q]) {
            j = q;
            lo = at.begin[q];
            hi = at.begin[q + 1];
        }
    const int t = lo + (SWZ ? xcd_swizzle(b - lo, hi - lo) : b - lo);
    const SpmvBatchEntry e = entries[j];
    spmv_tile<T, NT, BETA>(tiles[t], e.rowptr, e.colidx, e.cidx, e.runs, cbases[t], poffs[t], e.cmax,
                           (const T *)e.vals, (const T *)e.x,
                           (T *)e.y, (T *)e.partials, alpha, beta, BETA, e.nnz, e.vector_ok, lds,
                           wsum, rp_lds, hl, fuse);
}

template <typename T>
__global__ __launch_bounds__(64) void spmv_longrow_fixup_batch(
    const SpmvBatchEntry *__restrict__ entries, const SpmvLongRow *__restrict__ lr,
    SpmvBatchTable at, T alpha, T beta, int beta_nonzero) {
    const int i = blockIdx.x;  // one wave per long row
    int j = 0;
#pragma unroll
    for (int q = 1; q < kSpmvBatchMax; ++q)
        if (i >= at.begin[q]) j = q;
    const SpmvBatchEntry e = entries[j];
    fixup_row<T>(lr[i], (const T *)e.partials, (T *)e.y, alpha, beta, beta_nonzero);
}

template <typename T>
static hipError_t launch_spmv_batch(const SpmvBatchArgs &a, hipStream_t s) {
    const T alpha = (T)a.alpha, beta = (T)a.beta;
    const int bnz = a.beta != 0.0;
    const int ntiles = a.tiles_at.begin[a.count];
    const int fuse = !(a.variant & rsp::kSpmvVariantFixup);
    if (ntiles > 0) {
        const bool nt = !(a.variant & 1), swz = !(a.variant & 8);
        auto kern = bnz ? (nt ? (swz ? spmv_tiles_batch<T, true, true, true>
                                     : spmv_tiles_batch<T, true, true, false>)
                              : (swz ? spmv_tiles_batch<T, false, true, true>
                                     : spmv_tiles_batch<T, false, true, false>))
                        : (nt ? (swz ? spmv_tiles_batch<T, true, false, true>
                                     : spmv_tiles_batch<T, true, false, false>)
                              : (swz ? spmv_tiles_batch<T, false, false, true>
                                     : spmv_tiles_batch<T, false, false, false>));
        hipLaunchKernelGGL(kern, dim3(ntiles), dim3(kSpmvThreads), 0, s, a.entries, a.tiles,
                           a.cbases, a.poffs, a.tiles_at, alpha, beta, fuse);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int nlong = a.longs_at.begin[a.count];
    if (nlong > 0 && !fuse) {
        // the fixup reads begin[kSpmvBatchMax] as its bound: the table past
        // `count` holds INT_MAX, so pass the total explicitly
        SpmvBatchTable lt = a.longs_at;
        lt.begin[kSpmvBatchMax] = nlong;
        hipLaunchKernelGGL((spmv_longrow_fixup_batch<T>), dim3(nlong), dim3(64), 0, s,
                           a.entries, a.longrows, lt, alpha, beta, bnz);
        return hipGetLastError();
    }
    return hipSuccess;
}

hipError_t spmv_batch_f32(const SpmvBatchArgs &a, hipStream_t s) {
    return launch_spmv_batch<float>(a, s);
}

template <typename T>
static hipError_t launch_spmv(const SpmvArgs &a, hipStream_t s) {
    if (a.nblocks <= 0) return hipSuccess;
    const T alpha = (T)a.alpha, beta = (T)a.beta;
    const int bnz = a.beta != 0.0;
    const int fuse = !(a.variant & rsp::kSpmvVariantFixup);
    // vals/colidx are read once per call: non-temporal loads keep them from
    // evicting x (measured +2% fp64 / +7.5% fp32 on the cache-cold big set);
    // variant bit 0 restores default-policy loads for A/B runs
    auto kern = (a.variant & 1) ? (bnz ? spmv_tiles<T, false, true> : spmv_tiles<T, false, false>)
                                : (bnz ? spmv_tiles<T, true, true> : spmv_tiles<T, true, false>);
    hipLaunchKernelGGL(kern, dim3(a.nblocks), dim3(kSpmvThreads), 0, s, a.rowptr, a.colidx,
                       (const T *)a.vals, (const T *)a.x, (T *)a.y, a.blocks, a.nblocks, a.cbases,
                       a.poffs, a.cidx, a.runs, a.cmax, (T *)a.partials, alpha, beta, bnz, a.nnz, a.vector_ok, fuse);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.nlong > 0 && !fuse) {
        hipLaunchKernelGGL((spmv_longrow_fixup<T>), dim3(a.nlong), dim3(64), 0, s,
                           a.longrows, a.nlong, (const T *)a.partials, (T *)a.y, alpha, beta, bnz);
        e = hipGetLastError();
    }
    return e;
}

hipError_t spmv_f32(const SpmvArgs &a, hipStream_t s) { return launch_spmv<float>(a, s); }
void warm_spmv() {
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(spmv_tiles<float, true, false>));
    int o = 0;  // (the occupancy query is the use measured to load the code object)
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, spmv_tiles<float, true, false>, kSpmvThreads, 0);
}

#ifndef RSP_FTZ_BUILD
int spmv_tiles_per_cu(int elem_bytes) {
    int o = 0;
    const hipError_t e =
        elem_bytes == 8
            ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, spmv_tiles<double, true, false>, kSpmvThreads, 0)
            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, spmv_tiles<float, true, false>, kSpmvThreads, 0);
    return (e == hipSuccess && o > 0) ? o : 1;
}

// dst[i] = src[idx[i]]: halo pack/unpack of the multi-GPU SpMV. Grid-stride,
// 4 elements in flight per thread; ~12-20 B per element, HBM/L2 bound.
template <typename E>
__global__ __launch_bounds__(256) void gather_kernel(const int64_t *__restrict__ idx,
                                                     const E *__restrict__ src, E *__restrict__ dst,
                                                     int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = src[idx[i]];
}

template <typename E>
__global__ __launch_bounds__(256) void scatter_kernel(const int64_t *__restrict__ idx,
                                                      const E *__restrict__ src, E *__restrict__ dst,
                                                      int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[idx[i]] = src[i];
}

hipError_t scatter(int elem_bytes, int64_t n, const int64_t *idx, const void *src, void *dst,
                   hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t want = (n + 255) / 256;
    const int grid = (int)(want < 2048 ? want : 2048);
    if (elem_bytes == 8)
        hipLaunchKernelGGL((scatter_kernel<double>), dim3(grid), dim3(256), 0, s, idx,
                           (const double *)src, (double *)dst, n);
    else
        hipLaunchKernelGGL((scatter_kernel<float>), dim3(grid), dim3(256), 0, s, idx,
                           (const float *)src, (float *)dst, n);
    return hipGetLastError();
}

hipError_t gather(int elem_bytes, int64_t n, const int64_t *idx, const void *src, void *dst,
                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t want = (n + 255) / 256;
    const int grid = (int)(want < 2048 ? want : 2048);
    if (elem_bytes == 8)
        hipLaunchKernelGGL((gather_kernel<double>), dim3(grid), dim3(256), 0, s, idx,
                           (const double *)src, (double *)dst, n);
    else
        hipLaunchKernelGGL((gather_kernel<float>), dim3(grid), dim3(256), 0, s, idx,
                           (const float *)src, (float *)dst, n);
    return hipGetLastError();
}

hipError_t spmv_f64(const SpmvArgs &a, hipStream_t s) { return launch_spmv<double>(a, s); }
hipError_t spmv_batch_f64(const SpmvBatchArgs &a, hipStream_t s) {
    return launch_spmv_batch<double>(a, s);
}
#endif

}  // namespace RSP_KNS
