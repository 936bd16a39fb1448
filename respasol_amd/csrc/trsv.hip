// trsv.hip — level-scheduled triangular solves with the ILU(0) factors for
// gfx950, replacing cusparse?csrsv2_solve (GPU/ilu0.cu:287-302). They follow
// the segments of the analysis' level plans as the factor does (ilu0.hip:
// fat levels a launch each or one flow launch per run, thin runs one
// 1024-thread workgroup); the primitives are ilu_device.h and ilu_flow.h.
//
// Kind 0 = L op N, 1 = L^T op T, 2 = U, over the DAG's flat terms:
// y_i = (alpha x_i - sum_k vals[tpos[k]] * y[src[k]]) (/ u_ii), one fma per
// term in the term order (identical in the CPU oracle: bitwise equal):
//   L   y = alpha x : y_i = fma(-l_ij, y_j, ...) over j ascending, from alpha*x_i
//   L^T y = alpha x : y_i = fma(-l_ji, y_j, ...) over j DESCENDING, from alpha*x_i
//   U   y = alpha x : y_i = (alpha*x_i - sum_j>i u_ij y_j) / u_ii, j ascending
//
// Compiled twice like spmv.hip (rsp_k / rsp_k_ftz).

#include <hip/hip_runtime.h>

#include <type_traits>
#include <limits.h>

#include "ilu_device.h"
#include "ilu_flow.h"

namespace RSP_KNS {

using rsp::kThinThreads;
using rsp::LevelPlan;
using rsp::TrsvArgs;

// s - sum v_k y[src_k] over k = k0 .. k1-1 in order, from the solve streams
// (term values in flat order, no position indirection). The values and y
// indices of batch j+1 are loaded while batch j's y gather is in flight (the
// loads are clamped, unpredicated), so a batch costs one memory round trip.
template <typename T, int B>
__device__ __forceinline__ T stream_chain(T s, int k0, int k1, const T *sval, const int *src, const T *y) {
    const int n = k1 - k0;
    if (n <= 0) return s;
    T v[B];
    int id[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int k = k0 + min(b, n - 1);
        v[b] = sval[k];
        id[b] = src[k];
    }
    for (int b0 = 0; b0 < n; b0 += B) {
        T yv[B], vc[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            yv[b] = y[id[b]];
            vc[b] = v[b];
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int k = k0 + min(b0 + B + b, n - 1);
            v[b] = sval[k];
            id[b] = src[k];
        }
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (b0 + b < n) s = fma_t(-vc[b], yv[b], s);
    }
    return s;
}

// The serial chain of one hub row (thousands of terms) by a 256-thread
// workgroup: waves 1-3 gather the terms group by group (768 a group: value
// and y index, then the y) into an LDS double buffer while wave 0 runs the
// chain over the previous group on broadcast LDS operands, one fma per term
// in order. A wave alone paid two dependent global round trips per 64 terms.
// The result is valid in wave 0.
template <typename T>
__device__ __forceinline__ T block_chain(T s, int k0, int k1, const T *sval, const int *src, const T *y) {
    constexpr int NL = 192, PER = 4, GS = NL * PER;
    __shared__ T bv[2][GS], by[2][GS];
    const int tid = threadIdx.x, n = k1 - k0, ng = (n + GS - 1) / GS;
    auto gather = [&](int g) {  // loader waves: group g into buffer g & 1
        T v[PER], yv[PER];
        int id[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = min(g * GS + (tid - 64) + j * NL, n - 1);
            v[j] = sval[k0 + k];
            id[j] = src[k0 + k];
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) yv[j] = y[id[j]];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            bv[g & 1][(tid - 64) + j * NL] = v[j];
            by[g & 1][(tid - 64) + j * NL] = yv[j];
        }
    };
    if (tid >= 64) gather(0);
    __syncthreads();
    for (int g = 0; g < ng; ++g) {
        if (tid >= 64) {
            if (g + 1 < ng) gather(g + 1);
        } else {
            const T *pv = bv[g & 1], *py = by[g & 1];
            const int cnt = min(GS, n - g * GS);
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) s = fma_t(-pv[j], py[j], s);
        }
        __syncthreads();
    }
    return s;
}

// Fat level, terms from the solve streams (trsv_stream): blocks [0, nb) one
// thread per short row (the level's first nshort rows), the next nwb blocks
// one wave per long row (rows up to nwave), the blocks after them one hub row
// each. Slot off + r of the level order: task, alpha x_i (and u_ii) at the
// same index, so the row's first loads are independent.
template <typename T, int KIND, int B>
__global__ __launch_bounds__(256) void trsv_level(TrsvArgs a, int off, int nrows, int nshort, int nb,
                                                  int nwave, int nwb, int sbase) {
    const T *sval = (const T *)a.sval;
    T *y = (T *)a.y;
    const int *src = a.plan.src;
    int x;
    T s;
    rsp::RowTask t;
    if ((int)blockIdx.x >= nb + nwb) {  // hub row: the whole workgroup (uniform branch)
        x = off + nwave + (blockIdx.x - nb - nwb);
        t = a.plan.tasks[x];
        s = block_chain<T>(((const T *)a.sx)[x], t.t0, t.t1, sval, src, y);
        if (threadIdx.x != 0) return;
    } else if ((int)blockIdx.x < nb) {
        const int r = blockIdx.x * 256 + threadIdx.x;
        if (r >= nshort) return;
        x = off + r;
        t = a.plan.tasks[x];
        if (sbase >= 0) {
            // padded short rows: the row's kFatLongTerms flat terms start at
            // sbase + 8 r, so the values and y indices load with the task
            // instead of after it; pads (beyond t1) are never used
            constexpr int F = rsp::kFatLongTerms;
            const int t0 = sbase + r * F;
            T v[F], yv[F];
            int id[F];
#pragma unroll
            for (int b = 0; b < F; ++b) {
                v[b] = sval[t0 + b];
                id[b] = src[t0 + b];
            }
            s = ((const T *)a.sx)[x];
            const int n = t.t1 - t0;
#pragma unroll
            for (int b = 0; b < F; ++b) yv[b] = y[b < n ? id[b] : 0];
#pragma unroll
            for (int b = 0; b < F; ++b)
                if (b < n) s = fma_t(-v[b], yv[b], s);
        } else {
            s = stream_chain<T, B>(((const T *)a.sx)[x], t.t0, t.t1, sval, src, y);
        }
    } else {
        const int r = nshort + (blockIdx.x - nb) * 4 + (threadIdx.x >> 6);
        if (r >= nwave) return;
        x = off + r;
        t = a.plan.tasks[x];
        if (a.wave_lds) {
            __shared__ T cwv[4][64], cwy[4][64];
            const int w = threadIdx.x >> 6;
            s = wave_chain_lds<T>(((const T *)a.sx)[x], t.t0, t.t1, threadIdx.x & 63, cwv[w], cwy[w], sval,
                                  src, y);
        } else {
            s = wave_chain<T>(((const T *)a.sx)[x], t.t0, t.t1, threadIdx.x & 63,
                              [&](int k) { return sval[k]; }, [&](int k) { return y[src[k]]; });
        }
        if ((threadIdx.x & 63) != 0) return;
    }
    if constexpr (KIND == 2) s = qdiv<T>(s, ((const T *)a.sdg)[x]);
    y[t.i] = s;
}

// Flow segments (a solve DAG's runs of two or more fat levels): ONE launch of
// a.flow_grid workgroups instead of a launch per level. The waves walk the
// segment's work items (rsp::FlowItem, level order) statically or by claims
// (FlowClaims, rsp::FlowCtl); an item starts as soon as the y values it reads
// exist, not when its whole previous level has ended. Existence is read from
// the value itself: trsv_stream sets every y to kNotYet, a signalling-NaN
// bit pattern that no y can have (every y is an arithmetic result — alpha x_i,
// an fma, a division — and arithmetic only produces quiet NaNs); a row's y is
// written once, by one 4- / 8-byte device-scope (sc1) store, and a consumer
// reads its operands with device-scope (sc1) loads, re-reading (after an
// s_sleep) those still kNotYet: the data-tagged hand-off of the price list
// in MI355X_MICROARCH.md (handoff-1to1) — no flag, no fence.
// Progress: an item waits only for items of lower index, and each wave runs
// its items in index order; with static items the grid is resident at once
// (the lowest unfinished item is some wave's current item), with claims any
// item waited on is held by a running wave. A wait beyond fc.ticks (never
// expected) gives up and records the call in *fc.status (rsp_trsv_zero_pivot
// then returns EXECUTION_FAILED) instead of hanging the GPU.
// Same terms, same order, same fma chain as trsv_level: the same bits.
template <typename T, int KIND, bool TK>
__global__ __launch_bounds__(256) void trsv_flow(TrsvArgs a, int it0, int it1, unsigned long long base) {
    typedef typename FlowWord<T>::U U;
    constexpr int F = rsp::kFatLongTerms;
    __shared__ T fwv[4][64], fwy[4][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const T *sval = (const T *)a.sval, *sx = (const T *)a.sx;
    T *y = (T *)a.y;
    const int *src = a.plan.src;
    __shared__ std::conditional_t<TK, FlowTicketLds, int> tl_;  // (tickets only)
    FlowClaims<TK> fq(a.fc, base, it0, it1, blockIdx.x * 4 + wv, (int)gridDim.x * 4, reinterpret_cast<FlowTicketLds *>(&tl_));
    // claims are issued behind each item's first loads (task, term values and sources)
    for (fq.first(); fq.more(); fq.next()) {
        const int it = fq.item();
        if (it >= it1) continue;  // (tickets: a last round's spare waves)
        const rsp::FlowItem f = a.plan.fitems[it];
        if (f.n > 0) {  // short rows, a lane each (lanes past them repeat the last row)
            const int r = min(lane, f.n - 1), x = f.x0 + r;
            const rsp::RowTask t = a.plan.tasks[x];
            T v[F];
            int id[F], n;
            if (f.t0 >= 0) {  // padded: the terms load with the task
                const int t0 = f.t0 + r * F;
#pragma unroll
                for (int b = 0; b < F; ++b) {
                    v[b] = sval[t0 + b];
                    id[b] = src[t0 + b];
                }
                n = t.t1 - t0;
            } else {
                n = t.t1 - t.t0;
                const int kl = max(t.t1 - 1, 0);
#pragma unroll
                for (int b = 0; b < F; ++b) {
                    const int k = min(t.t0 + b, kl);
                    v[b] = sval[k];
                    id[b] = src[k];
                }
            }
            T s = sx[x];
            fq.claim_ahead();
            // yl: a wait yielded (as in ilu0_flow: the item runs through and stores nothing)
            bool yl = flow_gate<T>(f.gate, y, fq, a.flow_sleep);
            U w[F];
#pragma unroll
            for (int b = 0; b < F; ++b) w[b] = b < n ? flow_load(y + id[b]) : U(0);
            if (flow_wait<T, F>(w, id, n, y, fq, a.flow_sleep, yl)) yl = true;
#pragma unroll
            for (int b = 0; b < F; ++b)
                if (b < n) s = fma_t(-v[b], __builtin_bit_cast(T, w[b]), s);
            if constexpr (KIND == 2) s = qdiv<T>(s, ((const T *)a.sdg)[x]);
            if (lane < f.n && !yl) flow_store(y + t.i, s);
            fq.item_end(it, yl);
        } else {  // one row of more terms: a wave, 64 terms at a time on LDS broadcast operands
            const int x = f.x0;
            const rsp::RowTask t = a.plan.tasks[x];
            T s = sx[x];
            fq.claim_ahead();
            bool yl = flow_gate<T>(f.gate, y, fq, a.flow_sleep);
            for (int base = t.t0; base < t.t1; base += 64) {
                const int k = min(base + lane, t.t1 - 1);
                const T v = sval[k];
                int id[1] = {src[k]};
                U w[1] = {flow_load(y + id[0])};
                if (flow_wait<T, 1>(w, id, 1, y, fq, a.flow_sleep, yl)) yl = true;
                fwv[wv][lane] = v;
                fwy[wv][lane] = __builtin_bit_cast(T, w[0]);
                wave_sync();
                const int cnt = min(64, t.t1 - base);
                int j = 0;
                for (; j + 4 <= cnt; j += 4) {  // (wave_chain_lds's chain; folding the two changed this kernel's code)
                    T p[4], q[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        p[u] = fwv[wv][j + u];
                        q[u] = fwy[wv][j + u];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) s = fma_t(-p[u], q[u], s);
                }
                for (; j < cnt; ++j) s = fma_t(-fwv[wv][j], fwy[wv][j], s);
                wave_sync();  // this group's reads before the next group's stores
            }
            if constexpr (KIND == 2) s = qdiv<T>(s, ((const T *)a.sdg)[x]);
            if (lane == 0 && !yl) flow_store(y + t.i, s);
            fq.item_end(it, yl);
        }
    }
}

// Thin run (levels cut into LDS-staged chunks [c0, c1)), one 1024-thread
// workgroup. A chunk holds <= kChunkRows rows and <= kChunkTerms term slots;
// every row of a thin run has its terms padded to whole groups of G = 4 (or 2,
// for DAGs of short chains)
// (pads: a zero value times the zero slot of the y buffer, an exact no-op), so
// a row is read as groups of four terms with vector LDS loads and no length
// tests. LDS per chunk:
//   lrow[r]  = {alpha x_i, first group | groups << 16, y slot}  (one 16-B load)
//   lval[k], lidx[k] = term value, byte offset of its y in ybuf (row order)
//   ybuf     = [ y window (kYWin slots, run index mod kYWin) | 0 | y staged
//               for slot k at kYWin + 1 + k (producers before the run or
//               already out of the window) ]
// The chunk's data reaches LDS through registers, two chunks deep: while chunk
// c's levels run, the plan loads of chunk c+2 (task, term positions and
// sources, level offsets: one row and four slots per thread) and the gathers
// of chunk c+1 (x_i, term values, staged y) are in flight, unpredicated with
// clamped indices, so nothing waits on them before the switch; y is written to
// global memory only at chunk switches (one store per thread), so no store is
// pending under the levels. A staged y has its producer > kYWin rows back —
// at least two switches earlier — so it is in memory when prefetched.
//
// Levels: a narrow level (<= 64 rows, all short) is computed by wave 0 alone,
// and consecutive narrow levels are ordered by the wave's in-order LDS
// accesses instead of workgroup barriers; the wave runs them software-
// pipelined — while level q's y loads, fma chain and y store are on the
// critical path, the first term group of level q+1 and the row records of
// level q+2 are already loading — so a level costs about one LDS round trip.
// The other waves skip to the barrier after the run. (Deep-level circuits are
// ~10^4 levels of ~10 rows: nearly every level is narrow.) Wider levels use
// all waves, one row per thread, long rows (> kLongTerms terms) a wave each,
// and an LDS-only barrier after each level.
template <typename T>
struct alignas(16) ThinRow {  // LDS row record of a thin chunk
    T x;                      // alpha * x_i
    int g;                    // first group (chunk-relative) | groups << 16
    int out;                  // byte offset of the row's y window slot in ybuf
};
template <typename T, int G>
struct alignas(sizeof(T) * G) TermGroup {  // values of one group of terms
    T v[G];
};
template <int G>
struct alignas(4 * G) TermIds {  // byte offsets of their y in ybuf
    int v[G];
};

// Solve streams, one pass over the DAG before its thin runs: per flat term
// its value (0 for a pad), per level-order slot alpha x_i (and u_ii for the U
// solve) — so a thin run stages contiguous streams instead of gathering.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void trsv_stream(TrsvArgs a, T alpha) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const T *vals = (const T *)a.vals;
    if (k < a.plan.nterms) {
        const int tp = a.plan.tpos[k];
        ((T *)a.sval)[k] = tp >= 0 ? vals[tp] : T(0);
    }
    if (k < a.n) {
        const rsp::RowTask t = a.plan.tasks[k];
        ((T *)a.sx)[k] = alpha * ((const T *)a.x)[t.i];
        if constexpr (KIND == 2) ((T *)a.sdg)[k] = t.d >= 0 ? vals[t.d] : T(0);
        // flow segments read "not produced yet" from y itself (trsv_flow);
        // every other row's y is written by its own segment before any reader
        if (a.flow && a.plan.has_flow) ((typename FlowWord<T>::U *)a.y)[t.i] = FlowWord<T>::kNotYet;
    }
}

// The LDS layout of trsv_thin_pf (byte offsets into its one LDS object).
template <typename T, int KIND, int G>
struct ThinLay {
    static constexpr int al(int v, int a) { return (v + a - 1) / a * a; }
    static constexpr int idx = 0;
    static constexpr int val = al(idx + (rsp::kChunkTerms / G + 1) * (int)sizeof(TermIds<G>), 32);
    static constexpr int yb = al(val + (rsp::kChunkTerms / G + 1) * (int)sizeof(TermGroup<T, G>), 16);
    static constexpr int row = al(yb + (rsp::kYWin + 1 + rsp::kChunkTerms) * (int)sizeof(T), 16);
    static constexpr int rowi = row + rsp::kChunkRows * (int)sizeof(ThinRow<T>);
    static constexpr int ptr = rowi + 4 * rsp::kChunkRows;
    static constexpr int ns = ptr + 4 * (rsp::kChunkRows + 1);
    static constexpr int dg = al(ns + 4 * rsp::kChunkRows, 8);
    static constexpr int done = dg + (int)sizeof(T) * (KIND == 2 ? rsp::kChunkRows : 1);
    static constexpr int egr = done + 4;
    static constexpr int bytes = al(egr + rsp::kChunkRows, 16);
};

// PAIRS: narrow runs (levels of <= 64 short rows) on a.narrow_waves waves
// with two consecutive levels per wave turn (narrow_run_mw2), else one level
// per turn (narrow_run_mw; one wave: narrow_run). Its own instantiation (the
// registers).
// LW (round 5): the first LW waves never load the next chunk; the loader
// threads are the other kThinThreads - 64 LW (a thread stages rows lt + r NL
// and terms lt + j NL). The narrow waves then hold none of the chunk
// prefetch's registers, which gives narrow_run_mw2 the room to prepare every
// term group of up to three per level before its wait (G = 2): config-3 deep
// set, same box, interleaved x2 (profiles/r05_ilu_loaders_ab.txt): dc1 solve
// 4.77 -> 4.46 ms, G2_circuit 2.58 -> 2.33, matrix-new_3 5.60 -> 5.24; the
// split alone (without the extra groups) measured equal, and on DAGs that do
// not take the pair loop it cost (thermomech_TK 1.01 -> 1.05): LW = 4 with
// PAIRS only.
template <typename T, int KIND, int G, bool PAIRS = false, int LW = 0>
__global__ __launch_bounds__(rsp::kThinThreads) void trsv_thin_pf(TrsvArgs a, int c0, int c1, int base) {
    constexpr int NTH = rsp::kThinThreads;
    constexpr int NL = NTH - 64 * LW;                     // loader threads: lt = tid - 64 LW >= 0
    constexpr int TPT = (rsp::kChunkTerms + NL - 1) / NL;  // terms of a chunk per loader: lt + j NL
    constexpr int RPT = (rsp::kChunkRows + NL - 1) / NL;   // rows (and level pointers) per loader: lt + r NL
    static_assert(NL > 0 && G <= rsp::kGroup, "chunk loaders");
    static_assert(NTH >= rsp::kChunkRows, "a thin level's short rows: one per thread");
    constexpr int kZero = rsp::kYWin, kStaged = rsp::kYWin + 1;
    // + one pad group (values 0, y from the zero slot) after the chunk's groups
    constexpr int kPadGroup = rsp::kChunkTerms / G;
    // The workgroup's LDS is ONE object with a fixed layout, so the arrays the
    // narrow loops index per term sit where an LDS instruction's 16-bit offset
    // field can add their base: the term groups' y indices (lidx) at 0, their
    // values (lval) next, the y buffer (ybuf: window | zero slot | staged y)
    // after them; then the row records and the per-level arrays.
    using Lay = ThinLay<T, KIND, G>;
    static_assert(Lay::yb < 65536 && Lay::val < 65536 && Lay::bytes <= 163840, "LDS layout");
    __shared__ __attribute__((aligned(32))) char lds_arena[Lay::bytes];
    T *const ybuf = (T *)(lds_arena + Lay::yb);
    TermGroup<T, G> *const lval = (TermGroup<T, G> *)(lds_arena + Lay::val);
    TermIds<G> *const lidx = (TermIds<G> *)(lds_arena + Lay::idx);
    ThinRow<T> *const lrow = (ThinRow<T> *)(lds_arena + Lay::row);
    int *const lrowi = (int *)(lds_arena + Lay::rowi);
    unsigned char *const legr = (unsigned char *)(lds_arena + Lay::egr);  // per row: its early term groups (split order)
    T *const ldg = (T *)(lds_arena + Lay::dg);  // u_ii: U solve only
    int *const lptr = (int *)(lds_arena + Lay::ptr);
    int *const lns = (int *)(lds_arena + Lay::ns);
    int &lds_done = *(int *)(lds_arena + Lay::done);  // multi-wave narrow runs: absolute levels completed
    const int tid = threadIdx.x;
    const int lt = tid - 64 * LW;  // loader index (< 0: a narrow-run wave that never loads)
    if (tid == 0) lds_done = INT_MIN;  // ordered before any use by the first chunk's barriers
    const T *sval = (const T *)a.sval, *sx = (const T *)a.sx, *sdg = (const T *)a.sdg;
    T *y = (T *)a.y;
    const int *ptr = a.plan.ptr_dev;
    if (tid == 0) ybuf[kZero] = T(0);
    if (tid < G) {  // the pad group: exact no-op terms, fma(-0, 0, s) == s
        lval[kPadGroup].v[tid] = T(0);
        lidx[kPadGroup].v[tid] = kZero * (int)sizeof(T);
    }
    struct Pre {  // this loader's share of a chunk: rows lt + r NL, terms lt + j NL (all streams)
        rsp::ThinRowPlan r[RPT];
        T xv[RPT], dg[RPT], v[TPT];
        int id[TPT];
        int lp[RPT], ln[RPT], lpe;
    };
    struct Stg {  // staged terms lt + j NL of a chunk
        int slot[TPT], j[TPT];
    };
    struct StgY {  // ... and their y
        int slot[TPT];
        T y[TPT];
    };
    // Loads past the chunk's rows / terms are predicated off (a whole wave
    // past them issues nothing): the staging is bound by this CU's load
    // bandwidth, and a chunk of short rows fills a fraction of its term slots.
    auto load_pre = [&](const rsp::LevelChunk &ch) {
        Pre p;
        const int nl = ch.l1 - ch.l0;
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const int x = ch.x0 + lt + rr * NL;
            if (lt >= 0 && x < ch.x1) {
                p.r[rr] = a.plan.trow[x];
                p.xv[rr] = sx[x];
                p.dg[rr] = KIND == 2 ? sdg[x] : T(0);
            }
        }
#pragma unroll
        for (int j = 0; j < TPT; ++j) {
            const int k = ch.k0 + lt + j * NL;
            if (lt >= 0 && k < ch.k1) {
                p.v[j] = sval[k];
                p.id[j] = a.plan.sid[k];
            }
        }
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr)
            if (lt >= 0) {
                p.lp[rr] = ptr[ch.l0 + min(lt + rr * NL, nl)];
                p.ln[rr] = a.plan.nshort[ch.l0 + min(lt + rr * NL, max(nl - 1, 0))];
            }
        p.lpe = ptr[ch.l1];
        return p;
    };
    auto load_stg = [&](const rsp::LevelChunk &ch) {
        Stg q;
        const int el = max(ch.st1 - 1, 0);
#pragma unroll
        for (int j = 0; j < TPT; ++j)
            if (lt >= 0) {
                const rsp::StagedTerm t = a.plan.stg[max(min(ch.st0 + lt + j * NL, el), 0)];
                q.slot[j] = t.slot;
                q.j[j] = t.j;
            }
        return q;
    };
    auto load_stgy = [&](const Stg &q) {
        StgY w;
#pragma unroll
        for (int j = 0; j < TPT; ++j)
            if (lt >= 0) {
                w.slot[j] = q.slot[j];
                w.y[j] = y[q.j[j]];
            }
        return w;
    };
    // Chunk switch. The levels write y to the LDS window only; the previous
    // chunk's rows go to global y here, one store per thread, so no global
    // store is pending while levels run and the wait below only ever finds
    // operations issued a whole chunk ago (this chunk's prefetch, the flush
    // before). After it and the barrier, every flush up to the previous switch
    // is complete — the staged y a prefetch reads (producer > kYWin rows back,
    // i.e. in a chunk flushed at least one switch before) is in memory.
    auto mark_by = [&](int c, int j, int t) {  // diagnostics only (RSP_ILU_TRACE)
        if (a.trace && tid == t && 8 * c + j < a.trace_cap / 2) a.trace[8 * c + j] = wall_clock64();
    };
    auto mark = [&](int c, int j) { mark_by(c, j, 0); };
    auto stage = [&](int c, int px0, int px1, const rsp::LevelChunk &ch, const Pre &p, const StgY &w) {
        const int nk = ch.k1 - ch.k0, nl = ch.l1 - ch.l0, ns = ch.st1 - ch.st0;
        mark(c, 0);
        // the previous chunk's levels are done with LDS, and the y flushed at
        // earlier switches (global stores of other threads) are ordered before
        // this chunk's prefetch loads: workgroup-scope release / acquire
        __syncthreads();
        mark(c, 1);
        int fi[RPT];
        T fv[RPT];
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {  // read before this thread restages its slots
            const int t = min(max(lt, 0) + rr * NL, rsp::kChunkRows - 1);
            fi[rr] = lrowi[t];
            fv[rr] = ybuf[(px0 + t - base) & (rsp::kYWin - 1)];
        }
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const int t = lt + rr * NL;
            if (lt >= 0 && t < ch.x1 - ch.x0) {
                ThinRow<T> r;
                r.x = p.xv[rr];
                r.g = p.r[rr].g;
                r.out = (p.r[rr].out & 0xffff) * (int)sizeof(T);
                lrow[t] = r;
                legr[t] = (unsigned char)(p.r[rr].out >> 16);  // early groups (split order)
                lrowi[t] = p.r[rr].i;
                if constexpr (KIND == 2) ldg[t] = p.dg[rr];
            }
        }
#pragma unroll
        for (int j = 0; j < TPT; ++j)
            if (lt >= 0 && lt + j * NL < nk) {
                ((T *)lval)[lt + j * NL] = p.v[j];
                ((int *)lidx)[lt + j * NL] = p.id[j] * (int)sizeof(T);
            }
#pragma unroll
        for (int j = 0; j < TPT; ++j)
            if (lt >= 0 && lt + j * NL < ns) ybuf[kStaged + w.slot[j]] = w.y[j];
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const int t = lt + rr * NL;
            if (lt >= 0 && t <= nl) lptr[t] = p.lp[rr];
            if (lt >= 0 && t < nl) lns[t] = p.ln[rr];
        }
        if (lt == 0 && nl == rsp::kChunkRows) lptr[rsp::kChunkRows] = p.lpe;
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr)  // after the last use of the prefetched registers
            if (lt >= 0 && lt + rr * NL < px1 - px0) y[fi[rr]] = fv[rr];
        lds_barrier();
        mark(c, 2);
    };
    // s += -sum over the terms of one group (in order; pads are exact no-ops)
    auto yb = [&](int off) { return *(const T *)((const char *)ybuf + off); };
    auto put = [&](int off, T v) { *(T *)((char *)ybuf + off) = v; };
    auto group_fma = [&](T s, const TermGroup<T, G> &g, const TermIds<G> &id) {
        T yv[G];
#pragma unroll
        for (int j = 0; j < G; ++j) yv[j] = yb(id.v[j]);
#pragma unroll
        for (int j = 0; j < G; ++j) s = fma_t(-g.v[j], yv[j], s);
        return s;
    };
    // groups [g, ge) of a row after s, in order; group g+1's values, indices
    // and y are read under group g's fmas (the same fmas in the same order)
    auto groups_fma = [&](T s, int g, int ge) {
        TermGroup<T, G> vc = lval[g];
        T yc[G];
        {
            const TermIds<G> ic = lidx[g];
#pragma unroll
            for (int j = 0; j < G; ++j) yc[j] = yb(ic.v[j]);
        }
        for (; g < ge; ++g) {
            const int gn = min(g + 1, ge - 1);
            const TermGroup<T, G> vn = lval[gn];
            const TermIds<G> in = lidx[gn];
            T yn[G];
#pragma unroll
            for (int j = 0; j < G; ++j) yn[j] = yb(in.v[j]);
#pragma unroll
            for (int j = 0; j < G; ++j) s = fma_t(-vc.v[j], yc[j], s);
            vc = vn;
#pragma unroll
            for (int j = 0; j < G; ++j) yc[j] = yn[j];
        }
        return s;
    };
    // (groups_fma for every short row, and for the narrow rows' third group
    // on, measured 1.6 % slower on config 3: short chains gain nothing from
    // the lookahead and pay its loads; long rows gain 10 %)
    auto row_value = [&](const ThinRow<T> &r) {  // one short row, groups in order
        T s = r.x;
        const int g0 = r.g & 0xffff, ng = r.g >> 16;
        for (int g = 0; g < ng; ++g) s = group_fma(s, lval[g0 + g], lidx[g0 + g]);
        return s;
    };
    auto narrow = [&](int q) {
        const int cnt = lptr[q + 1] - lptr[q];
        return cnt <= 64 && lns[q] == cnt;
    };
    auto run_end = [&](int q, int nl) {  // first level >= q that is not narrow, or nl
        for (int b = q;; b += 64) {
            const int qq = b + (tid & 63);
            const unsigned long long m = __ballot(!(qq < nl && narrow(qq)));
            if (m) return b + __builtin_ctzll(m);
        }
    };
    // A lane past a narrow level's last row reads that last row's record (its
    // index is clamped) and so computes the same value into the same slot: no
    // store predicate (duplicate same-address LDS writes cost less than the
    // exec-mask branch of a predicate; measured). The prefetches for levels
    // q+1 / q+2 are unconditional (clamped indices: past the run they read
    // valid records that go unused), so a level is straight-line code; the
    // diagnostics stamp is a separate instantiation (TR), not a branch per level.
    auto narrow_run = [&](const rsp::LevelChunk &ch, int q0, int q1, auto trace_tag) {  // wave 0
        constexpr bool TR = decltype(trace_tag)::value;
        const int lane = tid, x0 = ch.x0, nl = ch.l1 - ch.l0;
        auto lpt = [&](int q) { return lptr[min(q, nl)]; };
        auto ld_row = [&](int p0, int p1) { return max(p0 - x0 + min(lane, p1 - p0 - 1), 0); };
        // level pointers p2, p3 = lptr[q+2], lptr[q+3] (clamped), rolling
        const int p1 = lpt(q0 + 1);
        int p2 = lpt(q0 + 2), p3 = lpt(q0 + 3);
        int cr = ld_row(lpt(q0), p1);
        ThinRow<T> cR = lrow[cr];
        TermIds<G> cI = lidx[cR.g & 0xffff];
        int nr = ld_row(p1, p2);
        ThinRow<T> nR = lrow[nr];
        // Drain the prologue's LDS loads here: the compiler merges the wait
        // state of the loop entry into the loop head, and with these loads
        // pending there it waits at the head of EVERY level — which in the
        // steady state is a wait for the previous level's y store.
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
        for (int q = q0; q < q1; ++q) {
            // loads for later levels (none depends on a y): the y indices of
            // level q+1's first group, the row records of level q+2. Term
            // values are not carried: they load with the y, off the critical path.
            const int p4 = lpt(q + 4);
            const TermIds<G> nI = lidx[nR.g & 0xffff];
            const int mr = ld_row(p2, p3);
            const ThinRow<T> mR = lrow[mr];
            // level q: y loads -> fma chain -> y store (the critical path)
            T s;
            const int g0 = cR.g & 0xffff, ng = cR.g >> 16;
            if (__ballot(ng >= 2)) {
                // a row of the level has a second group: every lane loads one
                // (its own, or the pad group) together with the first group's
                // y, so its y loads overlap instead of following the first
                // group's fma chain (one LDS round trip instead of two)
                const int gi = ng >= 2 ? g0 + 1 : kPadGroup;
                const TermIds<G> i2 = lidx[gi];
                s = group_fma(cR.x, lval[g0], cI);
                s = group_fma(s, lval[gi], i2);
                if (__ballot(ng >= 3))
                    for (int g = 2; g < ng; ++g) s = group_fma(s, lval[g0 + g], lidx[g0 + g]);
            } else {
                s = group_fma(cR.x, lval[g0], cI);
            }
            if constexpr (KIND == 2) s = qdiv<T>(s, ldg[cr]);
            put(cR.out, s);
            wave_sync();
            if constexpr (TR) {  // diagnostics: level end stamps
                if (lane == 0 && ch.l0 + q < a.trace_cap / 2)
                    a.trace[a.trace_cap / 2 + ch.l0 + q] = a.trace_clk ? clock64() : wall_clock64();
            }
            cR = nR;
            cr = nr;
            cI = nI;
            nR = mR;
            nr = mr;
            p2 = p3;
            p3 = p4;
        }
    };
    // Narrow run in the SPLIT term order (L / L^T: a row's terms from the
    // level just below it are its last groups, legr[] = the groups before
    // them), wave 0 alone, software-pipelined so that only the late part of a
    // level is on the critical path: after level q's y stores, the wave issues
    // the late y loads of level q+1 and, while they are in flight, finishes
    // level q+1's EARLY partial sum (its producers are two or more levels back,
    // done) and prefetches the records of the levels after; then it waits for
    // the late y, runs the late fmas from the early partial and stores. A
    // wave's LDS accesses are performed in order, so no counter and no barrier
    // orders consecutive levels. Lanes past a level's rows repeat its last row
    // (same value to the same slot); groups past a row's own read the pad
    // group (exact no-op fmas); past the run, records are clamped and unused.
    // Same terms, same order (early then late), same fma chain as every other
    // solve path in the split order: same bits.
    auto narrow_run_split = [&](const rsp::LevelChunk &ch, int q0, int q1) {  // wave 0
        const int lane = tid, x0 = ch.x0, nl = ch.l1 - ch.l0;
        auto lpt = [&](int q) { return lptr[min(q, nl)]; };
        struct Lev {
            ThinRow<T> R;
            int eg;  // early groups; late groups = (R.g >> 16) - eg
        };
        auto lev = [&](int q) {
            const int p0 = lpt(q), p1 = lpt(q + 1);
            const int cr = max(p0 - x0 + min(lane, p1 - p0 - 1), 0);
            Lev v;
            v.R = lrow[cr];
            v.eg = legr[cr];
            return v;
        };
        auto early_grp = [&](const Lev &v, int gi) { return gi < v.eg ? (v.R.g & 0xffff) + gi : kPadGroup; };
        auto late_grp = [&](const Lev &v, int gi) {
            return gi < (v.R.g >> 16) - v.eg ? (v.R.g & 0xffff) + v.eg + gi : kPadGroup;
        };
        auto fma_group = [&](T s, const TermGroup<T, G> &g, const T (&y)[G]) {
#pragma unroll
            for (int j = 0; j < G; ++j) s = fma_t(-g.v[j], y[j], s);
            return s;
        };
        auto ygroup = [&](T (&y)[G], const TermIds<G> &id) {
#pragma unroll
            for (int j = 0; j < G; ++j) y[j] = yb(id.v[j]);
        };
        auto nlate = [&](const Lev &v) { return (v.R.g >> 16) - v.eg; };
        Lev c = lev(q0), n = lev(q0 + 1);
        // early partial of level q0 (its early producers are done)
        T e = c.R.x;
        for (int gi = 0; __ballot(gi < c.eg); ++gi) {
            const int gg = early_grp(c, gi);
            e = group_fma(e, lval[gg], lidx[gg]);
        }
        // a level's first two late groups are read ahead (values and y
        // indices do not depend on any y), and their y are loaded together
        // right after the previous level's stores: one LDS round trip on the
        // critical path for rows of up to 2 G late terms
        bool c2 = __ballot(nlate(c) >= 2) != 0;
        TermGroup<T, G> cLV = lval[late_grp(c, 0)], cLV1 = lval[late_grp(c, 1)];
        TermIds<G> nEI = lidx[early_grp(n, 0)];
        TermGroup<T, G> nEV = lval[early_grp(n, 0)];
        T cy[G], cy1[G];
        {
            const TermIds<G> cLI = lidx[late_grp(c, 0)], cLI1 = lidx[late_grp(c, 1)];
            ygroup(cy, cLI);
            ygroup(cy1, cLI1);
        }
        for (int q = q0; q < q1; ++q) {
            // early y of level q+1 (producers two or more levels back)
            T ny[G];
            ygroup(ny, nEI);
            // records of level q+2, the late groups 0 and 1 of level q+1
            const Lev m = lev(q + 2);
            const bool n2 = __ballot(nlate(n) >= 2) != 0;
            const int nlg = late_grp(n, 0), nlg1 = late_grp(n, 1);
            const TermIds<G> nLI = lidx[nlg], nLI1 = lidx[nlg1];
            const TermGroup<T, G> nLV = lval[nlg], nLV1 = lval[nlg1];
            // level q: the late part (critical path)
            T s = fma_group(e, cLV, cy);
            if (c2) {
                s = fma_group(s, cLV1, cy1);
                for (int gi = 2; __ballot(gi < nlate(c)); ++gi) {
                    const int gg = late_grp(c, gi);
                    s = group_fma(s, lval[gg], lidx[gg]);
                }
            }
            put(c.R.out, s);
            wave_sync();
            // late y of level q+1 (after level q's stores)
            ygroup(cy, nLI);
            if (n2) ygroup(cy1, nLI1);
            // level q+1's early partial, under those loads
            T e2 = fma_group(n.R.x, nEV, ny);
            for (int gi = 1; __ballot(gi < n.eg); ++gi) {
                const int gg = early_grp(n, gi);
                e2 = group_fma(e2, lval[gg], lidx[gg]);
            }
            // early group 0 of level q+2
            const int meg = early_grp(m, 0);
            nEI = lidx[meg];
            nEV = lval[meg];
            e = e2;
            c = n;
            n = m;
            c2 = n2;
            cLV = nLV;
            cLV1 = nLV1;
        }
    };
    // Narrow run on K waves (a.narrow_waves): wave w computes levels q0 + w,
    // q0 + w + K, ... A level reads its row records, term indices and values
    // first (nothing there depends on a y), then waits until the run's
    // earlier levels are complete — an LDS counter of absolute levels done,
    // advanced by each level's wave after its y stores — and only then does
    // the critical part: y loads -> fma chain -> y stores. While one wave is
    // on its critical part, the others prepare their next levels, so a level
    // costs about its critical part alone (one wave did all of it in line).
    // The counter is a release store after the wave's y stores (lds_publish)
    // and the waiting wave's poll ends in an acquire fence, so its y loads
    // see them (HIP memory model, workgroup scope).
    // Same terms, same order, same fma chain as narrow_run: same bits.
    auto narrow_run_mw = [&](const rsp::LevelChunk &ch, int q0, int q1, int K) {
        const int w = tid >> 6, lane = tid & 63, x0 = ch.x0;
        const int L0 = ch.l0 + q0;
        for (int q = q0 + w; q < q1; q += K) {
            const int p0 = lptr[q], p1 = lptr[q + 1];
            const int cr = max(p0 - x0 + min(lane, p1 - p0 - 1), 0);
            const ThinRow<T> R = lrow[cr];
            const int g0 = R.g & 0xffff, ng = R.g >> 16;
            const bool two = __ballot(ng >= 2) != 0;
            const int gi = ng >= 2 ? g0 + 1 : kPadGroup;
            const TermIds<G> i1 = lidx[g0];
            const TermGroup<T, G> v1 = lval[g0];
            TermIds<G> i2;
            TermGroup<T, G> v2;
            if (two) {
                i2 = lidx[gi];
                v2 = lval[gi];
            }
            const int L = ch.l0 + q;
            if (L > L0) lds_wait_geq(&lds_done, L);
            T s = group_fma(R.x, v1, i1);
            if (two) {
                s = group_fma(s, v2, i2);
                if (__ballot(ng >= 3))
                    for (int g = 2; g < ng; ++g) s = group_fma(s, lval[g0 + g], lidx[g0 + g]);
            }
            if constexpr (KIND == 2) s = qdiv<T>(s, ldg[cr]);
            put(R.out, s);
            lds_publish(&lds_done, L + 1, lane == 0);  // after the y stores
            if (a.trace && lane == 0 && L < a.trace_cap / 2)  // diagnostics: level end stamps
                a.trace[a.trace_cap / 2 + L] = a.trace_clk ? clock64() : wall_clock64();
        }
    };
    // The same on K waves with TWO consecutive levels per turn (a.narrow_pairs,
    // RSP_ILU_NARROW_PAIRS; L / L^T of DAGs with small levels, see the
    // launcher): wave w takes levels (q0 + 2 (w + jK), + 1). (The same for the thin factor's narrow
    // rounds measured 21.2 -> 26.0 ms — the second level's item preparation
    // lands on the chain — and was removed.)
    // The second level of a pair reads the first's y from this wave's own
    // stores (in-order LDS of one wave, a wavefront fence between), so a
    // pair pays one counter wait and one release instead of two. Before the
    // wait the wave loads both levels' row records and the first level's
    // term groups; the second level's values load with its y. Same terms,
    // same order, same fma chain: same bits.
    auto narrow_run_mw2 = [&](const rsp::LevelChunk &ch, int q0, int q1, int K) {
        const int w = tid >> 6, lane = tid & 63, x0 = ch.x0;
        const int L0 = ch.l0 + q0;
        auto row_of = [&](int q) {
            const int p0 = lptr[q], p1 = lptr[q + 1];
            return max(p0 - x0 + min(lane, p1 - p0 - 1), 0);
        };
        for (int q = q0 + 2 * w; q < q1; q += 2 * K) {
            const bool has2 = q + 1 < q1;  // wave-uniform
            const int cr = row_of(q), cr2 = has2 ? row_of(q + 1) : cr;
            const ThinRow<T> R = lrow[cr], R2 = lrow[cr2];
            const int g0 = R.g & 0xffff, ng = R.g >> 16;
            const bool two = __ballot(ng >= 2) != 0;
            const int gi = ng >= 2 ? g0 + 1 : kPadGroup;
            const TermIds<G> i1 = lidx[g0];
            const TermGroup<T, G> v1 = lval[g0];
            const TermIds<G> j1 = lidx[R2.g & 0xffff];
            TermIds<G> i2;
            TermGroup<T, G> v2;
            if (two) {
                i2 = lidx[gi];
                v2 = lval[gi];
            }
            // LW > 0 (the narrow waves hold no chunk prefetch, so the registers
            // are there): the third group of the first level and the second and
            // third of the second are prepared before the wait as well, so those
            // groups' y loads join the level's first round trip
            const int h0 = R2.g & 0xffff, nh = R2.g >> 16;
            constexpr bool MORE = LW > 0 && G == 2;
            const bool three = MORE && __ballot(ng >= 3) != 0, two2 = MORE && has2 && __ballot(nh >= 2) != 0;
            const bool three2 = MORE && has2 && __ballot(nh >= 3) != 0;
            TermIds<G> i3, j2, j3;
            if (three) i3 = lidx[ng >= 3 ? g0 + 2 : kPadGroup];
            if (two2) j2 = lidx[nh >= 2 ? h0 + 1 : kPadGroup];
            if (three2) j3 = lidx[nh >= 3 ? h0 + 2 : kPadGroup];
            const int L = ch.l0 + q;
            if (L > L0) lds_wait_geq(&lds_done, L);
            T s;
            if (three) {  // groups 0-2 in one round trip
                T ya[3][G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    ya[0][j] = yb(i1.v[j]);
                    ya[1][j] = yb(i2.v[j]);
                    ya[2][j] = yb(i3.v[j]);
                }
                const TermGroup<T, G> v3 = lval[ng >= 3 ? g0 + 2 : kPadGroup];
                s = R.x;
#pragma unroll
                for (int j = 0; j < G; ++j) s = fma_t(-v1.v[j], ya[0][j], s);
#pragma unroll
                for (int j = 0; j < G; ++j) s = fma_t(-v2.v[j], ya[1][j], s);
#pragma unroll
                for (int j = 0; j < G; ++j) s = fma_t(-v3.v[j], ya[2][j], s);
                if (__ballot(ng >= 4))
                    for (int g = 3; g < ng; ++g) s = group_fma(s, lval[g0 + g], lidx[g0 + g]);
            } else {
                s = group_fma(R.x, v1, i1);
                if (two) {
                    s = group_fma(s, v2, i2);
                    if (!MORE && __ballot(ng >= 3))
                        for (int g = 2; g < ng; ++g) s = group_fma(s, lval[g0 + g], lidx[g0 + g]);
                }
            }
            if constexpr (KIND == 2) s = qdiv<T>(s, ldg[cr]);
            put(R.out, s);
            if (has2) {
                wave_sync();
                T t;
                if (two2) {  // groups 0-1 (or 0-2) in one round trip
                    T yb0[G], yb1[G], yb2[G];
#pragma unroll
                    for (int j = 0; j < G; ++j) {
                        yb0[j] = yb(j1.v[j]);
                        yb1[j] = yb(j2.v[j]);
                        if (three2) yb2[j] = yb(j3.v[j]);
                    }
                    const TermGroup<T, G> w0 = lval[h0], w1 = lval[nh >= 2 ? h0 + 1 : kPadGroup];
                    TermGroup<T, G> w2;
                    if (three2) w2 = lval[nh >= 3 ? h0 + 2 : kPadGroup];
                    t = R2.x;
#pragma unroll
                    for (int j = 0; j < G; ++j) t = fma_t(-w0.v[j], yb0[j], t);
#pragma unroll
                    for (int j = 0; j < G; ++j) t = fma_t(-w1.v[j], yb1[j], t);
                    if (three2) {
#pragma unroll
                        for (int j = 0; j < G; ++j) t = fma_t(-w2.v[j], yb2[j], t);
                    }
                    const int gn = three2 ? 3 : 2;
                    if (__ballot(nh > gn))
                        for (int g = gn; g < nh; ++g) t = group_fma(t, lval[h0 + g], lidx[h0 + g]);
                } else {
                    t = group_fma(R2.x, lval[h0], j1);
                    if (__ballot(nh >= 2))
                        for (int g = 1; g < nh; ++g) t = group_fma(t, lval[h0 + g], lidx[h0 + g]);
                }
                if constexpr (KIND == 2) t = qdiv<T>(t, ldg[cr2]);
                put(R2.out, t);
            }
            lds_publish(&lds_done, L + (has2 ? 2 : 1), lane == 0);  // after the y stores
            if (a.trace && lane == 0 && L + 1 < a.trace_cap / 2)  // diagnostics: pair end stamps
                a.trace[a.trace_cap / 2 + L + 1] = a.trace_clk ? clock64() : wall_clock64();
        }
    };
    // NAR: this thread may compute narrow runs (the loaders of LW > 0 never
    // do: their instance of levels() leaves that code, and its registers, out)
    auto levels = [&](const rsp::LevelChunk &ch, auto nar) {
        constexpr bool NAR = decltype(nar)::value;
        const int x0 = ch.x0, nl = ch.l1 - ch.l0;
        for (int q = 0; q < nl;) {
            if (narrow(q)) {
                const int qe = run_end(q, nl);
                if constexpr (NAR) {
                const int K = min(a.narrow_waves, LW > 0 ? LW : (int)(blockDim.x >> 6));  // waves of this launch
                if (KIND != 2 && G == 2 && a.narrow_split) {  // (G = 4: the registers are not there)
                    if constexpr (KIND != 2 && G == 2)
                        if (tid < 64) narrow_run_split(ch, q, qe);
                } else if (PAIRS && K > 1) {  // (its own instantiation: the registers)
                    if constexpr (PAIRS)
                        if (tid < 64 * K) narrow_run_mw2(ch, q, qe, K);
                } else if (K > 1) {
                    if (tid < 64 * K) narrow_run_mw(ch, q, qe, K);
                } else if (tid < 64) {
                    if (a.trace)
                        narrow_run(ch, q, qe, std::true_type());
                    else
                        narrow_run(ch, q, qe, std::false_type());
                }
                }
                lds_barrier();
                q = qe;
                continue;
            }
            const int l = ch.l0 + q;
            const int lp = lptr[q], off = lp - x0, cnt = lptr[q + 1] - lp, ns = lns[q];
            if (tid < ns) {  // (ns <= kChunkRows <= NTH)
                const ThinRow<T> r = lrow[off + tid];
                T s = row_value(r);
                if constexpr (KIND == 2) s = qdiv<T>(s, ldg[off + tid]);
                put(r.out, s);
            }
            for (int r = ns + (tid >> 6); r < cnt; r += NTH / 64) {  // long rows: a wave each
                const ThinRow<T> t = lrow[off + r];
                // every lane runs the row's chain on broadcast LDS operands,
                // group g+1's values, indices and y read under group g's fmas
                // (the same terms in the same order as wave_chain: same bits)
                const int g0 = t.g & 0xffff, ng = t.g >> 16;
                T s = ng > 0 ? groups_fma(t.x, g0, g0 + ng) : t.x;
                if constexpr (KIND == 2) s = qdiv<T>(s, ldg[off + r]);
                if ((tid & 63) == 0) put(t.out, s);
            }
            lds_barrier();
            if (a.trace && tid == 0 && l < a.trace_cap / 2)  // diagnostics: level end stamps
                a.trace[a.trace_cap / 2 + l] = a.trace_clk ? clock64() : wall_clock64();
            ++q;
        }
    };
    // chunk records through the constant address space: scalar loads, which
    // the y stores cannot alias and which leave vmcnt to the prefetch
    auto chunk = [&](int c) { return load_chunk(a.plan.chunks, c); };
    // Pipeline: while chunk c's levels run, the streams of chunk c+1 and the y
    // of its staged terms (their list loaded one chunk earlier) are loading,
    // and the staged-term list of chunk c+2. Streams have no dependent loads,
    // so one chunk of lead hides them.
    const int cl = c1 - 1;
    int px0 = 0, px1 = 0;  // the chunk to flush at the next switch
    if (LW == 0 || lt >= 0) {  // the loaders (every thread when LW == 0)
        rsp::LevelChunk rc = chunk(c0), rn = chunk(min(c0 + 1, cl));
        Pre p = load_pre(rc);
        StgY w = load_stgy(load_stg(rc));
        Stg sn = load_stg(rn);
        for (int c = c0; c < c1; ++c) {
            stage(c, px0, px1, rc, p, w);
            const rsp::LevelChunk cur = rc;
            if (c + 1 < c1) {
                const rsp::LevelChunk r2 = chunk(min(c + 2, cl));
                p = load_pre(rn);                           // chunk c+1's streams
                if (rn.st1 > rn.st0) w = load_stgy(sn);     // ... and its staged y
                if (r2.st1 > r2.st0) sn = load_stg(r2);     // chunk c+2's staged terms
                rc = rn;
                rn = r2;
            }
            mark_by(c, 4, 0);  // diagnostics: prefetch issued (wave 0 / last wave)
            mark_by(c, 5, NTH - 64);
            levels(cur, std::integral_constant<bool, LW == 0>());
            mark(c, 3);
            px0 = cur.x0;
            px1 = cur.x1;
        }
    } else {  // the first LW waves: the same barriers, no prefetch (so none of its registers)
        for (int c = c0; c < c1; ++c) {
            const rsp::LevelChunk cur = chunk(c);
            mark(c, 0);
            __syncthreads();  // stage(): the loaders restage the chunk between these two
            mark(c, 1);
            lds_barrier();
            mark(c, 2);
            mark_by(c, 4, 0);
            levels(cur, std::true_type());
            mark(c, 3);
            px0 = cur.x0;
            px1 = cur.x1;
        }
    }
    // the last chunk's rows (its levels ended with a barrier)
    for (int t = tid; t < px1 - px0; t += NTH) y[lrowi[t]] = ybuf[(px0 + t - base) & (rsp::kYWin - 1)];
}

template <typename T, int KIND, int B>
static hipError_t launch_solve(const TrsvArgs &a, hipStream_t s) {
    const LevelPlan &P = a.plan;
    const T alpha = (T)a.alpha;
    {  // the streams every level reads (term values, alpha x_i, u_ii in level order)
        const int nk = max(P.nterms, a.n);
        if (nk > 0) hipLaunchKernelGGL((trsv_stream<T, KIND>), dim3((nk + 255) / 256), dim3(256), 0, s, a, alpha);
    }
    for (int g = 0; g < P.nseg; ++g) {
        const rsp::LevelSeg sg = P.segs[g];
        if (sg.thin) {
            // term groups of 2 for DAGs of short chains (the plan padded them so)
            // the two-levels-per-turn narrow runs (L / L^T): RSP_ILU_NARROW_PAIRS
            // 1 / 0 forces them; by default (-1) for DAGs of <= 32 rows per
            // level on average (the deep circuits: config 3, same box, dc1
            // 5.18 -> 4.94 ms, matrix-new_3 6.09 -> 5.81, G2_circuit 3.45 ->
            // 3.22; on wider DAGs' narrow runs they cost: parabolic_fem 3.55
            // -> 3.95, Dubcova3 2.59 -> 2.84, thermomech_TK 0.95 -> 1.00)
            const bool pr = KIND != 2 && (a.narrow_pairs > 0 || (a.narrow_pairs < 0 && a.n <= 32LL * P.nlev));
            // the pair loop's waves never load the next chunk (LW = 4;
            // RSP_ILU_LOADERS=0 turns that off)
            const bool ldr = pr && a.loaders != 0;
            auto kern = P.group == 2 ? (pr ? (ldr ? trsv_thin_pf<T, KIND, 2, KIND != 2, 4> : trsv_thin_pf<T, KIND, 2, KIND != 2>)
                                           : trsv_thin_pf<T, KIND, 2>)
                                     : (pr ? (ldr ? trsv_thin_pf<T, KIND, 4, KIND != 2, 4> : trsv_thin_pf<T, KIND, 4, KIND != 2>)
                                           : trsv_thin_pf<T, KIND, 4>);
            hipLaunchKernelGGL(kern, dim3(1), dim3(kThinThreads), 0, s, a, sg.c0, sg.c1, P.ptr_host[sg.lb]);
            continue;
        }
        if (a.flow && sg.c1 > sg.c0) {  // flow segment: one persistent launch
            launch_flow<trsv_flow<T, KIND, true>, trsv_flow<T, KIND, false>>(a, sg.c0, sg.c1, s);
            continue;
        }
        for (int l = sg.lb; l < sg.le; ++l) {
            const int off = P.ptr_host[l], cnt = P.ptr_host[l + 1] - off;
            if (cnt <= 0) continue;
            const int ns = P.nshort_host[l], nb = (ns + 255) / 256;
            const int nw = P.nwave_host ? P.nwave_host[l] : cnt, nwb = (nw - ns + 3) / 4;
            const int sb = P.sbase_host ? P.sbase_host[l] : -1;
            hipLaunchKernelGGL((trsv_level<T, KIND, B>), dim3(nb + nwb + (cnt - nw)), dim3(256), 0,
                               s, a, off, cnt, ns, nb, nw, nwb, sb);
        }
    }
    return hipGetLastError();
}

// batch width from the plan (2, 4 or 8)
template <typename T, int KIND>
static hipError_t solve_dispatch(const TrsvArgs &a, hipStream_t s) {
    switch (a.plan.batch) {
        case 2: return launch_solve<T, KIND, 2>(a, s);
        case 4: return launch_solve<T, KIND, 4>(a, s);
        default: return launch_solve<T, KIND, 8>(a, s);
    }
}

hipError_t trsv_lower_n_f32(const TrsvArgs &a, hipStream_t s) { return solve_dispatch<float, 0>(a, s); }
hipError_t trsv_lower_t_f32(const TrsvArgs &a, hipStream_t s) { return solve_dispatch<float, 1>(a, s); }
hipError_t trsv_upper_f32(const TrsvArgs &a, hipStream_t s) { return solve_dispatch<float, 2>(a, s); }

void warm_ilu() {  // see rsp_kernels.h
    int o = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, trsv_stream<float, 0>, 256, 0);
}
#ifndef RSP_FTZ_BUILD
hipError_t trsv_lower_n_f64(const TrsvArgs &a, hipStream_t s) { return solve_dispatch<double, 0>(a, s); }
hipError_t trsv_lower_t_f64(const TrsvArgs &a, hipStream_t s) { return solve_dispatch<double, 1>(a, s); }
hipError_t trsv_upper_f64(const TrsvArgs &a, hipStream_t s) { return solve_dispatch<double, 2>(a, s); }
#endif

}  // namespace RSP_KNS
