// ilu0.hip — level-scheduled ILU(0) factorisation for gfx950, replacing
// cusparse?csrilu02 (GPU/ilu0.cu:257-282). The triangular solves over the
// same level plans are trsv.hip; the arithmetic and LDS primitives both use
// are ilu_device.h, the flow launches' scheduler ilu_flow.h.
//
// The analysis (rsp_ilu0_analysis, host) groups rows into dependency levels:
// row i depends on every row k < i with a_ik in the pattern (factor and
// L-solve), and for L^T on every row j > i with l_ji in the pattern. Rows of
// one level are independent. Execution follows the level plan's segments:
//   * fat level  -> one launch over its rows (the kernel boundary is the
//                   inter-level barrier);
//   * thin run   -> ONE launch of a single 1024-thread workgroup that walks a
//                   run of consecutive small levels with __syncthreads()
//                   between them (every row of the run is produced and
//                   consumed inside one CU, so the workgroup barrier orders
//                   it; rows of earlier fat levels come from earlier launches).
// Deep level sets (circuits: ~10^4 levels of ~10 rows) thus cost one launch
// per run instead of one per level.
//
// Arithmetic (identical in the CPU oracle, so results are bitwise equal):
//   factor, row i, k ascending over its lower entries:
//       l_ik = a_ik / u_kk;  a_ij = fma(-l_ik, u_kj, a_ij) for j > k in row k ∩ row i
//   evaluated in pull form: every position applies its own precomputed update
//   list in k order (same fma sequence per position), so the positions of a
//   row run in parallel lanes except where l_ij needs an l_ik of its own row.
// Zero pivots: the smallest i with u_ii == 0 after the factor (atomicMin),
// structural zeros (missing a_ii) are reported by the analysis.
//
// Compiled twice like spmv.hip (rsp_k / rsp_k_ftz).

#include <hip/hip_runtime.h>

#include <type_traits>
#include <limits.h>

#include "ilu_device.h"
#include "ilu_flow.h"

namespace RSP_KNS {

using rsp::IluArgs;
using rsp::kIluWaves;
using rsp::kThinThreads;
using rsp::LevelPlan;

// One position of the factor, pull form: v = a_p - sum_k l_ik u_kj over the
// position's update list (k ascending, one fma each — the same sequence of
// roundings as the IKJ loop).
template <typename T, int B>
__device__ __forceinline__ T factor_entry(const IluArgs &a, const T *vals, int p) {
    const int *ul = a.upd_l, *uu = a.upd_u;
    return fma_chain<T, B>(vals[p], a.upd_ptr[p], a.upd_ptr[p + 1],
                           [&](int u) { return vals[ul[u]]; },
                           [&](int u) { return vals[uu[u]]; });
}

// ILU(0) of row i by the 64 lanes of a wave: lower positions stage by stage
// (a stage's positions depend only on earlier stages of the row and on
// earlier rows), l_ij = v / u_jj, then every upper position at once.
template <typename T, int B>
__device__ __forceinline__ void factor_row(const IluArgs &a, int i, int lane) {
    T *vals = (T *)a.vals;
    const int rs = a.rowptr[i], re = a.rowptr[i + 1], di = a.dpos[i];
    for (int s = rs; s < di;) {
        const int e = a.lend[s];
        for (int x = s + lane; x < e; x += 64) {
            const int p = a.lord[x];
            const int k = a.colidx[p];
            const T ukk = a.hasdiag[k] ? vals[a.dpos[k]] : T(0);
            vals[p] = qdiv<T>(factor_entry<T, B>(a, vals, p), ukk);
        }
        // this stage's l_ik visible to the next stage's lanes
        __threadfence_block();
        s = e;
    }
    for (int p = di + lane; p < re; p += 64) {
        const T v = factor_entry<T, B>(a, vals, p);
        vals[p] = v;
        if (p == di && a.hasdiag[i] && v == T(0)) atomicMin(a.zero_pivot, i);
    }
}

// --------------------------------------------------------------- kernels

// Fat level, global-memory path: one wave per row.
template <typename T, int B>
__global__ __launch_bounds__(64 * kIluWaves) void ilu0_level(IluArgs a, int off, int nrows) {
    const int w = blockIdx.x * kIluWaves + (threadIdx.x >> 6);
    if (w >= nrows) return;
    factor_row<T, B>(a, a.plan.rows[off + w], threadIdx.x & 63);
}

// The stages of one fat-level row on LDS operands (ilu0_level_lds and
// ilu0_level_slot): lower positions stage by stage, l_ij = v / u_jj, then the
// upper positions; rv holds the row's values on entry and its factor on exit.
template <typename T>
__device__ __forceinline__ void row_lds_factor(T *rv, const T *dv, const T *pu, const int *up,
                                               const int *lo, const int *le, const unsigned short *pl,
                                               int nlo, int nr, int lane, int hasdiag, int i,
                                               int *zero_pivot) {
    wave_sync();
    auto entry = [&](int x) {  // a_ij - sum l_ik u_kj over its pairs, k ascending
        T v = rv[x];
        const int u0 = up[x], u1 = up[x + 1];
        auto batch = [&](int u) {
            T l[4], w[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int uu = min(u + b, u1 - 1);
                l[b] = rv[pl[uu]];
                w[b] = pu[uu];
            }
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (u + b < u1) v = fma_t(-l[b], w[b], v);
        };
        if (u1 > u0) {  // the first batch straight-line
            batch(u0);
            for (int u = u0 + 4; u < u1; u += 4) batch(u);
        }
        return v;
    };
    for (int s = 0; s < nlo;) {  // lower positions, stage by stage
        const int e = le[s];
        for (int x = s + lane; x < e; x += 64) {
            const int r = lo[x];
            const T d = dv[r];  // read before the chain, not after it
            rv[r] = qdiv<T>(entry(r), d);
        }
        wave_sync();
        s = e;
    }
    for (int x = nlo + lane; x < nr; x += 64) {  // upper positions (never operands of this row)
        const T v = entry(x);
        rv[x] = v;
        if (x == nlo && hasdiag && v == T(0)) atomicMin(zero_pivot, i);
    }
    wave_sync();
}

// Fat level, one wave (workgroup) per row with the row staged in LDS. Every
// operand that does not come from the row itself is final before the level
// starts: the u_kj of all the row's update pairs (rows of earlier levels)
// and its divisors u_kk. So they, the row's values and its stage structure
// are loaded up front in a few independent memory round trips; the stages
// then run on LDS operands only (an l_ik of an earlier stage is the row's own
// LDS value; one wave's LDS accesses are in order), and the row is written
// back once. Same per-position fma sequence and division as factor_row, so
// bitwise equal to it. Rows beyond kFacRow entries or kFacPairs pairs take
// the global path (factor_row).
template <typename T, int B>
__global__ __launch_bounds__(64) void ilu0_level_lds(IluArgs a, int off) {
    constexpr int R = rsp::kFacRow, Q = rsp::kFacPairs;
    __shared__ T rv[R], dv[R], pu[Q];
    __shared__ int up[R + 1], lo[R], le[R];
    __shared__ unsigned short pl[Q];
    const int lane = threadIdx.x;
    const rsp::FacRow fr = a.frow[off + blockIdx.x];
    T *vals = (T *)a.vals;
    const int i = fr.i, rs = fr.rs, re = fr.re, q0 = fr.q0;
    const int nr = re - rs, nq = fr.q1 - q0, nlo = fr.di - rs;
    if (nr > R || nq > Q) {
        factor_row<T, B>(a, i, lane);
        return;
    }
    for (int x = lane; x < nr; x += 64) {
        const bool lower = x < nlo;
        const int d = lower ? a.udiv[rs + x] : -1;
        rv[x] = vals[rs + x];
        dv[x] = d >= 0 ? vals[d] : T(0);
        up[x] = a.upd_ptr[rs + x] - q0;
        if (lower) {
            lo[x] = a.lord[rs + x] - rs;
            le[x] = a.lend[rs + x] - rs;
        }
    }
    if (lane == 0) up[nr] = nq;
    for (int u = lane; u < nq; u += 64) {
        pl[u] = (unsigned short)(a.upd_l[q0 + u] - rs);
        pu[u] = vals[a.upd_u[q0 + u]];
    }
    row_lds_factor<T>(rv, dv, pu, up, lo, le, pl, nlo, nr, lane, fr.hasdiag, i, a.zero_pivot);
    for (int x = lane; x < nr; x += 64) vals[rs + x] = rv[x];
}

// Fat level in the slot layout (rsp::FacSlotLevel): the row's structure is
// one fixed-stride slot, so its header, divisor positions, packed stage
// structure and update pairs are one memory round trip, issued together
// (KR / KQ = the level's entries / pairs per lane, compile-time, loads
// clamped and unpredicated); the values they point at (the row's a_ij, its
// divisors u_kk, the u_kj of its pairs) are the second. ilu0_level_lds reads
// a record first and then loops over its arrays, a dependent round trip per
// 64 pairs. Same LDS stages (row_lds_factor), so the same bits.
template <typename T, int KR, int KQ>
__global__ __launch_bounds__(64) void ilu0_level_slot(IluArgs a, const int *__restrict__ lvl, int stride,
                                                      int rm, int qm) {
    constexpr int R = rsp::kFacRow, Q = rsp::kFacPairs;
    static_assert(KR * 64 <= R && KQ * 64 <= Q, "slot kernel budgets");
    __shared__ T rv[R], dv[R], pu[Q];
    __shared__ int up[R + 1], lo[R], le[R];
    __shared__ unsigned short pl[Q];
    const int lane = threadIdx.x;
    const int *slot = lvl + (size_t)blockIdx.x * stride;
    const int pa = rsp::fac_pairs_at(rm);
    int dpos_[KR], bw[KR];
    int2 pr[KQ];
#pragma unroll
    for (int k = 0; k < KR; ++k) {  // clamped to the level's region sizes (rm, qm >= 1 here)
        const int x = min(lane + 64 * k, rm - 1);
        dpos_[k] = slot[8 + x];
        bw[k] = slot[8 + rm + x];
    }
#pragma unroll
    for (int k = 0; k < KQ; ++k)
        pr[k] = *reinterpret_cast<const int2 *>(slot + pa + 2 * min(lane + 64 * k, qm - 1));
    const int i = slot[0], rs = slot[1], nlo = slot[2], nr = slot[3], nq = slot[4];
    const int hasdiag = slot[5], global = slot[6];
    if (nr == 0) return;  // (an empty row has no lower entries: it is never in a slot level)
    if (global) {
        factor_row<T, 4>(a, i, lane);
        return;
    }
    T *vals = (T *)a.vals;
    T av[KR], dd[KR], uv[KQ];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        const int x = min(lane + 64 * k, nr - 1);
        av[k] = vals[rs + x];
        dd[k] = vals[max(dpos_[k], 0)];
    }
#pragma unroll
    for (int k = 0; k < KQ; ++k) uv[k] = vals[pr[k].x];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        const int x = lane + 64 * k;
        if (x < nr) {
            rv[x] = av[k];
            dv[x] = dpos_[k] >= 0 ? dd[k] : T(0);
            up[x] = bw[k] & 0x7ff;
            lo[x] = (bw[k] >> 11) & 0x1ff;
            le[x] = (bw[k] >> 20) & 0x1ff;
        }
    }
    if (lane == 0) up[nr] = nq;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const int u = lane + 64 * k;
        if (u < nq) {
            pl[u] = (unsigned short)pr[k].y;
            pu[u] = uv[k];
        }
    }
    row_lds_factor<T>(rv, dv, pu, up, lo, le, pl, nlo, nr, lane, hasdiag, i, a.zero_pivot);
    for (int x = lane; x < nr; x += 64) vals[rs + x] = rv[x];
}

// Before a factor call's flow runs (one launch over all their items): each
// flow row's upper part (diagonal included) — the values its consumers read
// as u_kk and u_kj — is saved to forig and replaced by kNotYet in vals, so
// that vals itself tells a consumer whether an operand is final (the
// data-tagged hand-off trsv_flow uses for y). A wave per item.
template <typename T>
__global__ __launch_bounds__(256) void ilu0_flow_prep(IluArgs a, int nitems) {
    const int lane = threadIdx.x & 63;
    const int it = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= nitems) return;
    const int *slot = a.fslots + a.fitems[it].off;
    const int rs = slot[1], nlo = slot[2], nr = slot[3];
    T *vals = (T *)a.vals, *orig = (T *)a.forig;
    typedef typename FlowWord<T>::U U;
    for (int x = nlo + lane; x < nr; x += 64) {
        orig[rs + x] = vals[rs + x];
        reinterpret_cast<U *>(vals)[rs + x] = FlowWord<T>::kNotYet;
    }
}

// Flow run of the factor (rsp::FacFlowRun): ONE launch of a.flow_grid
// workgroups over the run's rows in level order instead of a launch per fat
// level; the waves walk the items statically or by claims (FlowClaims,
// rsp::FlowCtl). The hand-off is DATA-TAGGED, as trsv_flow's: the rows of
// flow runs start the call with their upper values (the u_kk and u_kj other
// rows read) set to kNotYet by ilu0_flow_prep (originals in forig); a row
// reads its operands (divisors and update-pair values) straight from vals
// with agent-scope atomic loads and re-reads those still kNotYet; the
// producer publishes each final value with one agent-scope atomic store.
// Every hand-off is a single location written once by an atomic and read by
// atomics (coherence alone orders it under the HIP memory model): no flag,
// no fence, no dependency lookup. Operands of rows outside flow runs are
// final in vals (earlier kernels) and never kNotYet. A gate row three levels
// back is polled first (lane 0, its first upper value) so that waves far
// ahead of the front poll one word. Progress as trsv_flow (an item waits
// for lower items only); a wait past fc.ticks gives up (rsp::FlowCtl).
// Config 3 against the round-3 flag hand-off (flags stored relaxed after an
// s_waitcnt, which the HIP memory model does not order): fp64 factor 58.6 ->
// 59.5 ms; the same flags with an agent-scope release / acquire pair (an L2
// write-back and an L2 invalidate per row) took 116 ms. Structure and
// arithmetic as ilu0_level_slot (the level's rm / qm at run time, budgets
// KR / KQ at their maximum): the same bits.
template <typename T, bool TK>
__global__ __launch_bounds__(256) void ilu0_flow(IluArgs a, int it0, int it1, unsigned long long base) {
    constexpr int R = rsp::kFacRow, Q = rsp::kFacPairs, KR = R / 64, KQ = Q / 64;
    typedef typename FlowWord<T>::U U;
    __shared__ T rv_[4][R], dv_[4][R], pu_[4][Q];
    __shared__ int up_[4][R + 1], lo_[4][R], le_[4][R];
    __shared__ unsigned short pl_[4][Q];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *rv = rv_[wv], *dv = dv_[wv], *pu = pu_[wv];
    int *up = up_[wv], *lo = lo_[wv], *le = le_[wv];
    unsigned short *pl = pl_[wv];
    T *vals = (T *)a.vals;
    const T *orig = (const T *)a.forig;
    __shared__ std::conditional_t<TK, FlowTicketLds, int> tl_;  // (tickets only)
    FlowClaims<TK> fq(a.fc, base, it0, it1, blockIdx.x * 4 + wv, (int)gridDim.x * 4, reinterpret_cast<FlowTicketLds *>(&tl_));
    for (fq.first(); fq.more(); fq.next()) {
        const int it = fq.item();
        if (it >= it1) continue;  // (tickets: a last round's spare waves)
        const rsp::FacFlowItem f = a.fitems[it];
        const int *slot = a.fslots + f.off;
        const int rm = f.rmqm & 0xffff, qm = f.rmqm >> 16, pa = rsp::fac_pairs_at(rm);
        int dpos_[KR], bw[KR];
        int2 pr[KQ];
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (64 * k < rm) {
                const int x = min(lane + 64 * k, rm - 1);
                dpos_[k] = slot[8 + x];
                bw[k] = slot[8 + rm + x];
            }
#pragma unroll
        for (int k = 0; k < KQ; ++k)
            if (64 * k < qm) pr[k] = *reinterpret_cast<const int2 *>(slot + pa + 2 * min(lane + 64 * k, qm - 1));
        const int i = slot[0], rs = slot[1], nlo = slot[2], nr = slot[3], nq = slot[4], hasdiag = slot[5];
        int gp = -1, ge = -1;  // the gate row's first upper position and its row end
        if (f.gate >= 0 && lane == 0) {
            gp = a.dpos[f.gate];
            ge = a.rowptr[f.gate + 1];
        }
        fq.claim_ahead();  // behind this item's structure loads
        // the row's own a_ij: lower part from vals, upper part from forig
        // (its vals entries hold kNotYet until this row publishes them)
        T av[KR];
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (64 * k < rm) {
                const int x = min(lane + 64 * k, max(nr - 1, 0));
                av[k] = x < nlo ? vals[rs + x] : orig[rs + x];
            }
        // yl: a wait yielded (tickets, FlowClaims::expire): the item still
        // runs through on what it has, but stores nothing and runs again
        // later — no branch out of the polling loops (the structured control
        // flow of such an exit cost the factor ~9 %, config-3 FEM subset)
        int gate_yl = 0;
        if (lane == 0 && gp >= 0 && gp < ge) {
            U gw[1] = {flow_load(vals + gp)};
            const int gpos[1] = {gp};
            const bool gn[1] = {true};
            gate_yl = tagged_wait<T, 1>(gw, gpos, gn, vals, fq, a.flow_sleep, false);
        }
        bool yl = __builtin_amdgcn_readfirstlane(gate_yl) != 0;
        // operands: divisors u_kk of the lower entries, u_kj of the update pairs
        U dw[KR], uw[KQ];
        int dp[KR], upos[KQ];
        bool dn[KR], un[KQ];
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            dn[k] = 64 * k < rm && lane + 64 * k < nlo && dpos_[k] >= 0;
            dp[k] = 64 * k < rm ? max(dpos_[k], 0) : 0;
            dw[k] = 64 * k < rm ? flow_load(vals + dp[k]) : U(0);
        }
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            un[k] = 64 * k < qm && lane + 64 * k < nq;
            upos[k] = 64 * k < qm ? pr[k].x : 0;
            uw[k] = 64 * k < qm ? flow_load(vals + upos[k]) : U(0);
        }
        if (tagged_wait<T, KR>(dw, dp, dn, vals, fq, a.flow_sleep, yl)) yl = true;
        if (tagged_wait<T, KQ>(uw, upos, un, vals, fq, a.flow_sleep, yl)) yl = true;
        if (nr > 0) {
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                const int x = lane + 64 * k;
                if (64 * k < rm && x < nr) {
                    rv[x] = av[k];
                    dv[x] = dpos_[k] >= 0 ? __builtin_bit_cast(T, dw[k]) : T(0);
                    up[x] = bw[k] & 0x7ff;
                    lo[x] = (bw[k] >> 11) & 0x1ff;
                    le[x] = (bw[k] >> 20) & 0x1ff;
                }
            }
            if (lane == 0) up[nr] = nq;
#pragma unroll
            for (int k = 0; k < KQ; ++k) {
                const int u = lane + 64 * k;
                if (64 * k < qm && u < nq) {
                    pl[u] = (unsigned short)pr[k].y;
                    pu[u] = __builtin_bit_cast(T, uw[k]);
                }
            }
            // (after a yield: a zero pivot found here is real — a pivot built
            // from a kNotYet operand is a NaN — and the rerun finds it again)
            row_lds_factor<T>(rv, dv, pu, up, lo, le, pl, nlo, nr, lane, hasdiag, i, a.zero_pivot);
            if (!yl)
                for (int x = lane; x < nr; x += 64) flow_store(vals + rs + x, flow_publishable(rv[x]));
        }
        fq.item_end(it, yl);
    }
}

// The whole factor of a pattern without update pairs (IluArgs::fac_one: a
// stored lower triangle): l_ik = a_ik / u_kk for every lower position, where
// u_kk = a_kk is never updated, and the zero-pivot check of each diagonal; a
// thread per row. Per position the division factor_row and row_lds_factor
// make (no fma: the update lists are empty), the divisor read as they read
// it (0 for a row without diagonal): the same bits. Diagonals are only read,
// so the rows are independent. One launch instead of the L DAG's levels
// (G2_circuit: 5 799) or of the one-level plan's per-row workgroups. A row
// with more than kScaleRow lower entries (a circuit's hub row: thousands, a
// serial chain of dependent gathers for one thread) is listed in LDS and
// done by the whole workgroup after its short rows.
template <typename T>
__global__ __launch_bounds__(256) void ilu0_scale_lower(IluArgs a) {
    constexpr int kScaleRow = 32;
    __shared__ int hub[256];
    __shared__ int nhub;
    if (threadIdx.x == 0) nhub = 0;
    __syncthreads();
    T *vals = (T *)a.vals;
    auto scale = [&](int p) {
        const int k = a.colidx[p];
        const T ukk = a.hasdiag[k] ? vals[a.dpos[k]] : T(0);
        vals[p] = qdiv<T>(vals[p], ukk);
    };
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) {
        const int rs = a.rowptr[i], di = a.dpos[i];
        if (di - rs <= kScaleRow)
            for (int p = rs; p < di; ++p) scale(p);
        else
            hub[atomicAdd(&nhub, 1)] = i;
        if (a.hasdiag[i] && vals[di] == T(0)) atomicMin(a.zero_pivot, i);
    }
    __syncthreads();
    for (int h = 0; h < nhub; ++h) {
        const int r = hub[h], di = a.dpos[r];
        for (int p = a.rowptr[r] + (int)threadIdx.x; p < di; p += 256) scale(p);
    }
}

// Thin run of the factor in ROUNDS (plan: build_factor_plan; rsp::RndChunk,
// rsp::RndItem), one 1024-thread workgroup. A round's items (positions) are
// independent: each is v = a_ij - sum_k l_ik u_kj over its update pairs (k
// ascending, one fma each — the oracle's rounding sequence), then / u_kk for
// a lower item; its operands are earlier rounds' values. Per chunk, LDS holds
// V = [chunk slots, buffer 0 | chunk slots, buffer 1 | staged | 0] (this
// chunk's and the previous chunk's values alternate buffers), the item
// records, the update pairs as operand indices, and the round starts.
// Staging is pipelined like the solve's: while chunk c's rounds run, the
// a_ij and staged values of chunk c+1 (gathers by the positions loaded a
// chunk earlier; staged producers are two or more chunks back, so their
// stores completed at this chunk's switch) and the records of chunk c+2 are
// in flight. Rounds of <= 64 items run on wave 0 alone, consecutive narrow
// rounds without workgroup barriers (in-order LDS of one wave); wider rounds
// use every thread and an LDS-only barrier.
template <typename T>
__global__ __launch_bounds__(kThinThreads) void ilu0_rounds(IluArgs a, int c0, int c1) {
    constexpr int NTH = kThinThreads, K = rsp::kRndItems, S = rsp::kRndStaged;
    constexpr int IPT = K / NTH, PPT = rsp::kRndPairs / NTH, SPT = S / NTH, RPT = rsp::kRndRounds / NTH;
    static_assert((K & (K - 1)) == 0 && IPT * NTH == K && PPT * NTH == rsp::kRndPairs &&
                      SPT * NTH == S && RPT * NTH == rsp::kRndRounds, "chunk budgets per thread");
    constexpr int kZero = 2 * K + S;
    __shared__ T V[2 * K + S + 1];
    __shared__ int4 litem[K];               // pos, pairs (start | count << 16), divisor index, zr
    __shared__ int lpair[rsp::kRndPairs];   // operand indices l_ik | u_kj << 16
    __shared__ int lrnd[rsp::kRndRounds + 1];
    __shared__ unsigned char lfirst[rsp::kRndRounds + 1];  // round opens a level (rsp::kRndLevelStart)
    __shared__ int lds_rdone;  // multi-wave narrow runs: absolute rounds completed
    const int tid = threadIdx.x, lane = tid & 63;
    T *vals = (T *)a.vals;
    if (tid == 0) {
        V[kZero] = T(0);
        lds_rdone = INT_MIN;  // ordered before any use by the first chunk's barriers
    }
    auto chunk = [&](int c) { return load_chunk(a.rchunks, c); };  // scalar loads
    struct Recs {  // item records and staged positions of a chunk (this thread's share)
        rsp::RndItem it[IPT];
        int q[SPT];
    };
    struct Pre {  // ... its a_ij and staged values, pairs, round starts
        T aij[IPT], sv[SPT];
        int pr[PPT], rs[RPT];
    };
    auto load_recs = [&](const rsp::RndChunk &ch) {
        Recs R;
#pragma unroll
        for (int j = 0; j < IPT; ++j)
            if (ch.i0 + tid + j * NTH < ch.i1) R.it[j] = a.ritems[ch.i0 + tid + j * NTH];
#pragma unroll
        for (int j = 0; j < SPT; ++j)
            if (ch.s0 + tid + j * NTH < ch.s1) R.q[j] = a.rstaged[ch.s0 + tid + j * NTH];
        return R;
    };
    auto load_pre = [&](const rsp::RndChunk &ch, const Recs &R) {
        Pre P;
#pragma unroll
        for (int j = 0; j < IPT; ++j)
            if (ch.i0 + tid + j * NTH < ch.i1) P.aij[j] = vals[R.it[j].pos];
#pragma unroll
        for (int j = 0; j < SPT; ++j)
            if (ch.s0 + tid + j * NTH < ch.s1) P.sv[j] = vals[R.q[j]];
#pragma unroll
        for (int j = 0; j < PPT; ++j)
            if (ch.p0 + tid + j * NTH < ch.p1) P.pr[j] = a.rpairs[ch.p0 + tid + j * NTH];
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (ch.r0 + tid + j * NTH < ch.r1) P.rs[j] = a.rrounds[ch.r0 + tid + j * NTH];
        return P;
    };
    // plan operand class -> LDS index for chunk parity par
    auto idx = [&](int x, int par) { return x < 2 * K ? (((x >= K) ^ par) * K + (x & (K - 1))) : x; };
    auto stage = [&](int c, const rsp::RndChunk &ch, const Recs &R, const Pre &P) {
        const int ni = ch.i1 - ch.i0, ns = ch.s1 - ch.s0, np = ch.p1 - ch.p0, nr = ch.r1 - ch.r0;
        const int par = c & 1, cb = par * K;
        __syncthreads();  // earlier chunks' values stored and visible (workgroup scope); LDS free
#pragma unroll
        for (int j = 0; j < IPT; ++j)
            if (tid + j * NTH < ni) {
                const rsp::RndItem r = R.it[j];
                litem[tid + j * NTH] = make_int4(r.pos, r.u, r.d >= 0 ? idx(r.d, par) : -1, r.zr);
                V[cb + tid + j * NTH] = P.aij[j];
            }
#pragma unroll
        for (int j = 0; j < SPT; ++j)
            if (tid + j * NTH < ns) V[2 * K + tid + j * NTH] = P.sv[j];
#pragma unroll
        for (int j = 0; j < PPT; ++j)
            if (tid + j * NTH < np)
                lpair[tid + j * NTH] = idx(P.pr[j] & 0xffff, par) | idx(P.pr[j] >> 16, par) << 16;
#pragma unroll
        for (int j = 0; j < RPT; ++j)
            if (tid + j * NTH < nr) {
                lrnd[tid + j * NTH] = P.rs[j] & (rsp::kRndLevelStart - 1);
                lfirst[tid + j * NTH] = (P.rs[j] & rsp::kRndLevelStart) != 0;
            }
        if (tid == 0) {
            lrnd[nr] = ni;
            lfirst[nr] = 1;
        }
        lds_barrier();
    };
    // An item: its value in the chunk's LDS slot and (wide rounds, STORE) in
    // vals. Narrow rounds skip the global store and the zero-pivot check: a
    // run's items go to vals in one flush by all threads after the run, so a
    // narrow round is LDS traffic and arithmetic only.
    auto process = [&](int it, int cb, auto store_tag) {
        constexpr bool STORE = decltype(store_tag)::value;
        const int4 r = litem[it];
        T v = V[cb + it];
        const T dv = V[r.z >= 0 ? r.z : kZero];  // the divisor, read with the pair indices
        const int u0 = r.y & 0xffff, u1 = u0 + (r.y >> 16);
        auto batch = [&](int u) {  // operands of 4 pairs loaded together (clamped)
            int pr[4];
            T l[4], w[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) pr[b] = lpair[min(u + b, u1 - 1)];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                l[b] = V[pr[b] & 0xffff];
                w[b] = V[pr[b] >> 16];
            }
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (u + b < u1) v = fma_t(-l[b], w[b], v);
        };
        if (u1 > u0) {  // the first batch straight-line (most items have <= 4 pairs)
            batch(u0);
            for (int u = u0 + 4; u < u1; u += 4) batch(u);
        }
        if (r.z >= 0) v = qdiv<T>(v, dv);
        V[cb + it] = v;
        if constexpr (STORE) {
            vals[r.x] = v;
            if (r.w >= 0 && v == T(0)) atomicMin(a.zero_pivot, r.w);
        }
    };
    auto flush = [&](int cb, int i0, int i1) {  // items [i0, i1) of a narrow run, after its barrier
        for (int i = i0 + tid; i < i1; i += NTH) {
            const int4 r = litem[i];
            const T v = V[cb + i];
            vals[r.x] = v;
            if (r.w >= 0 && v == T(0)) atomicMin(a.zero_pivot, r.w);
        }
    };
    auto narrow = [&](int q) { return lrnd[q + 1] - lrnd[q] <= 64; };
    auto run_end = [&](int q, int nr) {  // first round >= q that is not narrow, or nr
        for (int b = q;; b += 64) {
            const int qq = b + lane;
            const unsigned long long m = __ballot(!(qq < nr && narrow(qq)));
            if (m) return b + __builtin_ctzll(m);
        }
    };
    // Narrow run on KW waves (a.narrow_waves, deferred stores only): the run's
    // rounds are cut into segments at the rounds that open a level (a level's
    // rounds depend on each other through its rows' l_ik: one wave runs a
    // segment in order, its in-order LDS accesses ordering them, as in the
    // one-wave run), and wave w takes segments w, w + KW, ... Before waiting,
    // a wave loads what no value of the run feeds — the first two rounds'
    // item records, initial values a_ij and first four pair indices; then it
    // waits until the segment before its own is complete (an LDS counter of
    // absolute rounds done, published by each segment's wave with a release
    // store after its value stores, lds_publish), and only then reads operands (divisors, l_ik,
    // u_kj) and runs the fma chains and divisions. While one wave is on its
    // chain, the others have prepared their next levels. Same items, same
    // pairs in the same order, same divisions as the one-wave run: same bits.
    struct ItemPre {
        int4 r;
        T v;
        int pr[4];
    };
    auto item_pre = [&](int it, int cb) {
        ItemPre p;
        p.r = litem[it];
        p.v = V[cb + it];
        const int u0 = p.r.y & 0xffff, u1 = u0 + (p.r.y >> 16);
#pragma unroll
        for (int b = 0; b < 4; ++b) p.pr[b] = lpair[min(u0 + b, max(u1 - 1, 0))];
        return p;
    };
    // short: no item of the wave's round has more than two pairs (wave-
    // uniform), so only the first two pairs' operands are read and chained
    auto item_post = [&](int it, int cb, const ItemPre &p, bool short2) {
        const int4 r = p.r;
        T v = p.v;
        const T dv = V[r.z >= 0 ? r.z : kZero];
        const int u0 = r.y & 0xffff, u1 = u0 + (r.y >> 16);
        if (short2) {
            if (u1 > u0) {
                T l[2], w[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    l[b] = V[p.pr[b] & 0xffff];
                    w[b] = V[p.pr[b] >> 16];
                }
                v = fma_t(-l[0], w[0], v);
                if (u1 > u0 + 1) v = fma_t(-l[1], w[1], v);
            }
        } else if (u1 > u0) {
            T l[4], w[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                l[b] = V[p.pr[b] & 0xffff];
                w[b] = V[p.pr[b] >> 16];
            }
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (u0 + b < u1) v = fma_t(-l[b], w[b], v);
            for (int u = u0 + 4; u < u1; u += 4) {  // items of more than four pairs (rare)
                int pr[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) pr[b] = lpair[min(u + b, u1 - 1)];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    l[b] = V[pr[b] & 0xffff];
                    w[b] = V[pr[b] >> 16];
                }
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (u + b < u1) v = fma_t(-l[b], w[b], v);
            }
        }
        if (r.z >= 0) v = qdiv<T>(v, dv);
        V[cb + it] = v;
    };
    auto run_mw = [&](const rsp::RndChunk &ch, int q, int qe, int cb, int KW) {
        const int w = tid >> 6;
        auto seg_end = [&](int s) {  // first round > s that opens a level, or qe (wave-uniform)
            for (int b = s + 1;; b += 64) {
                const int qq = b + lane;
                const unsigned long long m = __ballot(qq >= qe || lfirst[qq]);
                if (m) return min(b + (int)__builtin_ctzll(m), qe);
            }
        };
        int k = 0;
        for (int s0 = q; s0 < qe; ++k) {
            const int s1 = seg_end(s0);
            if (k % KW == w) {
                const int b0 = lrnd[s0], n0 = lrnd[s0 + 1] - b0;
                const bool has1 = s0 + 1 < s1;
                const int b1 = has1 ? lrnd[s0 + 1] : b0, n1 = has1 ? lrnd[s0 + 2] - b1 : 0;
                // (a third round's records too: levels of three rounds are
                // common on the deep circuits, dc1 2.7 rounds per level)
                const bool has2 = s0 + 2 < s1;
                const int b2 = has2 ? lrnd[s0 + 2] : b0, n2 = has2 ? lrnd[s0 + 3] - b2 : 0;
                const ItemPre p0 = item_pre(b0 + min(lane, n0 - 1), cb);
                const ItemPre p1 = item_pre(b1 + min(lane, max(n1 - 1, 0)), cb);
                ItemPre p2{};
                if (has2) p2 = item_pre(b2 + min(lane, max(n2 - 1, 0)), cb);  // (wave-uniform: levels of >= 3 rounds)
                const bool sh2 = !__ballot(lane < n2 && (p2.r.y >> 16) > 2);
                const bool sh0 = !__ballot(lane < n0 && (p0.r.y >> 16) > 2);
                const bool sh1 = !__ballot(lane < n1 && (p1.r.y >> 16) > 2);
                if (s0 > q) lds_wait_geq(&lds_rdone, ch.r0 + s0);
                if (lane < n0) item_post(b0 + lane, cb, p0, sh0);
                wave_sync();
                if (has1) {
                    if (lane < n1) item_post(b1 + lane, cb, p1, sh1);
                    wave_sync();
                    if (has2) {
                        if (lane < n2) item_post(b2 + lane, cb, p2, sh2);
                        wave_sync();
                    }
                    for (int qq = s0 + 3; qq < s1; ++qq) {  // levels of more than three rounds
                        const int bq = lrnd[qq];
                        if (bq + lane < lrnd[qq + 1]) process(bq + lane, cb, std::false_type());
                        wave_sync();
                    }
                }
                lds_publish(&lds_rdone, ch.r0 + s1, lane == 0);  // after the value stores
            }
            s0 = s1;
        }
    };
    auto rounds = [&](int c, const rsp::RndChunk &ch) {
        const int nr = ch.r1 - ch.r0, cb = (c & 1) * K;
        for (int q = 0; q < nr;) {
            if (narrow(q)) {
                const int qe = run_end(q, nr);
                // long runs defer the global stores to one flush after the
                // run; short ones (between wide rounds) store as they go
                const bool defer = qe - q >= a.defer_rounds;
                auto run = [&](auto store_tag) {
                    for (int qq = q; qq < qe; ++qq) {
                        const int b0 = lrnd[qq];
                        if (b0 + lane < lrnd[qq + 1]) process(b0 + lane, cb, store_tag);
                        wave_sync();
                    }
                };
                const int KW = min(a.narrow_waves, NTH / 64);
                if (defer && KW > 1) {
                    if (tid < 64 * KW) run_mw(ch, q, qe, cb, KW);
                } else if (tid < 64) {  // (a software-pipelined form of this loop measured slower)
                    if (defer)
                        run(std::false_type());
                    else
                        run(std::true_type());
                }
                lds_barrier();
                if (defer) flush(cb, lrnd[q], lrnd[qe]);
                q = qe;
                continue;
            }
            for (int it = lrnd[q] + tid; it < lrnd[q + 1]; it += NTH) process(it, cb, std::true_type());
            lds_barrier();
            ++q;
        }
    };
    const int cl = c1 - 1;
    rsp::RndChunk rc = chunk(c0), rn = chunk(min(c0 + 1, cl));
    Recs R = load_recs(rc);
    Pre P = load_pre(rc, R);
    Recs Rn = load_recs(rn);
    auto mark = [&](int c, int j, unsigned long long v) {  // diagnostics only (RSP_ILU_FTRACE)
        if (a.trace && tid == 0 && 4 * c + j < a.trace_cap) a.trace[4 * c + j] = v;
    };
    for (int c = c0; c < c1; ++c) {
        mark(c, 0, clock64());
        stage(c, rc, R, P);
        mark(c, 1, clock64());
        const rsp::RndChunk cur = rc;
        if (c + 1 < c1) {
            const rsp::RndChunk r2 = chunk(min(c + 2, cl));
            P = load_pre(rn, Rn);  // chunk c+1's gathers
            R = Rn;
            Rn = load_recs(r2);    // chunk c+2's records
            rc = rn;
            rn = r2;
        }
        rounds(c, cur);
        mark(c, 2, clock64());
        mark(c, 3, (unsigned long long)(cur.r1 - cur.r0) | (unsigned long long)(cur.i1 - cur.i0) << 32);
    }
}

template <typename T, int B>
static hipError_t launch_factor(const IluArgs &a, hipStream_t s) {
    if (a.fac_one) {
        if (a.n > 0) hipLaunchKernelGGL((ilu0_scale_lower<T>), dim3((a.n + 255) / 256), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    const LevelPlan &P = a.plan;
    int fr = 0;  // next flow run (sorted by level)
    int flow_launched = 0;
    if (a.flow && a.nfruns > 0) {  // the flow rows' upper values become kNotYet (ilu0_flow_prep)
        const int nitems = a.fruns[a.nfruns - 1].c1;
        hipLaunchKernelGGL((ilu0_flow_prep<T>), dim3((nitems + 3) / 4), dim3(256), 0, s, a, nitems);
    }
    for (int g = 0; g < P.nseg; ++g) {
        const rsp::LevelSeg sg = P.segs[g];
        if (sg.thin) {
            hipLaunchKernelGGL((ilu0_rounds<T>), dim3(1), dim3(kThinThreads), 0, s, a, sg.c0, sg.c1);
            continue;
        }
        for (int l = sg.lb; l < sg.le; ++l) {
            while (fr < a.nfruns && a.fruns[fr].lb < l) ++fr;
            if (a.flow && fr < a.nfruns && a.fruns[fr].lb == l) {  // flow run: one persistent launch
                const rsp::FacFlowRun r = a.fruns[fr];
                launch_flow<ilu0_flow<T, true>, ilu0_flow<T, false>>(a, r.c0, r.c1, s);
                ++flow_launched;
                l = r.le - 1;
                continue;
            }
            const int off = P.ptr_host[l], cnt = P.ptr_host[l + 1] - off;
            if (cnt <= 0) continue;
            const rsp::FacSlotLevel *sl = a.fat_slots && a.fslev ? &a.fslev[l] : nullptr;
            if (sl && sl->stride > 0 && sl->rm > 0 && sl->qm > 0) {
                const int *lvl = a.fslots + sl->off;
                auto kern = sl->rm <= 64 ? (sl->qm <= 128 ? ilu0_level_slot<T, 1, 2>
                                                          : sl->qm <= 512 ? ilu0_level_slot<T, 1, 8>
                                                                          : ilu0_level_slot<T, 1, 16>)
                                         : (sl->qm <= 128 ? ilu0_level_slot<T, 4, 2>
                                                          : sl->qm <= 512 ? ilu0_level_slot<T, 4, 8>
                                                                          : ilu0_level_slot<T, 4, 16>);
                hipLaunchKernelGGL(kern, dim3(cnt), dim3(64), 0, s, a, lvl, sl->stride, sl->rm, sl->qm);
            } else if (a.fat_lds)
                hipLaunchKernelGGL((ilu0_level_lds<T, B>), dim3(cnt), dim3(64), 0, s, a, off);
            else
                hipLaunchKernelGGL((ilu0_level<T, B>), dim3((cnt + kIluWaves - 1) / kIluWaves),
                                   dim3(64 * kIluWaves), 0, s, a, off, cnt);
        }
    }
    // ilu0_flow_prep tagged the upper values of EVERY flow run's rows; only the
    // run's own launch restores them. A run the level walk skipped would leave
    // its rows tagged (a corrupt factor reported as success): fail the call.
    if (a.flow && flow_launched != a.nfruns) return hipErrorLaunchFailure;
    return hipGetLastError();
}

// batch width from the plan (2, 4 or 8)
template <typename T>
static hipError_t factor_dispatch(const IluArgs &a, hipStream_t s) {
    switch (a.plan.batch) {
        case 2: return launch_factor<T, 2>(a, s);
        case 4: return launch_factor<T, 4>(a, s);
        default: return launch_factor<T, 8>(a, s);
    }
}

hipError_t ilu0_factor_f32(const IluArgs &a, hipStream_t s) { return factor_dispatch<float>(a, s); }
#ifndef RSP_FTZ_BUILD
// Slot rows of the fat factor levels (analysis, once per pattern). Padding
// is written too: divisor positions -1 and pairs (0, 0), so every value
// index the factor kernel loads from a slot is a valid position.
__global__ __launch_bounds__(64) void ilu0_slot_build(IluArgs a, const int4 *__restrict__ desc,
                                                      const long long *__restrict__ offs,
                                                      int *__restrict__ slots) {
    const int lane = threadIdx.x;
    const int4 d = desc[blockIdx.x];
    int *q = slots + offs[blockIdx.x];
    const int x = d.x, rm = d.y, qm = d.z;
    const int i = a.plan.rows[x], rs = a.rowptr[i], re = a.rowptr[i + 1];
    const int nr = re - rs, nlo = a.dpos[i] - rs;
    const int q0 = a.upd_ptr[rs], nq = a.upd_ptr[re] - q0;
    const bool global = nr > rsp::kFacRow || nq > rsp::kFacPairs;
    if (lane < 8) {
        const int h[8] = {i, rs, nlo, nr, nq, a.hasdiag[i], global ? 1 : 0, 0};
        q[lane] = h[lane];
    }
    for (int y = lane; y < rm; y += 64) {
        const bool in = !global && y < nr, lower = in && y < nlo;
        q[8 + y] = lower ? a.udiv[rs + y] : -1;
        q[8 + rm + y] = in ? ((a.upd_ptr[rs + y] - q0) | ((lower ? a.lord[rs + y] - rs : 0) << 11) |
                              ((lower ? a.lend[rs + y] - rs : 0) << 20))
                           : 0;
    }
    const int pa = rsp::fac_pairs_at(rm);
    for (int u = lane; u < qm; u += 64) {
        const bool in = !global && u < nq;
        q[pa + 2 * u] = in ? a.upd_u[q0 + u] : 0;
        q[pa + 2 * u + 1] = in ? a.upd_l[q0 + u] - rs : 0;
    }
}

hipError_t ilu0_build_slots(const IluArgs &a, const int4 *desc, const long long *offs, int nrows, int *slots,
                            hipStream_t s) {
    if (nrows <= 0) return hipSuccess;
    hipLaunchKernelGGL(ilu0_slot_build, dim3(nrows), dim3(64), 0, s, a, desc, offs, slots);
    return hipGetLastError();
}

hipError_t ilu0_factor_f64(const IluArgs &a, hipStream_t s) { return factor_dispatch<double>(a, s); }
#endif

}  // namespace RSP_KNS
