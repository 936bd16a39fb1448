// ilu_flow.h — the flow scheduler of the persistent launches ilu0_flow
// (ilu0.hip) and trsv_flow (trsv.hip): the data-tagged hand-off words, the
// walk of a launch's work items (FlowClaims: static, claimed, start tickets
// with steals), the bounded waits, and the host side of a flow launch.
// Compiled in the including unit's kernel namespace (rsp_k / rsp_k_ftz).
#pragma once

#include "ilu_device.h"

namespace RSP_KNS {

// Words handed between workgroups of one persistent launch (trsv_flow,
// ilu0_flow): written once by a 4- / 8-byte device-scope (sc1) store, read by
// device-scope (sc1) loads, which bypass the reader's L1 — MI355X_MICROARCH.md
// (inter-workgroup visibility; price list, handoff-1to1 / handoff-flag).
template <typename T>
struct FlowWord;
template <>
struct FlowWord<double> {
    typedef unsigned long long U;
    static constexpr U kNotYet = 0x7ff5eed15eed1001ull;
};
template <>
struct FlowWord<float> {
    typedef unsigned int U;
    static constexpr U kNotYet = 0x7fa5eed1u;
};
// A flow wait gives up after fc.ticks of the 100 MHz wall clock (default
// 0.2 s, RSP_ILU_FLOW_TIMEOUT_US) and records the call's generation in
// *fc.status (rsp::FlowCtl).
__device__ __forceinline__ void flow_give_up(const rsp::FlowCtl &fc) {
    if ((threadIdx.x & 63) == 0) __hip_atomic_store(fc.status, fc.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Work-item claims of a flow launch (rsp::FlowCtl): lane 0 takes the next
// item with an agent-scope fetch_add, issued one item ahead (its return is
// read at the top of the next item, so the atomic's latency overlaps the
// current item); flow_item() turns the claim into the item index.
__device__ __forceinline__ unsigned long long flow_claim(const rsp::FlowCtl &fc) {
    return (threadIdx.x & 63) == 0
               ? __hip_atomic_fetch_add(fc.claim, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
               : 0ull;
}
__device__ __forceinline__ int flow_item(unsigned long long c, unsigned long long base, int it0, int it1) {
    // the difference fits an int (claims of this launch); lane 0's is the one
    const long long d = (long long)(c - base);
    return __builtin_amdgcn_readfirstlane((int)min(d, (long long)(it1 - it0))) + it0;
}

// One wave's walk over the items [it0, it1) of a flow launch (rsp::FlowCtl):
//   for (fq.first(); fq.more(); fq.next()) { const int it = fq.item(); ... }
// A wait inside an item that returns true (fq.expire(), tickets only) makes
// the item yield: it runs through on what it has but stores nothing, and
// fq.item_end(it, true) has next() run it again or walk a grown ticket list.
// Static (RSP_ILU_FLOW_MODE=0): w, w + W, ... (the whole grid must be resident).
// Claimed (kFlowClaims): in start order, TWO items ahead — the claim for item
// j + 2 is issued during item j, behind its first loads (claim_ahead), and
// read when item j + 1 ends, so the atomic's latency hides under a whole
// item. A wave makes 2 + (items it processes) claims, so a launch advances
// the counter by exactly items + 2 W (flow_claims on the host). The lowest
// unfinished item is always some running wave's CURRENT item (a wave's
// claimed items are above its current one), so progress needs no
// co-residency.
// Start tickets (kFlowTickets, the default): thread 0 takes the workgroup's
// ticket t — from one of eight counters (blockIdx % 8; counter q hands out
// q, q + 8, ..., so the G start claims do not queue on one address) of the
// launch's counter slot (base & 1; block 0 zeroes the other slot for the
// next launch, the previous launch's, which has ended) — and each wave walks
// the static items of t, it0 + 4 t + wave + k W: a resident grid runs
// exactly the static walk. A workgroup whose counter is spent owns nothing.
// Steals: a wait past kFlowStealUs (2 us once its workgroup has stolen)
// asks expire(): with every counter spent and the owned list unchanged
// (calm) it waits on; else the item yields — it runs through on what it
// has, stores nothing — and next() claims another ticket for the workgroup
// (under an LDS lock, inserted so that own[] stays ascending) unless none
// is left, then runs the item again — unless the list has grown (by this
// steal or another wave's): then the wave walks again from the start:
// rounds k = 0, 1, ..., in each the owned tickets in list order — the
// merged index order of its items — skipping the items it has finished
// (those of the start ticket below the round it had reached, and those
// marked with the call's epoch in fc.done since).
// A wave out of items waits in the workgroup until all four are (the list
// could still grow), counted with the list length in one LDS word.
// Progress: let u be the lowest unfinished item. If its ticket is owned,
// its owner's wave for u has walked every owned item below u (finished) and
// is at u, or waits on a higher item or for its siblings and sees the list
// grow once u's ticket joined it: it comes to u, whose operands are lower
// items, finished. If u's ticket is unclaimed, every started wave that
// cannot go on waits, and either steals (a ticket is claimed) or its
// workgroup ends (a new one starts and claims). Every wait is bounded by
// fc.ticks; nothing needs co-residency.
struct FlowTicketLds {
    int own[rsp::kFlowOwnMax];  // the workgroup's tickets, ascending (own[0] the start ticket until a steal)
    int state;                  // tickets owned | waves out of items << 16
    int lock;                   // a steal is in progress
    int dry;                    // every counter is spent: no ticket left to steal
};
template <bool TK>  // TK: start tickets (kFlowTickets); else static or claimed (fc.mode)
struct FlowClaims {
    const rsp::FlowCtl &fc;
    unsigned long long base, c1 = 0, c2 = 0;
    int it0, it1, cur, stride, wv;
    int mode;  // 0 static, 1 claims, 2 tickets (TK)
    FlowTicketLds *L;
    // tickets: the owned list as this wave last read it, its position
    // (round k, list index j), the round its fast walk reached (start ticket
    // items below it are finished), whether it walks with done checks
    int nseen = 0, k = 0, j = 0, fast_k = 0, t0 = 0;
    // a wait this long (100 MHz ticks) may steal: kFlowStealUs, 2 us after a steal
    unsigned long long steal_at = 100ull * rsp::kFlowStealUs;
    bool scan = false, redo = false, over = false;
    __device__ FlowClaims(const rsp::FlowCtl &f, unsigned long long b, int i0, int i1, int w, int W,
                          FlowTicketLds *l)
        : fc(f), base(b), it0(i0), it1(i1), cur(i0 + w), stride(W), wv(w & 3),
          mode(TK ? 2 : (f.mode & rsp::kFlowClaims) ? 1 : 0), L(l) {}
    // tickets: counter q of this launch's slot hands out q, q + 8, q + 16, ...
    // (eight counters, so the G start claims do not queue on one address)
    __device__ unsigned *ctr() const { return fc.tickets + rsp::kFlowTicketCtrs * (int)(base & 1); }
    __device__ int take(int q) const {
        return q + rsp::kFlowTicketCtrs * (int)__hip_atomic_fetch_add(ctr() + q, 1u, __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ bool spent(int q) const {  // counter q has no ticket < G left
        return q + rsp::kFlowTicketCtrs * (long long)__hip_atomic_load(ctr() + q, __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT) >= (long long)gridDim.x;
    }
    __device__ static int lds_ld(const int *p) {
        return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    }
    // LDS-only acquire (the "local" address-space fence): a workgroup-scope
    // acquire on a plain atomic would also wait for the wave's outstanding
    // GLOBAL accesses (s_waitcnt vmcnt(0))
    __device__ static int lds_acq(const int *p) {
        const int v = lds_ld(p);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        return v;
    }
    __device__ void first() {
        if constexpr (!TK) {
            if (mode == 1) {
                const unsigned long long c0 = flow_claim(fc);
                c1 = flow_claim(fc);
                cur = flow_item(c0, base, it0, it1);
            }
            return;
        }
        if (threadIdx.x == 0) {
            if (blockIdx.x == 0)  // the next launch's slot (the previous launch's: it has ended)
                for (int q = 0; q < rsp::kFlowTicketCtrs; ++q)
                    __hip_atomic_store(fc.tickets + rsp::kFlowTicketCtrs * (int)((base + 1) & 1) + q, 0u,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int t = take(blockIdx.x % rsp::kFlowTicketCtrs);
            L->own[0] = t;
            L->state = t < (int)gridDim.x ? 1 : 0;
            L->lock = 0;
            L->dry = t >= (int)gridDim.x;
        }
        __syncthreads();  // (once, at the start)
        nseen = lds_ld(&L->state) & 0xffff;
        t0 = lds_ld(&L->own[0]);
        settle();
    }
    __device__ bool more() const { return TK ? !over : cur < it1; }
    __device__ int item() const { return cur; }
    __device__ void claim_ahead() {
        __builtin_amdgcn_sched_barrier(0);
        if (mode == 1) c2 = flow_claim(fc);
        __builtin_amdgcn_sched_barrier(0);
    }
    // tickets: from position (k, j), the next item of this wave to run
    // (cur), or none left in the workgroup (over)
    __device__ void settle() {
        if (!scan && nseen == 1) {  // the start ticket alone: the static walk
            const int it = it0 + 4 * t0 + wv + k * stride;
            if (it < it1) {
                cur = it;
                return;
            }
        }
        for (;;) {
            if (j >= nseen && nseen > 0) {
                ++k;
                j = 0;
            }
            if (nseen > 0) {
                const int tj = lds_ld(&L->own[j]);
                const int it = it0 + 4 * tj + wv + k * stride;
                if (it < it1) {
                    const bool fin = scan && ((tj == t0 && k < fast_k) ||
                                              __hip_atomic_load(fc.done + it, __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_WAVEFRONT) == (int)fc.epoch);
                    if (!fin) {
                        cur = it;
                        return;
                    }
                    ++j;
                    continue;
                }
                if (j > 0) {  // the rest of round k is past it1 too
                    ++k;
                    j = 0;
                    continue;
                }
            }
            const int s = idle();  // out of items
            if (s < 0) {
                over = true;
                cur = it1;
                return;
            }
            rescan(s);
        }
    }
    // walk again from the start over an owned list of s tickets
    __device__ void rescan(int s) {
        if (!scan) fast_k = k;  // (the fast walk was at round k of the start ticket)
        scan = true;
        steal_at = 200;
        nseen = s;
        k = j = 0;
    }
    // out of items: wait until the owned list grows (its new length) or all
    // four waves are out (-1)
    __device__ int idle() {
        const int me = __builtin_amdgcn_readfirstlane((int)(threadIdx.x & 63));
        int r = -1;
        if ((int)(threadIdx.x & 63) == me) {
            int s = __hip_atomic_fetch_add(&L->state, 1 << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) +
                    (1 << 16);
            for (;;) {
                if ((s & 0xffff) != nseen) {
                    __hip_atomic_fetch_add(&L->state, -(1 << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    r = s & 0xffff;
                    break;
                }
                if ((s >> 16) == 4) break;
                __builtin_amdgcn_s_sleep(2);
                s = __hip_atomic_load(&L->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        r = __builtin_amdgcn_readfirstlane(r);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");  // own[] entries up to r
        return r;
    }
    // a wait that began at wall clock t0 runs until this deadline, then
    // expire() tells it to give up or (tickets) to yield the item to next(),
    // which may steal, then runs the item again or walks a grown list; the
    // give-up bound counts from the wait's start (one compare per poll, as
    // without tickets; nothing written, so a wait of one lane is fine). An
    // item yields only while a steal can follow (not calm), fewer than G + 1
    // times per wave, so no item escapes the bound by yielding.
    __device__ unsigned long long deadline(unsigned long long t0) const {
        if constexpr (!TK) return t0 + fc.ticks;
        return t0 + min(fc.ticks, steal_at);
    }
    // a wait past its deadline: 0 give up, 1 yield, 2 wait on until the new
    // deadline dl (tickets: nothing to steal and the owned list as this wave
    // knows it — every ticket is claimed, a grown list would have had a
    // steal succeed first)
    __device__ int expire(unsigned long long now, unsigned long long t0, unsigned long long &dl) const {
        if (TK && now <= t0 + fc.ticks) {
            if (!calm()) return 1;
            dl = t0 + fc.ticks;
            return 2;
        }
        flow_give_up(fc);
        return 0;
    }
    // tickets: no steal can succeed (LDS dry, set here once the counter
    // shows all G tickets claimed) and the owned list has not grown past nseen
    __device__ bool calm() const {
        if constexpr (!TK) return true;
        if (!__hip_atomic_load(&L->dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
            for (int q = 0; q < rsp::kFlowTicketCtrs; ++q)
                if (!spent(q)) return false;
            __hip_atomic_store(&L->dry, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return (__hip_atomic_load(&L->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & 0xffff) == nseen;
    }
    // next() after a yield: the owned list's length if it has grown past
    // nseen (maybe by a steal made here), else 0
    __device__ int steal() {
        const int me = __builtin_amdgcn_readfirstlane((int)(threadIdx.x & 63));
        int r = 0;
        if ((int)(threadIdx.x & 63) == me) {
            const int s = __hip_atomic_load(&L->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if ((s & 0xffff) != nseen)
                r = s & 0xffff;
            else if (!__hip_atomic_load(&L->dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                int z = 0;
                if (__hip_atomic_compare_exchange_strong(&L->lock, &z, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_WORKGROUP)) {
                    const int n = __hip_atomic_load(&L->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) &
                                  0xffff;
                    if (n != nseen)
                        r = n;
                    else if (n < rsp::kFlowOwnMax) {
                        int t = (int)gridDim.x;
                        for (int d = 0; d < rsp::kFlowTicketCtrs && t >= (int)gridDim.x; ++d) {
                            const int q = (int)(blockIdx.x + d) % rsp::kFlowTicketCtrs;
                            if (!spent(q)) t = take(q);
                        }
                        if (t < (int)gridDim.x) {  // insert, keeping own[] ascending
                            int x = n;
                            for (; x > 0 && L->own[x - 1] > t; --x) L->own[x] = L->own[x - 1];
                            L->own[x] = t;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                            __hip_atomic_fetch_add(&L->state, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            r = n + 1;
                        } else
                            __hip_atomic_store(&L->dry, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    __hip_atomic_store(&L->lock, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        r = __builtin_amdgcn_readfirstlane(r);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");  // own[] entries up to r
        return r;
    }
    // the item is finished: after a steal its index is marked with the epoch
    __device__ void done(int it) const {
        if (TK && scan && (threadIdx.x & 63) == 0)
            __hip_atomic_store(fc.done + it, (int)fc.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    // the item ends: finished, or (yl) yielded — then next() runs it again
    // unless the owned list grows
    __device__ void item_end(int it, bool yl) {
        if constexpr (!TK) return;
        if (yl)
            redo = true;
        else
            done(it);
    }
    __device__ void next() {
        if constexpr (!TK) {
            if (mode == 0) {
                cur += stride;
            } else {
                cur = flow_item(c1, base, it0, it1);
                c1 = c2;
            }
            return;
        }
        if (__builtin_expect(!redo && !scan && nseen == 1, 1)) {  // the static walk of the start ticket
            cur += stride;
            ++k;
            if (cur < it1) return;
        } else if (redo) {  // the item yielded: it runs again unless the owned list grows
            redo = false;
            const int n = steal();
            if (n == 0) return;
            rescan(n);
        } else
            ++j;
        settle();
    }
};

template <typename T>
__device__ __forceinline__ typename FlowWord<T>::U flow_load(const T *p) {
    return __hip_atomic_load((typename FlowWord<T>::U *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void flow_store(T *p, T v) {
    typedef typename FlowWord<T>::U U;
    __hip_atomic_store((U *)p, __builtin_bit_cast(U, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Re-read this lane's operand words [0, n) that are still kNotYet until none
// of the wave's is (wave-uniform loop; the pause between polls doubles up to
// max_sleep s_sleep units of 64 clocks). True: the item yields (FlowClaims::expire).
template <typename T, int NB, typename FQ>
__device__ __forceinline__ bool flow_wait(typename FlowWord<T>::U (&w)[NB], const int (&id)[NB], int n,
                                          const T *y, FQ &fq, int max_sleep, bool skip = false) {
    constexpr auto kNot = FlowWord<T>::kNotYet;
    auto pending = [&] {
        bool p = false;
#pragma unroll
        for (int b = 0; b < NB; ++b) p |= b < n && w[b] == kNot;
        return p;
    };
    if (!__ballot(pending())) return false;
    const unsigned long long t0 = wall_clock64();
    unsigned long long dl = skip ? 0ull : fq.deadline(t0);  // (skip: the item has yielded)
    for (int sl = 1;; sl = min(2 * sl, max_sleep)) {
        for (int q = 0; q < sl; ++q) __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b < n && w[b] == kNot) w[b] = flow_load(y + id[b]);
        if (!__ballot(pending())) return false;
        const unsigned long long now = wall_clock64();
        if (now > dl) {
            const int r = fq.expire(now, t0, dl);
            if (r != 2) return r != 0;
        }
    }
}

// An item's gate: before polling its own operands, a wave waits (one lane,
// one word) for the y of the last row of the level three below its own (plan:
// RSP_ILU_FLOW_GATE; 2 and 1 measured slower) — only
// a throttle, so that waves whose items are far ahead of the progress front
// poll one word instead of a word per operand (the operand polls alone, up to
// 8 per lane, slowed the loads on the critical path). Row g's item has a
// lower index, so the gate cannot deadlock.
template <typename T, typename FQ>
__device__ __forceinline__ bool flow_gate(int g, const T *y, FQ &fq, int max_sleep) {
    if (g < 0) return false;
    typename FlowWord<T>::U w[1] = {0};
    int id[1] = {g};
    if ((threadIdx.x & 63) == 0) w[0] = flow_load(y + g);
    return flow_wait<T, 1>(w, id, (threadIdx.x & 63) == 0 ? 1 : 0, y, fq, max_sleep);
}

// The same wait over the words a need[] mask selects (ilu0_flow's operands in
// vals). Its own copy of the loop: one wait taking the predicate as a
// parameter changed the flow kernels' machine code (profiles/r08_ilu_split_isa.txt).
template <typename T, int NB, typename FQ>
__device__ __forceinline__ bool tagged_wait(typename FlowWord<T>::U (&w)[NB], const int (&pos)[NB],
                                            const bool (&need)[NB], const T *vals, FQ &fq,
                                            int max_sleep, bool skip) {
    constexpr auto kNot = FlowWord<T>::kNotYet;
    auto pending = [&] {
        bool p = false;
#pragma unroll
        for (int b = 0; b < NB; ++b) p |= need[b] && w[b] == kNot;
        return p;
    };
    if (!__ballot(pending())) return false;
    const unsigned long long t0 = wall_clock64();
    unsigned long long dl = skip ? 0ull : fq.deadline(t0);  // (skip: the item has yielded)
    for (int sl = 1;; sl = min(2 * sl, max_sleep)) {
        for (int q = 0; q < sl; ++q) __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (need[b] && w[b] == kNot) w[b] = flow_load(vals + pos[b]);
        if (!__ballot(pending())) return false;
        const unsigned long long now = wall_clock64();
        if (now > dl) {
            const int r = fq.expire(now, t0, dl);
            if (r != 2) return r != 0;
        }
    }
}

// A finished factor value as it is published: a value whose bits are the
// kNotYet pattern (only an untouched input can be: arithmetic never makes a
// signalling NaN) is published as the quiet NaN of the same payload.
template <typename T>
__device__ __forceinline__ T flow_publishable(T v) {
    typedef typename FlowWord<T>::U U;
    constexpr U kQuiet = sizeof(T) == 8 ? (U)0x0008000000000000ull : (U)0x00400000u;
    const U b = __builtin_bit_cast(U, v);
    return b == FlowWord<T>::kNotYet ? __builtin_bit_cast(T, (U)(b | kQuiet)) : v;
}

// Workgroups of a flow launch: with static items every one must be resident
// at once (rsp::FlowCtl): the occupancy query, less one workgroup per CU of
// margin (it can overstate by one, MI355X_MICROARCH.md residency notes),
// caps the requested grid.
template <auto KERNEL>
static int flow_grid(const rsp::FlowCtl &fc, int want, int cus, int items) {
    static int occ = 0;  // per kernel
    if (occ == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, KERNEL, 256, 0) != hipSuccess) nb = 1;
        occ = max(nb - 1, 1);
    }
    // (start tickets need no residency: the same grid keeps the walk of the
    // static one; tests oversubscribe it, RSP_ILU_FLOW_GRID_X, so that
    // workgroups wait for others to end and steals carry the launch)
    const int g = min(want, cus * occ) * ((fc.mode & rsp::kFlowTickets) ? fc.grid_x : 1);
    return max(1, min(min(g, rsp::kFlowOwnMax), (items + 3) / 4));
}

// A flow launch of `items` items on `grid` 4-wave workgroups: its claim base,
// and the host mirror advanced by the claims it will make (rsp::FlowCtl).
static unsigned long long flow_claims(const rsp::FlowCtl &fc, int items, int grid) {
    const unsigned long long base = *fc.claim_host;
    if (fc.mode & rsp::kFlowTickets) return (*fc.tk_seq)++;  // the launch's counter slot (FlowClaims)
    if (!(fc.mode & rsp::kFlowClaims)) return base;  // static items: no claims
    *fc.claim_host = base + (unsigned long long)items + 2ull * 4ull * (unsigned long long)grid;
    return base;
}

// One flow launch over the items [it0, it1) of a (IluArgs / TrsvArgs): the
// kernel's start-ticket instantiation K_TK or its static / claimed one K_NO
// (a.fc.mode), on the grid of that instantiation's occupancy.
template <auto K_TK, auto K_NO, typename A>
static void launch_flow(const A &a, int it0, int it1, hipStream_t s) {
    const bool tk = a.fc.mode & rsp::kFlowTickets;
    const int grid = tk ? flow_grid<K_TK>(a.fc, a.flow_grid, a.flow_cus, it1 - it0)
                        : flow_grid<K_NO>(a.fc, a.flow_grid, a.flow_cus, it1 - it0);
    const unsigned long long base = flow_claims(a.fc, it1 - it0, grid);
    hipLaunchKernelGGL(tk ? K_TK : K_NO, dim3(grid), dim3(256), 0, s, a, it0, it1, base);
}

}  // namespace RSP_KNS
