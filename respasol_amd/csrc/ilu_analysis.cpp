// ilu_analysis.cpp — host half of the ILU(0) analysis (see ilu_analysis.h).
// Replaces the dependency analysis inside cusparse?csrilu02_analysis and
// cusparse?csrsv2_analysis (GPU/ilu0.cu:196-252). No HIP calls here.

#include "ilu_analysis.h"

#include <limits.h>
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <mutex>

namespace rsp_an {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

void Phases::start() {
    t_last = now_ms();
    next = 0;
}

void Phases::mark(const char *what) {
    const double t = now_ms();
    if (print) fprintf(stderr, "rsp_ilu0_analysis n=%d %-14s %8.2f ms\n", n, what, t - t_last);
    if (ms && next < kPhases) ms[next] = t - t_last;
    next++;
    t_last = t;
}

// rows grouped by level (stable: ascending row within a level). A counting
// sort; on large level sets with few levels per row block, in parallel: each
// of T contiguous row blocks counts its levels, block t's rows of level v go
// after those of blocks < t (the same order as the sequential pass).
void group_levels(const hvec<int> &lev, int nlev, hvec<int> &ptr, hvec<int> &rows) {
    const int n = (int)lev.size();
    const int T = host_threads();
    ptr.assign((size_t)nlev + 1, 0);
    rows.resize(lev.size());
    if (n < (1 << 16) || T < 2 || (long long)nlev * T > n) {
        for (int v : lev) ptr[(size_t)v + 1]++;
        for (int l = 0; l < nlev; l++) ptr[(size_t)l + 1] += ptr[(size_t)l];
        hvec<int> fill(ptr.begin(), ptr.end() - 1);
        for (size_t i = 0; i < lev.size(); i++) rows[(size_t)fill[(size_t)lev[i]]++] = (int)i;
        return;
    }
    std::vector<int> cnt((size_t)T * nlev, 0);  // cnt[t * nlev + v]
    auto block = [&](int t, int &a, int &b) {
        a = (int)((long long)n * t / T);
        b = (int)((long long)n * (t + 1) / T);
    };
    pfor_dyn(T, n, 1, [&](int t) {
        int a, b;
        block(t, a, b);
        int *c = cnt.data() + (size_t)t * nlev;
        for (int i = a; i < b; i++) c[lev[(size_t)i]]++;
    });
    // per level: its start, then each block's offset within it (level-major)
    int run = 0;
    for (int v = 0; v < nlev; v++) {
        ptr[(size_t)v] = run;
        for (int t = 0; t < T; t++) {
            const int k = cnt[(size_t)t * nlev + v];
            cnt[(size_t)t * nlev + v] = run;
            run += k;
        }
    }
    ptr[(size_t)nlev] = run;
    pfor_dyn(T, n, 1, [&](int t) {
        int a, b;
        block(t, a, b);
        int *c = cnt.data() + (size_t)t * nlev;
        for (int i = a; i < b; i++) rows[(size_t)c[lev[(size_t)i]]++] = i;
    });
}

void timed_plan(int n, const char *what, const std::function<void()> &fn) {
    const double t0 = now_ms();
    fn();
    if (env_int("RSP_ILU_TIMING", 0) >= 2)  // diagnostics: per-plan wall time
        fprintf(stderr, "rsp_ilu0_analysis n=%d   plan %-10s %8.2f ms\n", n, what, now_ms() - t0);
}

// Symbolic ILU(0): the update list of every position (see IluArgs) and the
// intra-row stages of the lower positions. Row i is scattered into a dense
// column -> position map, then each lower k (ascending) walks row k's upper
// part; a hit at column j appends (pos l_ik, pos u_kj) to position (i, j).
// One row of it, the only implementation on the host (plan_symbolic: every
// row; symbolic_rows: the device analysis' long rows). `map` (n entries) is
// all -1 on entry and on return. cnt != nullptr: the update-list counts of the
// row's positions; else the pairs at ptr, the stages, the stage order (lower
// positions by (stage, column)) and the divisor positions.
static void symbolic_row(int i, std::vector<int> &map, std::vector<int> &cur, std::vector<int> &order,
                         const int *rp, const int *ci, const int *dpos, const int *hasdiag, int *cnt,
                         const int *ptr, int *upd_l, int *upd_u, int *stage, int *lord, int *lend, int *udiv) {
    const int rs = rp[i], re = rp[i + 1], di = dpos[i];
    for (int p = rs; p < re; p++) map[(size_t)ci[p]] = p;
    if (cnt) {
        for (int p = rs; p < re; p++) cnt[p] = 0;
    } else {
        cur.assign(ptr + rs, ptr + re);
        for (int p = rs; p < re; p++) stage[p] = 0;
    }
    for (int p = rs; p < di; p++) {
        const int k = ci[p];
        for (int q = dpos[k] + hasdiag[k]; q < rp[k + 1]; q++) {
            const int t = map[(size_t)ci[q]];
            if (t > p) {
                if (cnt) {
                    cnt[t]++;
                } else {
                    const int u = cur[(size_t)(t - rs)]++;
                    upd_l[u] = p;
                    upd_u[u] = q;
                    if (t < di) stage[t] = std::max(stage[t], stage[p] + 1);
                }
            }
        }
    }
    for (int p = rs; p < re; p++) map[(size_t)ci[p]] = -1;
    if (cnt) return;
    order.resize((size_t)(di - rs));
    for (int p = rs; p < di; p++) order[(size_t)(p - rs)] = p;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return stage[a] < stage[b]; });
    for (int x = 0; x < di - rs; x++) lord[rs + x] = order[(size_t)x];
    for (int x = di - rs - 1; x >= 0; x--) {
        const bool last = x == di - rs - 1 || stage[order[(size_t)x]] != stage[order[(size_t)x + 1]];
        lend[rs + x] = last ? rs + x + 1 : lend[rs + x + 1];
    }
    for (int p = di; p < re; p++) lord[p] = lend[p] = 0;
    for (int p = rs; p < re; p++) {
        const int k = ci[p];
        udiv[p] = (p < di && hasdiag[k]) ? dpos[k] : -1;
    }
}

// The symbolic factor of a few given rows on the host (the device analysis
// leaves its long rows here: a hub row's lower positions form a long serial
// chain that one GPU lane walks at global-memory latency, where the host
// walks it in cache). cnt as for symbolic_row.
void symbolic_rows(const hvec<int> &rows, int n, const int *rp, const int *ci, const int *dpos,
                   const int *hasdiag, int *cnt, const int *ptr, int *upd_l, int *upd_u, int *stage, int *lord,
                   int *lend, int *udiv) {
    if (rows.empty()) return;
    // rows in parallel (each writes only its own positions and update-list
    // slots; round 5: the hub rows were one sequential pass, ~1-1.7 ms per
    // circuit, twice), in blocks of rows: a block has ONE column map of n
    // entries, reset after each row at the row's own columns only, so the
    // pass stays O(nnz of the rows' DAG) plus O(n) per block (a map per row
    // cost O(n) per long row: quadratic on patterns with many long rows)
    const int nr = (int)rows.size();
    const int nblk = std::max(1, std::min(nr, 2 * host_threads()));
    pfor_dyn(nblk, (long long)nr << 14, 1 << 14, [&](int b) {
        std::vector<int> map((size_t)n, -1), cur, order;
        for (int ri = (int)((long long)nr * b / nblk); ri < (int)((long long)nr * (b + 1) / nblk); ri++)
            symbolic_row(rows[(size_t)ri], map, cur, order, rp, ci, dpos, hasdiag, cnt, ptr, upd_l, upd_u, stage,
                         lord, lend, udiv);
    });
}

rsp_status_t plan_validate(int n, const int *rpp, const int *cip, IluHostPlan &hp) {
    hp = IluHostPlan();
    hp.n = n;
    if (n < 0 || (n > 0 && !rpp)) return RSP_STATUS_INVALID_VALUE;
    if (n > 0 && rpp[0] != 0) return RSP_STATUS_INVALID_VALUE;
    for (int i = 0; i < n; i++)
        if (rpp[i + 1] < rpp[i]) return RSP_STATUS_INVALID_VALUE;
    const int nnz_s = n > 0 ? rpp[n] : 0;
    if (nnz_s > 0 && !cip) return RSP_STATUS_INVALID_VALUE;
    hp.nnz_s = nnz_s;
    const int *rp = rpp, *ci = cip;
    // columns in range, and each row strictly increasing (the reference loader
    // sorts rows, loadMatrixMarket.cpp:237-242; csrilu02 requires sorted,
    // duplicate-free rows): otherwise INVALID_VALUE, never a wrong factor
    bool bad = false;
    {
        std::mutex mu;
        parallel_rows(n, [&](int r0, int r1) {
            bool b = false;
            for (int i = r0; i < r1 && !b; i++)
                for (int p = rp[i]; p < rp[i + 1]; p++) {
                    const int c = ci[p];
                    if (c < 0 || c >= n || (p > rp[i] && c <= ci[p - 1])) {
                        b = true;
                        break;
                    }
                }
            if (b) {
                std::lock_guard<std::mutex> g(mu);
                bad = true;
            }
        });
    }
    if (bad) return RSP_STATUS_INVALID_VALUE;
    hvec<int> &dpos = hp.dpos, &hasdiag = hp.hasdiag;
    dpos.assign((size_t)n, 0);
    hasdiag.assign((size_t)n, 0);
    parallel_rows(n, [&](int r0, int r1) {
        for (int i = r0; i < r1; i++) {
            const int *b = ci + rp[i], *e = ci + rp[i + 1];
            const int *p = std::lower_bound(b, e, i);
            dpos[(size_t)i] = (int)(p - ci);
            hasdiag[(size_t)i] = (p != e && *p == i) ? 1 : 0;
        }
    });
    for (int i = 0; i < n; i++)  // the first missing diagonal (cusparseXcsrilu02_zeroPivot)
        if (!hasdiag[(size_t)i]) {
            hp.structural_zero = i;
            break;
        }
    return RSP_STATUS_SUCCESS;
}

// The split term order of both solve DAGs (IluHostPlan::lpos): per row, its
// early terms, then its late ones (producer one level below the row's), each
// part in the reference's order; a stable partition per row, rows in
// parallel. (The oracle restates it: rsp_oracle.c ORACLE_TRSV_SPLIT.)
static void split_terms(const int *rp, const int *ci, IluHostPlan &hp) {
    const int n = hp.n;
    const hvec<int> &dpos = hp.dpos, &lv = hp.lev_l, &lvt = hp.lev_lt;
    if (!hp.split) {  // the reference's order: every term "late", none moved. Left
        // empty (identity order, no early terms: the consumers treat an empty
        // lpos / ne as that) instead of materialised: the fill was 1-4 ms of
        // the level phase on the 1 M-row patterns (round 5)
        hp.lpos.clear();
        hp.ne_l.clear();
        hp.ne_lt.clear();
        return;
    }
    hp.lpos.assign((size_t)std::max(hp.nnz_s, 1), 0);
    hp.ne_l.assign((size_t)std::max(n, 1), 0);
    hp.ne_lt.assign((size_t)std::max(n, 1), 0);
    parallel_rows(n, [&](int r0, int r1) {
        hvec<int> late, late_c;
        for (int i = r0; i < r1; i++) {
            // L: row i reads y_j, j = ci[p] < i
            int k = rp[i];
            late.clear();
            for (int p = rp[i]; p < dpos[(size_t)i]; p++) {
                if (lv[(size_t)ci[p]] == lv[(size_t)i] - 1)
                    late.push_back(p);
                else
                    hp.lpos[(size_t)k++] = p;
            }
            hp.ne_l[(size_t)i] = k - rp[i];
            for (int p : late) hp.lpos[(size_t)k++] = p;
            // L^T: row i reads y_j, j = ltc[q] > i, q in [ltp[i], ltp[i+1])
            const int q0 = hp.ltp[(size_t)i], q1 = hp.ltp[(size_t)i + 1];
            late.clear();
            late_c.clear();
            int w = q0;
            for (int q = q0; q < q1; q++) {
                const int j = hp.ltc[(size_t)q], tp = hp.lts[(size_t)q];
                if (lvt[(size_t)j] == lvt[(size_t)i] - 1) {
                    late.push_back(tp);
                    late_c.push_back(j);
                } else {
                    hp.lts[(size_t)w] = tp;
                    hp.ltc[(size_t)w++] = j;
                }
            }
            hp.ne_lt[(size_t)i] = w - q0;
            for (size_t u = 0; u < late.size(); u++) {
                hp.lts[(size_t)w] = late[u];
                hp.ltc[(size_t)w++] = late_c[u];
            }
        }
    });
}

// The lower DAG's levels (factor + L solve): the longest path ending at each
// row (each row needs its producers'). rsp_ilu0_analysis waits for these only.
void plan_levels_lower(const int *rp, const int *ci, IluHostPlan &hp) {
    const int n = hp.n;
    const hvec<int> &dpos = hp.dpos;
    const double t0 = now_ms();
    hvec<int> &lv = hp.lev_l;
    lv.assign((size_t)n, 0);
    int nl = n > 0 ? 1 : 0;
    for (int i = 0; i < n; i++) {
        int l = 0;
        for (int p = rp[i]; p < dpos[(size_t)i]; p++) l = std::max(l, lv[(size_t)ci[p]] + 1);
        lv[(size_t)i] = l;
        nl = std::max(nl, l + 1);
    }
    group_levels(lv, nl, hp.L.ptr, hp.L.rows);
    if (env_int("RSP_ILU_TIMING", 0) >= 3)
        fprintf(stderr, "rsp_ilu0_analysis n=%d     levels: L %.2f ms\n", n, now_ms() - t0);
}

// The solves-only half of the level analysis: the L^T DAG's levels and the
// transposed strict lower part (two independent passes, run concurrently:
// each is memory-latency bound), then the split term order. Round 6: started
// by the solve plans' thread, so the analysis proper (the reference's
// csrilu02_analysis) no longer waits for it. The split order reads the L
// levels too: with split = false it is left to the caller (plan_levels).
void plan_levels_upper(const int *rp, const int *ci, IluHostPlan &hp, bool split) {
    const int n = hp.n;
    hp.split = env_int("RSP_ILU_SPLIT", 0) != 0;
    const hvec<int> &dpos = hp.dpos;
    const double t0 = now_ms();
    double t_lt = 0, t_tr = 0;  // diagnostics (RSP_ILU_TIMING >= 3): each pass's wall time
    // levels of the L^T DAG: row i waits for every j > i with l_ji != 0
    Task tt([&] {
        hvec<int> &lvt = hp.lev_lt;
        lvt.assign((size_t)n, 0);
        int nlt = n > 0 ? 1 : 0;
        for (int j = n - 1; j >= 0; j--) {
            nlt = std::max(nlt, lvt[(size_t)j] + 1);
            for (int p = rp[j]; p < dpos[(size_t)j]; p++) {
                const int k = ci[p];
                lvt[(size_t)k] = std::max(lvt[(size_t)k], lvt[(size_t)j] + 1);
            }
        }
        group_levels(lvt, nlt, hp.LT.ptr, hp.LT.rows);
        t_lt = now_ms() - t0;
    });
    // transposed strict lower: row k lists (j, pos) for l_jk, j descending.
    // Rows in parallel: counts and slots by relaxed atomics, then each
    // column's slots sorted by j (descending; one entry per j, so the order
    // is unique whatever the interleaving). Round 5: the sequential form was
    // the level phase's longest pass (tmt_unsym 9.4 ms against 4.4 / 4.6 ms
    // for the two level passes).
    hvec<int> &ltp = hp.ltp, &lts = hp.lts, &ltc = hp.ltc;
    ltp.assign((size_t)n + 1, 0);
    parallel_rows(n, [&](int r0, int r1) {
        for (int j = r0; j < r1; j++)
            for (int p = rp[j]; p < dpos[(size_t)j]; p++) __atomic_fetch_add(&ltp[(size_t)ci[p] + 1], 1, __ATOMIC_RELAXED);
    });
    for (int k = 0; k < n; k++) ltp[(size_t)k + 1] += ltp[(size_t)k];
    lts.resize((size_t)ltp[(size_t)n]);
    ltc.resize((size_t)ltp[(size_t)n]);
    {
        hvec<int> fill(ltp.begin(), ltp.end() - 1);
        parallel_rows(n, [&](int r0, int r1) {
            for (int j = r0; j < r1; j++)
                for (int p = rp[j]; p < dpos[(size_t)j]; p++) {
                    const int slot = __atomic_fetch_add(&fill[(size_t)ci[p]], 1, __ATOMIC_RELAXED);
                    lts[(size_t)slot] = p;
                    ltc[(size_t)slot] = j;
                }
        });
    }
    parallel_rows(n, [&](int k0, int k1) {
        std::vector<std::pair<int, int>> tmp;
        for (int k = k0; k < k1; k++) {
            const int a = ltp[(size_t)k], b = ltp[(size_t)k + 1];
            if (b - a <= 32) {  // insertion sort, j descending
                for (int x = a + 1; x < b; x++) {
                    const int cj = ltc[(size_t)x], cp = lts[(size_t)x];
                    int y = x - 1;
                    for (; y >= a && ltc[(size_t)y] < cj; y--) {
                        ltc[(size_t)y + 1] = ltc[(size_t)y];
                        lts[(size_t)y + 1] = lts[(size_t)y];
                    }
                    ltc[(size_t)y + 1] = cj;
                    lts[(size_t)y + 1] = cp;
                }
            } else {
                tmp.resize((size_t)(b - a));
                for (int x = a; x < b; x++) tmp[(size_t)(x - a)] = {ltc[(size_t)x], lts[(size_t)x]};
                std::sort(tmp.begin(), tmp.end(), [](const std::pair<int, int> &u, const std::pair<int, int> &v) {
                    return u.first > v.first;
                });
                for (int x = a; x < b; x++) {
                    ltc[(size_t)x] = tmp[(size_t)(x - a)].first;
                    lts[(size_t)x] = tmp[(size_t)(x - a)].second;
                }
            }
        }
    });
    t_tr = now_ms() - t0;
    tt.join();
    const double t_j = now_ms() - t0;
    if (split) split_terms(rp, ci, hp);
    if (env_int("RSP_ILU_TIMING", 0) >= 3)
        fprintf(stderr, "rsp_ilu0_analysis n=%d     levels: LT %.2f transpose %.2f joined %.2f split %.2f ms\n",
                n, t_lt, t_tr, t_j, now_ms() - t0 - t_j);
}

void plan_levels(const int *rp, const int *ci, IluHostPlan &hp) {
    hp.split = env_int("RSP_ILU_SPLIT", 0) != 0;
    Task tl([&] { plan_levels_lower(rp, ci, hp); });
    plan_levels_upper(rp, ci, hp, false);
    tl.join();
    split_terms(rp, ci, hp);
}

// The symbolic factor of every row (the all-host analysis): symbolic_row over
// contiguous row blocks, a column map per block; the count pass, the serial
// prefix sum into upd_ptr, then the fill pass (rows are independent: a row
// writes only its own positions and their update-list slots).
rsp_status_t plan_symbolic(const int *rp, const int *ci, IluHostPlan &hp) {
    const int n = hp.n, nnz = hp.nnz_s;
    IluSymbolic &s = hp.sym;
    hvec<int> cnt;
    resize_uninit(cnt, (size_t)nnz);
    auto pass = [&](int *counts) {
        parallel_rows(n, [&](int r0, int r1) {
            std::vector<int> map((size_t)n, -1), cur, order;
            for (int i = r0; i < r1; i++)
                symbolic_row(i, map, cur, order, rp, ci, hp.dpos.data(), hp.hasdiag.data(), counts,
                             s.upd_ptr.data(), s.upd_l.data(), s.upd_u.data(), s.stage.data(), s.lord.data(),
                             s.lend.data(), hp.udiv.data());
        });
    };
    pass(cnt.data());
    long long total = 0;
    for (int p = 0; p < nnz; p++) total += cnt[(size_t)p];
    if (total > INT_MAX) return RSP_STATUS_ALLOC_FAILED;
    s.upd_ptr.assign((size_t)nnz + 1, 0);
    for (int p = 0; p < nnz; p++) s.upd_ptr[(size_t)p + 1] = s.upd_ptr[(size_t)p] + cnt[(size_t)p];
    s.upd_l.resize((size_t)total);
    s.upd_u.resize((size_t)total);
    for (hvec<int> *v : {&s.stage, &s.lord, &s.lend, &hp.udiv}) resize_uninit(*v, (size_t)nnz);  // rows write all
    pass(nullptr);
    return RSP_STATUS_SUCCESS;
}

void plan_rest(const int *rp, const int *ci, long long slot_cap, bool want_u, IluHostPlan &hp) {
    Task ts([&] {
        plan_solves(rp, ci, hp);
        if (want_u) plan_u(rp, ci, hp);
    });
    plan_factor(rp, ci, slot_cap, hp);
    ts.join();
}

rsp_status_t plan_host(int n, const int *rp, const int *ci, long long slot_cap, bool want_u, IluHostPlan &hp,
                       Phases &ph) {
    rsp_status_t st = plan_validate(n, rp, ci, hp);
    if (st != RSP_STATUS_SUCCESS) return st;
    ph.mark("validate");
    plan_levels(rp, ci, hp);
    ph.mark("levels");
    st = plan_symbolic(rp, ci, hp);
    if (st != RSP_STATUS_SUCCESS) return st;
    ph.mark("symbolic");
    // the plans see what they see after the device analysis: no host copy of
    // the stage order, stage ends or divisor positions (kept for the digest)
    hvec<int> lord, lend, udiv;
    lord.swap(hp.sym.lord);
    lend.swap(hp.sym.lend);
    udiv.swap(hp.udiv);
    // ... and, like it, only the thin rows' update pairs, packed (the full
    // lists are kept for the digest)
    hvec<int> upd_l, upd_u;
    if (env_int("RSP_ILU_PACK_PAIRS", 1)) {
        const hvec<int> trows = factor_thin_rows(rp, hp);
        hvec<int> pl, pu;
        hp.sym.pair_base.assign((size_t)std::max(n, 1), 0);
        for (int i : trows) {
            hp.sym.pair_base[(size_t)i] = (int)pl.size();
            for (int q = hp.sym.upd_ptr[(size_t)rp[i]]; q < hp.sym.upd_ptr[(size_t)rp[i + 1]]; q++) {
                pl.push_back(hp.sym.upd_l[(size_t)q]);
                pu.push_back(hp.sym.upd_u[(size_t)q]);
            }
        }
        upd_l.swap(hp.sym.upd_l);
        upd_u.swap(hp.sym.upd_u);
        hp.sym.upd_l.swap(pl);
        hp.sym.upd_u.swap(pu);
    }
    plan_rest(rp, ci, slot_cap, want_u, hp);
    // block-inverse plans of the deep DAGs (as rsp_ilu0_analysis)
    if (blocks_wanted(n, (int)hp.L.ptr.size() - 1)) hp.has_lb = plan_blocks(0, rp, ci, hp, hp.Lb);
    if (blocks_wanted(n, (int)hp.LT.ptr.size() - 1)) hp.has_ltb = plan_blocks(1, rp, ci, hp, hp.LTb);
    lord.swap(hp.sym.lord);
    lend.swap(hp.sym.lend);
    udiv.swap(hp.udiv);
    if (!hp.sym.pair_base.empty()) {
        hp.sym.pair_base.clear();
        hp.sym.upd_l.swap(upd_l);
        hp.sym.upd_u.swap(upd_u);
    }
    ph.mark("plans");
    return RSP_STATUS_SUCCESS;
}

uint64_t digest(const IluHostPlan &hp) {
    Fnv f;
    f.bytes(&hp.n, sizeof(hp.n));
    f.bytes(&hp.structural_zero, sizeof(hp.structural_zero));
    f.vec(hp.dpos);
    f.vec(hp.hasdiag);
    f.vec(hp.udiv);
    f.vec(hp.sym.upd_ptr);
    f.vec(hp.sym.upd_l);
    f.vec(hp.sym.upd_u);
    f.vec(hp.sym.lord);
    f.vec(hp.sym.lend);
    for (const DagHost *d : {&hp.L, &hp.LT}) {
        f.vec(d->ptr);
        f.vec(d->rows);
        f.vec(d->sp.tasks);
        f.vec(d->sp.tpos);
        f.vec(d->sp.src);
        f.vec(d->sp.segs);
        f.vec(d->sp.chunks);
        f.vec(d->sp.trow);
        f.vec(d->sp.sid);
        f.vec(d->sp.stg);
        f.vec(d->sp.nshort);
        f.vec(d->sp.nwave);
        f.vec(d->sp.sbase);
        f.vec(d->sp.fitems);
    }
    for (const BlkPlanHost *b : {&hp.Lb, &hp.LTb}) {
        f.bytes(&b->nb, sizeof(b->nb));
        f.bytes(&b->lds_elems, sizeof(b->lds_elems));
        f.bytes(&b->lds_words, sizeof(b->lds_words));
        f.vec(b->order);
        f.vec(b->desc);
        f.vec(b->rows);
        f.vec(b->ref);
        f.vec(b->vpos);
        f.vec(b->eord);
        f.vec(b->lptr);
        f.vec(b->rptr);
        f.vec(b->rit);
        f.vec(b->segs);
    }
    f.bytes(&hp.fac_one, sizeof(hp.fac_one));
    f.bytes(&hp.fac_scale, sizeof(hp.fac_scale));
    f.vec(hp.F.ptr);
    f.vec(hp.F.rows);
    f.vec(hp.fplan.segs);
    f.vec(hp.fplan.chunks);
    f.vec(hp.fplan.items);
    f.vec(hp.fplan.pairs);
    f.vec(hp.fplan.staged);
    f.vec(hp.fplan.rounds);
    f.vec(hp.frow);
    f.vec(hp.fslev);
    f.vec(hp.slot_desc);
    f.vec(hp.slot_offs);
    f.vec(hp.fruns);
    f.vec(hp.ffitems);
    return f.h;
}

}  // namespace rsp_an
