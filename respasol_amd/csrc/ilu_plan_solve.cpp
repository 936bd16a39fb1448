// ilu_plan_solve.cpp — the solve plans of the ILU(0) host analysis (see
// ilu_analysis.h): the L and L^T DAGs' (plan_solves / plan_solves_rows) and the
// U DAG's (plan_u). No HIP calls here.

#include "ilu_analysis.h"

#include <stdio.h>

#include <algorithm>

namespace rsp_an {

// Solve plan of one DAG (see LevelPlan): tasks in level order over flat
// terms (term k of row i: matrix value at tpos[k], y of column col_of(k)),
// segments (a level is thin if it has <= thin_rows rows and its terms fit one
// chunk), the LDS-staged chunks of every thin run (<= kChunkRows rows and
// <= kChunkTerms terms each), and the y source of every term of a thin run:
// the LDS window slot (run index mod kYWin) if the column was produced earlier
// in the run and no later row of the run can have reused that slot by the end
// of the consumer's level, else the column (global y, or its value staged at
// the chunk start — the producer is then in an earlier chunk or before the
// run, so its store is visible after the chunk's full barrier).

// Built in two parts, each in parallel phases (rows, levels and chunks as
// work items, prefix sums over level order in between):
//   solve_plan_rows  (host): segments, row classes and order, tasks, flow
//                    items, the thin runs' chunks (levels, slots, terms) —
//                    per-row and per-level decisions; row_count(i) = the
//                    number of terms of row i;
//   solve_plan_terms (host; the device analysis runs ilu_an_solve_terms
//                    instead, the same arrays bit for bit): per flat term
//                    its position and y source, the window remap, the thin
//                    runs' row records, y indices and staged terms.
// A thin-run row's padded terms: its early and its late terms (split order,
// IluHostPlan::lpos) each padded to whole groups, at least one group.
static inline int split_padded(int ne, int cnt, int group) {
    const int pe = (ne + group - 1) / group * group, pl = (cnt - ne + group - 1) / group * group;
    return std::max(group, pe + pl);
}

template <typename RowCount, typename RowEarly>
static void solve_plan_rows(int n, const hvec<int> &ptr, const hvec<int> &rows,
                            int thin_rows, int group, const hvec<int> &diag,
                            RowCount row_count, RowEarly row_early, SolvePlan &sp) {
    const int nlev = (int)ptr.size() - 1;
    const long long nx = (long long)rows.size();
    constexpr long long kGrain = 1 << 14;
    const bool tm = env_int("RSP_ILU_TIMING", 0) >= 4;  // diagnostics: sub-steps
    double tq = now_ms();
    auto step = [&](const char *what) {
        if (!tm) return;
        const double t = now_ms();
        fprintf(stderr, "rsp_ilu0_analysis n=%d       solve rows %-10s %6.2f ms\n", n, what, t - tq);
        tq = t;
    };
    hvec<int> order(rows);
    // (row_count / row_early are O(1) lookups: called where needed, not
    // copied into per-row arrays first)
    auto padded_row = [&](int i) { return split_padded(row_early(i), row_count(i), group); };
    hvec<int> lpad((size_t)std::max(nlev, 1), 0);
    pfor_dyn(nlev, nx, kGrain, [&](int l) {
        int t = 0;
        for (int x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; x++) t += padded_row(order[(size_t)x]);
        lpad[(size_t)l] = t;
    });
    step("counts");
    // RSP_ILU_THIN_TERMS: tuning knob (a thin level's padded terms, <= kChunkTerms)
    const int thin_terms = std::min(env_int("RSP_ILU_THIN_TERMS", rsp::kThinSolveTerms), rsp::kChunkTerms);
    sp.segs.clear();
    for (int l = 0; l < nlev; l++) {
        const int cnt = ptr[(size_t)l + 1] - ptr[(size_t)l];
        const int thin = (cnt <= thin_rows && cnt <= rsp::kThinThreads && cnt <= rsp::kChunkRows &&
                          lpad[(size_t)l] <= thin_terms) ? 1 : 0;
        if (!sp.segs.empty() && sp.segs.back().thin == thin && sp.segs.back().le == l)
            sp.segs.back().le = l + 1;
        else
            sp.segs.push_back({l, l + 1, thin, 0, 0, 0});
    }
    hvec<char> thin_lev((size_t)std::max(nlev, 1), 0);
    for (const rsp::LevelSeg &sg : sp.segs)
        for (int l = sg.lb; l < sg.le; l++) thin_lev[(size_t)l] = (char)sg.thin;
    step("segs");
    // within each level (stable): short rows, then wave rows, then (fat
    // levels) hub rows
    const int fat_long = env_int("RSP_ILU_FAT_LONG", rsp::kFatLongDefault);
    const int hub = env_int("RSP_ILU_HUB", rsp::kHubTerms);
    sp.nshort.assign((size_t)std::max(nlev, 1), 0);
    sp.nwave.assign((size_t)std::max(nlev, 1), 0);
    pfor_dyn(nlev, nx, kGrain, [&](int l) {
        const int lim = thin_lev[(size_t)l] ? rsp::kLongTerms : fat_long;
        const int b = ptr[(size_t)l], e = ptr[(size_t)l + 1];
        int c[3] = {0, 0, 0};
        auto cls = [&](int i) {
            const int t = row_count(i);
            return t <= lim ? 0 : (thin_lev[(size_t)l] || t <= hub ? 1 : 2);
        };
        for (int x = b; x < e; x++) c[cls(order[(size_t)x])]++;
        sp.nshort[(size_t)l] = c[0];
        sp.nwave[(size_t)l] = c[0] + c[1];
        if (c[0] == e - b || c[1] == e - b || c[2] == e - b) return;  // one class: order unchanged
        hvec<int> tmp(order.begin() + b, order.begin() + e);
        int w[3] = {b, b + c[0], b + c[0] + c[1]};
        for (int i : tmp) order[(size_t)w[cls(i)]++] = i;
    });
    step("classes");
    // flat term ranges in level order: a thin row's terms padded to whole
    // groups; a padded fat level's short rows own kFatLongTerms terms each
    const bool pad_fat = fat_long == rsp::kFatLongTerms && env_int("RSP_ILU_FAT_PAD", 1) != 0;
    sp.sbase.assign((size_t)std::max(nlev, 1), -1);
    sp.tasks.assign(std::max<size_t>(rows.size(), 1), rsp::RowTask{0, 0, 0, -1});
    hvec<int> len((size_t)std::max(nx, 1LL), 0);
    pfor_dyn(nlev, nx, kGrain, [&](int l) {
        const bool padl = pad_fat && !thin_lev[(size_t)l] && sp.nshort[(size_t)l] > 0;
        for (int x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; x++) {
            const int i = order[(size_t)x], t = row_count(i);
            const int t1 = thin_lev[(size_t)l] ? padded_row(i) : t;
            len[(size_t)x] = padl && x - ptr[(size_t)l] < sp.nshort[(size_t)l] ? std::max(t1, rsp::kFatLongTerms) : t1;
            sp.tasks[(size_t)x].t1 = t1;  // length for now
        }
    });
    step("lengths");
    long long total = 0;
    for (long long x = 0; x < nx; x++) {
        sp.tasks[(size_t)x].t0 = (int)total;
        total += len[(size_t)x];
    }
    for (int l = 0; l < nlev; l++)
        if (pad_fat && !thin_lev[(size_t)l] && sp.nshort[(size_t)l] > 0) sp.sbase[(size_t)l] = sp.tasks[(size_t)ptr[(size_t)l]].t0;
    sp.nterm = total;
    step("prefix");
    pfor(nx, kGrain, [&](long long a, long long b) {
        for (long long x = a; x < b; x++) {
            rsp::RowTask &t = sp.tasks[(size_t)x];
            t.i = order[(size_t)x];
            t.t1 += t.t0;
            t.d = diag.empty() ? -1 : diag[(size_t)t.i];
        }
    });
    step("tasks");
    // flow segments: fat segments of two or more levels run as one persistent
    // launch (trsv_flow) over work items in level order — a level's short rows
    // in groups of 64 (a lane each), then its wave and hub rows (a wave each).
    // Short rows must fit one batch of kFatLongTerms terms (RSP_ILU_FAT_LONG).
    sp.fitems.clear();
    const int gate_d = env_int("RSP_ILU_FLOW_GATE", 3);  // levels between an item and its gate (0: none)
    if (fat_long <= rsp::kFatLongTerms && env_int("RSP_ILU_FLOW_PLAN", 1) != 0)
        for (rsp::LevelSeg &sg : sp.segs) {
            if (sg.thin || sg.le - sg.lb < 2) continue;
            sg.c0 = (int)sp.fitems.size();
            for (int l = sg.lb; l < sg.le; l++) {
                const int p0 = ptr[(size_t)l], cnt = ptr[(size_t)l + 1] - p0, ns = sp.nshort[(size_t)l];
                const int sb = sp.sbase[(size_t)l];
                // gate: the last row of level l - gate_d when it is in this segment
                const int lg = l - gate_d;
                const int gate = gate_d > 0 && lg >= sg.lb && ptr[(size_t)lg + 1] > ptr[(size_t)lg]
                                     ? order[(size_t)ptr[(size_t)lg + 1] - 1] : -1;
                for (int r = 0; r < ns; r += 64)
                    sp.fitems.push_back({p0 + r, std::min(64, ns - r), sb >= 0 ? sb + r * rsp::kFatLongTerms : -1, gate});
                for (int r = ns; r < cnt; r++) sp.fitems.push_back({p0 + r, 0, -1, gate});
            }
            sg.c1 = (int)sp.fitems.size();
        }
    if (env_int("RSP_ILU_PLANSTATS", 0)) {  // diagnostics: the segment structure of this DAG
        int nthin = 0, nfat = 0, nflow = 0, lthin = 0, lfat = 0, lflow = 0;
        for (const rsp::LevelSeg &sg : sp.segs) {
            const int nl = sg.le - sg.lb;
            if (sg.thin) nthin++, lthin += nl;
            else if (sg.c1 > sg.c0) nflow++, lflow += nl;
            else nfat++, lfat += nl;
        }
        fprintf(stderr, "rsp_ilu0 plan n=%d levels=%d group=%d thin %d segs / %d levels, fat %d / %d, flow %d / %d (%zu items)\n",
                n, nlev, group, nthin, lthin, nfat, lfat, nflow, lflow, sp.fitems.size());
    }
    if (sp.fitems.empty()) sp.fitems.push_back({0, 0, -1, -1});
    step("flow");
    hvec<int> lterms((size_t)std::max(nlev, 1), 0);
    for (int l = 0; l < nlev; l++)
        if (ptr[(size_t)l + 1] > ptr[(size_t)l])
            lterms[(size_t)l] = sp.tasks[(size_t)ptr[(size_t)l + 1] - 1].t1 - sp.tasks[(size_t)ptr[(size_t)l]].t0;
    for (rsp::LevelSeg &sg : sp.segs)
        if (sg.thin) sg.nth = rsp::kThinThreads;
    // chunks of the thin runs (greedy over levels): levels, slots, terms, and
    // each chunk's run base (the run's first slot)
    sp.chunks.clear();
    sp.cbase.clear();
    for (rsp::LevelSeg &sg : sp.segs) {
        if (!sg.thin) continue;
        sg.c0 = (int)sp.chunks.size();
        int crow = 0, cterm = 0;
        for (int l = sg.lb; l < sg.le; l++) {
            const int cnt = ptr[(size_t)l + 1] - ptr[(size_t)l];
            if (sp.chunks.size() == (size_t)sg.c0 || crow + cnt > rsp::kChunkRows ||
                cterm + lterms[(size_t)l] > rsp::kChunkTerms) {
                sp.chunks.push_back({l, l + 1, 0, 0, 0, 0, 0, 0});
                sp.cbase.push_back(ptr[(size_t)sg.lb]);
                crow = 0;
                cterm = 0;
            } else {
                sp.chunks.back().l1 = l + 1;
            }
            crow += cnt;
            cterm += lterms[(size_t)l];
        }
        sg.c1 = (int)sp.chunks.size();
    }
    for (rsp::LevelChunk &ch : sp.chunks) {
        ch.x0 = ptr[(size_t)ch.l0];
        ch.x1 = ptr[(size_t)ch.l1];
        ch.k0 = ch.x1 > ch.x0 ? sp.tasks[(size_t)ch.x0].t0 : 0;
        ch.k1 = ch.x1 > ch.x0 ? sp.tasks[(size_t)ch.x1 - 1].t1 : 0;
    }
    if (sp.chunks.empty()) {
        sp.chunks.push_back({0, 0, 0, 0, 0, 0, 0, 0});
        sp.cbase.push_back(0);
    }
    step("chunks");
}

// row_terms(i, emit) calls emit(tpos, col) for the terms of row i in order
// (row_count(i) of them, as given to solve_plan_rows; the first row_early(i)
// of them early). A thin row (its task spans split_padded terms) places its
// late terms at the first group after its early ones; other rows keep their
// terms contiguous (when split_padded equals the count the two coincide).
static inline int late_offset(int ne, int cnt, int len, int group) {
    return len == split_padded(ne, cnt, group) ? (ne + group - 1) / group * group : ne;
}
template <typename RowTerms, typename RowEarly>
static void solve_plan_terms(int n, const hvec<int> &ptr, int group, RowTerms row_terms, RowEarly row_early,
                             SolvePlan &sp) {
    constexpr long long kGrain = 1 << 14;
    const int nlev = (int)ptr.size() - 1;
    const long long nx = (long long)ptr[(size_t)nlev], total = sp.nterm;
    sp.tpos.assign((size_t)total, -1);
    hvec<int> col((size_t)total, -1);
    hvec<int> egroups((size_t)std::max(nx, 1LL), 0);  // thin rows: whole groups of early terms
    pfor(nx, kGrain, [&](long long a, long long b) {
        for (long long x = a; x < b; x++) {
            const rsp::RowTask &t = sp.tasks[(size_t)x];
            const int ne = row_early(t.i);
            int cnt = 0;
            row_terms(t.i, [&](int, int) { cnt++; });
            const int lo = late_offset(ne, cnt, t.t1 - t.t0, group);
            if (t.t1 - t.t0 == split_padded(ne, cnt, group)) egroups[(size_t)x] = lo / group;
            int o = 0;
            row_terms(t.i, [&](int tp, int c) {
                const int k = t.t0 + (o < ne ? o : lo + (o - ne));
                sp.tpos[(size_t)k] = tp;
                col[(size_t)k] = c;
                o++;
            });
        }
    });
    sp.src.resize((size_t)total);
    pfor(total, kGrain, [&](long long a, long long b) {
        for (long long k = a; k < b; k++) sp.src[(size_t)k] = col[(size_t)k] < 0 ? rsp::kPadSrc : col[(size_t)k];
    });
    hvec<int> slot_of((size_t)n, -1);
    pfor(nx, kGrain, [&](long long a, long long b) {
        for (long long x = a; x < b; x++) slot_of[(size_t)sp.tasks[(size_t)x].i] = (int)x;
    });
    hvec<int> thin_base((size_t)std::max(nlev, 1), -1);  // per thin level: its run's first slot
    for (const rsp::LevelSeg &sg : sp.segs)
        if (sg.thin)
            for (int l = sg.lb; l < sg.le; l++) thin_base[(size_t)l] = ptr[(size_t)sg.lb];
    // y sources of the thin runs' terms: the LDS window slot when the
    // producer is earlier in the run and still in the window
    pfor_dyn(nlev, nx, kGrain, [&](int l) {
        const int base = thin_base[(size_t)l];
        if (base < 0) return;
        const int r_end = ptr[(size_t)l + 1] - base;
        for (int x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; x++)
            for (int k = sp.tasks[(size_t)x].t0; k < sp.tasks[(size_t)x].t1; k++) {
                if (col[(size_t)k] < 0) continue;  // pad
                const int sj = slot_of[(size_t)col[(size_t)k]];
                if (sj < base || sj >= ptr[(size_t)l]) continue;  // before the run
                const int rj = sj - base;
                if (r_end - rj <= rsp::kYWin) sp.src[(size_t)k] = -((rj & (rsp::kYWin - 1)) + 1);
            }
    });
    if (sp.tpos.empty()) {
        sp.tpos.push_back(0);
        sp.src.push_back(0);
    }
    // per chunk: static row records, term y indices, staged terms (counted
    // per chunk, then filled at their prefix offsets)
    sp.trow.assign(std::max<size_t>((size_t)nx, 1), rsp::ThinRowPlan{0, 0, 0, -1});
    sp.sid.assign(sp.tpos.size(), rsp::kYWin);
    const int nch = (int)sp.chunks.size();
    hvec<int> nst((size_t)std::max(nch, 1), 0);
    pfor_dyn(nch, nx, kGrain, [&](int c) {
        const rsp::LevelChunk &ch = sp.chunks[(size_t)c];
        int m = 0;
        for (int x = ch.x0; x < ch.x1; x++)
            for (int k = sp.tasks[(size_t)x].t0; k < sp.tasks[(size_t)x].t1; k++) m += sp.src[(size_t)k] >= 0;
        nst[(size_t)c] = m;
    });
    long long nstg = 0;
    for (int c = 0; c < nch; c++) {
        sp.chunks[(size_t)c].st0 = (int)nstg;
        nstg += nst[(size_t)c];
        sp.chunks[(size_t)c].st1 = (int)nstg;
    }
    sp.stg.assign((size_t)nstg, rsp::StagedTerm{0, 0});
    pfor_dyn(nch, nx, kGrain, [&](int c) {
        const rsp::LevelChunk &ch = sp.chunks[(size_t)c];
        const int base = sp.cbase[(size_t)c];
        int st = ch.st0;
        for (int x = ch.x0; x < ch.x1; x++) {
            const rsp::RowTask &t = sp.tasks[(size_t)x];
            sp.trow[(size_t)x] = {(t.t0 - ch.k0) / group | ((t.t1 - t.t0) / group) << 16,
                                  ((x - base) & (rsp::kYWin - 1)) | egroups[(size_t)x] << 16, t.i, t.d};
            for (int k = t.t0; k < t.t1; k++) {
                const int sc = sp.src[(size_t)k];
                if (sc < 0) {
                    sp.sid[(size_t)k] = -sc - 1;
                } else {
                    sp.sid[(size_t)k] = rsp::kYWin + 1 + (k - ch.k0);
                    sp.stg[(size_t)st++] = {k - ch.k0, sc};
                }
            }
        }
    });
    if (sp.stg.empty()) sp.stg.push_back({0, 0});
}

// Both parts on the host.
template <typename RowCount, typename RowTerms, typename RowEarly>
static void build_solve_plan(int n, const hvec<int> &ptr, const hvec<int> &rows,
                             int thin_rows, int group, const hvec<int> &diag,
                             RowCount row_count, RowTerms row_terms, RowEarly row_early, SolvePlan &sp) {
    solve_plan_rows(n, ptr, rows, thin_rows, group, diag, row_count, row_early, sp);
    solve_plan_terms(n, ptr, group, row_terms, row_early, sp);
}

// RSP_ILU_THIN_SOLVE: tuning knob of all three DAGs (0 = no thin runs)
static int thin_solve_rows() {
    return std::min(env_int("RSP_ILU_THIN_SOLVE", rsp::kThinSolveRows), rsp::kThinThreads);
}

// The L and L^T solve plans; terms_on_host = false builds only the per-row
// half (the device analysis builds the per-term half on the MI355X:
// rsp_k::ilu_an_solve_terms).
static void plan_solves_impl(const int *rp, const int *ci, IluHostPlan &hp, bool terms_on_host) {
    const int n = hp.n;
    const hvec<int> &dpos = hp.dpos;
    const hvec<int> &ltp = hp.ltp, &lts = hp.lts, &ltc = hp.ltc;
    const int thin_solve = thin_solve_rows();
    long long nlo = 0;
    for (int i = 0; i < n; i++) nlo += dpos[(size_t)i] - rp[(size_t)i];
    hp.L.batch = hp.LT.batch = chain_batch(nlo, n);
    auto cnt_l = [&](int i) { return dpos[(size_t)i] - rp[(size_t)i]; };
    auto cnt_lt = [&](int i) { return ltp[(size_t)i + 1] - ltp[(size_t)i]; };
    // thin-run term groups, per DAG. Reference order (default): 2 only where
    // groups of 4 would save almost no groups (sum ceil(c/2) <= 1.15 sum
    // ceil(c/4): chains of <= 2 terms, the 2-D grids), else 4 — a circuit's
    // short mean chain hides hub rows of thousands of terms (config 3, same
    // box: G2_circuit solve 3.21 -> 2.66 ms, ASIC_320ks 1.52 -> 1.31, ss1
    // 1.34 -> 1.16 against the round-3 rule of 2 for every DAG of mean chain
    // <= 2.5; ecology2 / tmt_unsym keep 2: 4.26 / 4.22 against 4.49 / 4.45 ms
    // with 4; profiles/r04_ilu_group_ab.txt). Split order (RSP_ILU_SPLIT=1):
    // 2 where a row's two parts are short on average (mean chain <= 5 terms).
    auto group_of = [&](auto cnt) {
        if (hp.split) return n > 0 && (double)nlo / n <= 5.0 ? 2 : 4;
        long long s2 = 0, s4 = 0;
        for (int i = 0; i < n; i++) {
            const int c = cnt(i);
            s2 += (c + 1) / 2;
            s4 += (c + 3) / 4;
        }
        return 100 * s2 <= 115 * s4 ? 2 : 4;
    };
    const int g_env = env_int("RSP_ILU_GROUP", 0);
    hp.L.group = g_env ? (g_env == 2 ? 2 : 4) : group_of(cnt_l);
    hp.LT.group = g_env ? (g_env == 2 ? 2 : 4) : group_of(cnt_lt);
    // split term order (IluHostPlan::lpos): early terms first
    // (empty: the reference's order, split_terms)
    auto ne_l = [&](int i) { return hp.ne_l.empty() ? 0 : hp.ne_l[(size_t)i]; };
    auto ne_lt = [&](int i) { return hp.ne_lt.empty() ? 0 : hp.ne_lt[(size_t)i]; };
    // the two DAGs' plans (flat terms in level order, thin-run chunks, y
    // sources) are independent: built concurrently
    Task tl([&] {
        timed_plan(n, "L", [&] {
            solve_plan_rows(n, hp.L.ptr, hp.L.rows, thin_solve, hp.L.group, hvec<int>(), cnt_l, ne_l, hp.L.sp);
            if (terms_on_host)
                solve_plan_terms(n, hp.L.ptr, hp.L.group, [&](int i, auto emit) {
                    for (int o = rp[(size_t)i]; o < dpos[(size_t)i]; o++) {
                        const int p = hp.lpos.empty() ? o : hp.lpos[(size_t)o];
                        emit(p, ci[(size_t)p]);
                    }
                }, ne_l, hp.L.sp);
        });
    });
    timed_plan(n, "LT", [&] {
        solve_plan_rows(n, hp.LT.ptr, hp.LT.rows, thin_solve, hp.LT.group, hvec<int>(), cnt_lt, ne_lt, hp.LT.sp);
        if (terms_on_host)
            solve_plan_terms(n, hp.LT.ptr, hp.LT.group, [&](int i, auto emit) {
                for (int q = ltp[(size_t)i]; q < ltp[(size_t)i + 1]; q++) emit(lts[(size_t)q], ltc[(size_t)q]);
            }, ne_lt, hp.LT.sp);
    });
    tl.join();
    hp.L.planned = hp.LT.planned = true;
}

void plan_solves(const int *rp, const int *ci, IluHostPlan &hp) { plan_solves_impl(rp, ci, hp, true); }
void plan_solves_rows(const int *rp, const int *ci, IluHostPlan &hp) { plan_solves_impl(rp, ci, hp, false); }

// The U DAG (extension: the true L.U apply, rsp_trsv_upper): row i waits
// for every j > i with u_ij != 0.
void plan_u(const int *rp, const int *ci, IluHostPlan &hp) {
    const int n = hp.n;
    const hvec<int> &dpos = hp.dpos, &hasdiag = hp.hasdiag;
    hvec<int> lvu((size_t)n, 0);
    int nlu = n > 0 ? 1 : 0;
    for (int i = n - 1; i >= 0; i--) {
        int l = 0;
        for (int p = dpos[(size_t)i] + hasdiag[(size_t)i]; p < rp[(size_t)i + 1]; p++)
            l = std::max(l, lvu[(size_t)ci[(size_t)p]] + 1);
        lvu[(size_t)i] = l;
        nlu = std::max(nlu, l + 1);
    }
    group_levels(lvu, nlu, hp.U.ptr, hp.U.rows);
    long long nu = 0;
    for (int i = 0; i < n; i++) nu += rp[(size_t)i + 1] - dpos[(size_t)i] - hasdiag[(size_t)i];
    hp.U.batch = chain_batch(nu, n);
    hp.U.group = env_int("RSP_ILU_GROUP", hp.U.batch == 2 ? 2 : 4) == 2 ? 2 : 4;
    hvec<int> udiag((size_t)n);
    for (int i = 0; i < n; i++) udiag[(size_t)i] = hasdiag[(size_t)i] ? dpos[(size_t)i] : -1;
    build_solve_plan(n, hp.U.ptr, hp.U.rows, thin_solve_rows(), hp.U.group, udiag,
                     [&](int i) { return rp[(size_t)i + 1] - dpos[(size_t)i] - hasdiag[(size_t)i]; },
                     [&](int i, auto emit) {
        for (int p = dpos[(size_t)i] + hasdiag[(size_t)i]; p < rp[(size_t)i + 1]; p++) emit(p, ci[(size_t)p]);
    }, [](int) { return 0; }, hp.U.sp);  // (the U solve keeps the reference order: no split)
    hp.U.planned = true;
}

}  // namespace rsp_an
