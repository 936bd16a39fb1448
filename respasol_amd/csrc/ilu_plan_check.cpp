// ilu_plan_check.cpp — validity check and facts of the level plans the ILU(0)
// host analysis builds (see ilu_analysis.h: check_plans, plan_facts; the C
// entry is rsp_ilu0_plan_facts_host). Tests only: the kernels never call it.
// The check restates what the kernels of ilu0.hip / trsv.hip rely on, from
// the pattern and the level sets alone — it shares no code with the planners
// (ilu_plan_solve.cpp, ilu_plan_factor.cpp) beyond the record layouts. No HIP
// calls here.

#include "ilu_analysis.h"

#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <functional>
#include <utility>
#include <vector>

namespace rsp_an {
namespace {

std::string fmt(const char *f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
#define CHK(cond, ...)                         \
    do {                                       \
        if (!(cond)) return fmt(__VA_ARGS__);  \
    } while (0)

inline int round_up(int v, int g) { return (v + g - 1) / g * g; }
// a thin row's flat terms: early and late part each in whole groups, >= one group
inline int padded_terms(int ne, int cnt, int g) { return std::max(g, round_up(ne, g) + round_up(cnt - ne, g)); }

using TermList = std::vector<std::pair<int, int>>;  // (position in vals, column) in solve order
struct DagView {
    const char *name;
    const DagHost *d;
    std::function<void(int, TermList &)> terms;
    std::function<int(int)> early, diag;
};

// per level: 1 thin, 0 fat; "" or what is wrong with the segments
std::string seg_levels(const char *nm, const hvec<rsp::LevelSeg> &segs, int nlev, std::vector<char> &thin) {
    thin.assign((size_t)std::max(nlev, 1), 0);
    int l = 0;
    for (const rsp::LevelSeg &sg : segs) {
        CHK(sg.lb == l && sg.le > sg.lb && sg.le <= nlev, "%s: segment [%d, %d) after level %d", nm, sg.lb, sg.le, l);
        for (l = sg.lb; l < sg.le; l++) thin[(size_t)l] = (char)(sg.thin != 0);
    }
    CHK(l == nlev, "%s: segments end at level %d of %d", nm, l, nlev);
    return "";
}

std::string check_solve(int n, const DagView &v) {
    const char *nm = v.name;
    const DagHost &d = *v.d;
    const SolvePlan &sp = d.sp;
    const hvec<int> &ptr = d.ptr;
    const int nlev = (int)ptr.size() - 1, g = d.group;
    CHK(d.planned && (g == 2 || g == 4), "%s: not planned, or group %d", nm, g);
    CHK((int)d.rows.size() == n && ptr[0] == 0 && ptr[(size_t)nlev] == n, "%s: level sets do not hold %d rows", nm, n);
    CHK(n == 0 || (int)sp.tasks.size() == n, "%s: %zu tasks for %d rows", nm, sp.tasks.size(), n);
    if (n == 0) return "";
    std::vector<char> thin;
    std::string e = seg_levels(nm, sp.segs, nlev, thin);
    if (!e.empty()) return e;
    CHK((int)sp.nshort.size() >= nlev && (int)sp.nwave.size() >= nlev && (int)sp.sbase.size() >= nlev,
        "%s: per-level arrays shorter than %d", nm, nlev);
    CHK(sp.nterm >= 0 && (long long)sp.tpos.size() >= sp.nterm && sp.src.size() == sp.tpos.size() &&
            sp.sid.size() == sp.tpos.size(), "%s: term arrays do not hold %d terms", nm, sp.nterm);
    const int fat_long = env_int("RSP_ILU_FAT_LONG", rsp::kFatLongDefault);
    const int hub = env_int("RSP_ILU_HUB", rsp::kHubTerms);

    // ---- tasks: every row once, in level order, short / wave / hub within a level;
    // flat terms: the row's own, in solve order, pads only where a thin row's groups end
    std::vector<int> lev_of((size_t)n, -1), slot_of((size_t)n, -1), col((size_t)std::max(sp.nterm, 1), -2);
    std::vector<int> lo_groups((size_t)n, 0);  // per slot: whole groups of early terms (thin rows)
    for (int l = 0; l < nlev; l++)
        for (int x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; x++) lev_of[(size_t)d.rows[(size_t)x]] = l;
    TermList tv;
    std::vector<int> want_pos, want_col;
    int prev_t1 = 0;
    for (int l = 0; l < nlev; l++) {
        const int b = ptr[(size_t)l], en = ptr[(size_t)l + 1], lim = thin[(size_t)l] ? rsp::kLongTerms : fat_long;
        const int sb = sp.sbase[(size_t)l];
        CHK(sb < 0 || (!thin[(size_t)l] && sp.nshort[(size_t)l] > 0 && sb == sp.tasks[(size_t)b].t0),
            "%s: level %d: padded short-row base %d", nm, l, sb);
        int cls_cnt[3] = {0, 0, 0}, prev_cls = 0, prev_i = -1;
        for (int x = b; x < en; x++) {
            const rsp::RowTask &t = sp.tasks[(size_t)x];
            CHK(t.i >= 0 && t.i < n && lev_of[(size_t)t.i] == l && slot_of[(size_t)t.i] < 0,
                "%s: slot %d of level %d holds row %d (another level's, or twice)", nm, x, l, t.i);
            slot_of[(size_t)t.i] = x;
            v.terms(t.i, tv);
            const int c = (int)tv.size(), ne = v.early(t.i), len = t.t1 - t.t0;
            const int cls = c <= lim ? 0 : (thin[(size_t)l] || c <= hub ? 1 : 2);
            CHK(cls > prev_cls || (cls == prev_cls && t.i > prev_i), "%s: level %d: row %d (class %d) after row %d (class %d)",
                nm, l, t.i, cls, prev_i, prev_cls);
            prev_cls = cls, prev_i = t.i;
            cls_cnt[cls]++;
            CHK(ne >= 0 && ne <= c, "%s: row %d: %d early of %d terms", nm, t.i, ne, c);
            const int want_len = thin[(size_t)l] ? padded_terms(ne, c, g) : c;
            const int lo = thin[(size_t)l] ? round_up(ne, g) : ne;
            CHK(len == want_len, "%s: row %d: %d flat terms, %d wanted", nm, t.i, len, want_len);
            CHK(t.t0 >= prev_t1 && t.t1 <= sp.nterm, "%s: row %d: terms [%d, %d) overlap or pass %d", nm, t.i, t.t0, t.t1, sp.nterm);
            CHK(!(thin[(size_t)l] && x > b) || t.t0 == prev_t1, "%s: row %d: gap before its terms in a thin level", nm, t.i);
            CHK(!(sb >= 0 && x - b < sp.nshort[(size_t)l]) || t.t0 == sb + (x - b) * rsp::kFatLongTerms,
                "%s: row %d: padded short row at term %d", nm, t.i, t.t0);
            prev_t1 = t.t1;
            CHK(t.d == v.diag(t.i), "%s: row %d: diagonal %d", nm, t.i, t.d);
            want_pos.assign((size_t)len, -1);
            want_col.assign((size_t)len, -1);
            for (int o = 0; o < c; o++) {
                const int k = o < ne ? o : lo + (o - ne);
                CHK(k < len && want_col[(size_t)k] < 0, "%s: row %d: term %d has no place", nm, t.i, o);
                want_pos[(size_t)k] = tv[(size_t)o].first;
                want_col[(size_t)k] = tv[(size_t)o].second;
            }
            for (int k = 0; k < len; k++) {
                const int f = t.t0 + k;
                CHK(sp.tpos[(size_t)f] == want_pos[(size_t)k], "%s: row %d: term %d reads position %d, %d wanted", nm, t.i, k,
                    sp.tpos[(size_t)f], want_pos[(size_t)k]);
                col[(size_t)f] = want_col[(size_t)k];
                if (want_col[(size_t)k] < 0)
                    CHK(sp.src[(size_t)f] == rsp::kPadSrc, "%s: row %d: pad term %d has source %d", nm, t.i, k, sp.src[(size_t)f]);
                else if (!thin[(size_t)l])
                    CHK(sp.src[(size_t)f] == want_col[(size_t)k], "%s: row %d: term %d has source %d, column %d", nm, t.i, k,
                        sp.src[(size_t)f], want_col[(size_t)k]);
            }
            lo_groups[(size_t)x] = thin[(size_t)l] ? lo / g : 0;
        }
        CHK(sp.nshort[(size_t)l] == cls_cnt[0] && sp.nwave[(size_t)l] == cls_cnt[0] + cls_cnt[1],
            "%s: level %d: nshort %d nwave %d, classes %d / %d / %d", nm, l, sp.nshort[(size_t)l], sp.nwave[(size_t)l],
            cls_cnt[0], cls_cnt[1], cls_cnt[2]);
    }

    // ---- thin runs: chunks, row records, window and staged terms
    int st_next = -1;
    for (const rsp::LevelSeg &sg : sp.segs) {
        if (!sg.thin) continue;
        const int base = ptr[(size_t)sg.lb];
        CHK(sg.c0 >= 0 && sg.c1 > sg.c0 && sg.c1 <= (int)sp.chunks.size() && sp.cbase.size() == sp.chunks.size(),
            "%s: thin segment [%d, %d): chunks [%d, %d)", nm, sg.lb, sg.le, sg.c0, sg.c1);
        int x_next = base, l_next = sg.lb;
        for (int c = sg.c0; c < sg.c1; c++) {
            const rsp::LevelChunk &ch = sp.chunks[(size_t)c];
            CHK(ch.x1 - ch.x0 <= rsp::kChunkRows, "%s: chunk %d holds %d rows", nm, c, ch.x1 - ch.x0);
            CHK(ch.l0 == l_next && ch.l1 > ch.l0 && ch.l1 <= sg.le && ch.x0 == x_next && ch.x0 == ptr[(size_t)ch.l0] &&
                    ch.x1 == ptr[(size_t)ch.l1], "%s: chunk %d: levels [%d, %d) slots [%d, %d) do not tile the run", nm, c,
                ch.l0, ch.l1, ch.x0, ch.x1);
            CHK(ch.x1 > ch.x0, "%s: chunk %d is empty", nm, c);
            CHK(ch.k0 == sp.tasks[(size_t)ch.x0].t0 && ch.k1 == sp.tasks[(size_t)ch.x1 - 1].t1,
                "%s: chunk %d: terms [%d, %d)", nm, c, ch.k0, ch.k1);
            CHK(ch.k1 - ch.k0 <= rsp::kChunkTerms, "%s: chunk %d holds %d terms", nm, c, ch.k1 - ch.k0);
            CHK(sp.cbase[(size_t)c] == base, "%s: chunk %d: run base %d", nm, c, sp.cbase[(size_t)c]);
            CHK(ch.st1 >= ch.st0 && ch.st0 >= 0 && ch.st1 <= (int)sp.stg.size() && (st_next < 0 || ch.st0 == st_next),
                "%s: chunk %d: staged range [%d, %d)", nm, c, ch.st0, ch.st1);
            st_next = ch.st1;
            x_next = ch.x1, l_next = ch.l1;
            std::vector<int> stg_at((size_t)(ch.k1 - ch.k0), -1);
            for (int s = ch.st0; s < ch.st1; s++) {
                const rsp::StagedTerm &st = sp.stg[(size_t)s];
                CHK(st.slot >= 0 && st.slot < ch.k1 - ch.k0 && stg_at[(size_t)st.slot] < 0 && st.j >= 0 && st.j < n,
                    "%s: chunk %d: staged term %d (slot %d, row %d)", nm, c, s, st.slot, st.j);
                stg_at[(size_t)st.slot] = st.j;
            }
            int staged = 0;
            for (int l = ch.l0; l < ch.l1; l++)
                for (int x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; x++) {
                    const rsp::RowTask &t = sp.tasks[(size_t)x];
                    const rsp::ThinRowPlan &tr = sp.trow[(size_t)x];
                    const int first = (t.t0 - ch.k0) / g, groups = (t.t1 - t.t0) / g, out = (x - base) & (rsp::kYWin - 1);
                    CHK((t.t0 - ch.k0) % g == 0 && (tr.g & 0xffff) == first && (int)((unsigned)tr.g >> 16) == groups &&
                            first < 65536 && groups < 65536, "%s: row %d: record groups %#x, first %d count %d", nm, t.i,
                        tr.g, first, groups);
                    CHK((tr.out & 0xffff) == out && (int)((unsigned)tr.out >> 16) == lo_groups[(size_t)x],
                        "%s: row %d: record out %#x, slot %d early groups %d", nm, t.i, tr.out, out, lo_groups[(size_t)x]);
                    CHK(tr.i == t.i && tr.d == t.d, "%s: row %d: record row %d diagonal %d", nm, t.i, tr.i, tr.d);
                    for (int k = t.t0; k < t.t1; k++) {
                        const int cj = col[(size_t)k], sc = sp.src[(size_t)k], rel = k - ch.k0;
                        if (cj < 0) {
                            CHK(sp.sid[(size_t)k] == rsp::kYWin && stg_at[(size_t)rel] < 0, "%s: row %d: pad term %d is staged or reads y %d",
                                nm, t.i, k, sp.sid[(size_t)k]);
                            continue;
                        }
                        const int sj = slot_of[(size_t)cj];
                        CHK(sj >= 0 && sj < ptr[(size_t)l], "%s: row %d reads row %d of its own or a later level", nm, t.i, cj);
                        if (sc < 0) {
                            const int s = -sc - 1;
                            CHK(s < rsp::kYWin && sj >= base && ((sj - base) & (rsp::kYWin - 1)) == s,
                                "%s: row %d: window slot %d is not row %d's (run slot %d)", nm, t.i, s, cj, sj - base);
                            CHK(ptr[(size_t)l + 1] - sj <= rsp::kYWin, "%s: row %d: row %d is %d slots before its level's end", nm,
                                t.i, cj, ptr[(size_t)l + 1] - sj);
                            CHK(sp.sid[(size_t)k] == s && stg_at[(size_t)rel] < 0, "%s: row %d: window term %d has y index %d", nm,
                                t.i, k, sp.sid[(size_t)k]);
                        } else {
                            CHK(sc == cj && sj < ch.x0, "%s: row %d: staged term %d (source %d, column %d) produced in its own chunk",
                                nm, t.i, k, sc, cj);
                            CHK(stg_at[(size_t)rel] == cj, "%s: row %d: term %d (row %d) is not staged in chunk %d", nm, t.i, k, cj, c);
                            CHK(sp.sid[(size_t)k] == rsp::kYWin + 1 + rel, "%s: row %d: staged term %d has y index %d", nm, t.i, k,
                                sp.sid[(size_t)k]);
                            staged++;
                        }
                    }
                }
            CHK(staged == ch.st1 - ch.st0, "%s: chunk %d: %d staged records for %d staged terms", nm, c, ch.st1 - ch.st0, staged);
        }
        CHK(x_next == ptr[(size_t)sg.le], "%s: thin segment [%d, %d): chunks end at slot %d", nm, sg.lb, sg.le, x_next);
    }

    // ---- flow segments: items cover each level's rows once, in order
    const int gate_d = env_int("RSP_ILU_FLOW_GATE", 3);
    for (const rsp::LevelSeg &sg : sp.segs) {
        if (sg.thin || sg.c1 == sg.c0) continue;
        CHK(sg.le - sg.lb >= 2 && sg.c0 >= 0 && sg.c1 <= (int)sp.fitems.size(), "%s: flow segment [%d, %d): items [%d, %d)", nm,
            sg.lb, sg.le, sg.c0, sg.c1);
        int it = sg.c0;
        for (int l = sg.lb; l < sg.le; l++) {
            const int b = ptr[(size_t)l], en = ptr[(size_t)l + 1], ns = sp.nshort[(size_t)l], sb = sp.sbase[(size_t)l];
            const int lg = l - gate_d;
            const int gate = gate_d > 0 && lg >= sg.lb && ptr[(size_t)lg + 1] > ptr[(size_t)lg]
                                 ? sp.tasks[(size_t)ptr[(size_t)lg + 1] - 1].i : -1;
            for (int x = b; x < en;) {
                CHK(it < sg.c1, "%s: flow segment [%d, %d): items end before slot %d", nm, sg.lb, sg.le, x);
                const rsp::FlowItem &fi = sp.fitems[(size_t)it++];
                CHK(fi.x0 == x, "%s: flow item %d starts at slot %d, %d wanted", nm, it - 1, fi.x0, x);
                CHK(fi.gate == gate, "%s: flow item %d: gate %d, %d wanted", nm, it - 1, fi.gate, gate);
                if (x - b < ns) {
                    CHK(fi.n >= 1 && fi.n <= 64 && x - b + fi.n <= ns, "%s: flow item %d: %d short rows at %d of %d", nm, it - 1,
                        fi.n, x - b, ns);
                    CHK(fi.t0 == (sb >= 0 ? sb + (x - b) * rsp::kFatLongTerms : -1), "%s: flow item %d: first term %d", nm, it - 1, fi.t0);
                    x += fi.n;
                } else {
                    CHK(fi.n == 0 && fi.t0 == -1, "%s: flow item %d: a wave row with n %d, t0 %d", nm, it - 1, fi.n, fi.t0);
                    x++;
                }
            }
        }
        CHK(it == sg.c1, "%s: flow segment [%d, %d): %d items left over", nm, sg.lb, sg.le, sg.c1 - it);
    }
    return "";
}

struct FacLevel {
    int rm = 0, qm = 0, global_rows = 0;
    long long own = 0;
};
FacLevel fac_level(const IluHostPlan &hp, const hvec<int> &lp, int l) {
    FacLevel f;
    for (int x = lp[(size_t)l]; x < lp[(size_t)l + 1]; x++) {
        const rsp::FacRow &fr = hp.frow[(size_t)x];
        const int nr = fr.re - fr.rs, nq = fr.q1 - fr.q0;
        if (nr <= rsp::kFacRow && nq <= rsp::kFacPairs) {
            f.rm = std::max(f.rm, nr);
            f.qm = std::max(f.qm, nq);
        } else {
            f.global_rows++;
        }
        f.own += (rsp::fac_pairs_at(std::min(nr, rsp::kFacRow)) + 2 * std::min(nq, rsp::kFacPairs) + 3) & ~3;
    }
    return f;
}

std::string check_factor(const int *rp, const IluHostPlan &hp, long long slot_cap) {
    const int n = hp.n;
    if (n == 0 || hp.fac_scale) return "";  // (the one-launch scaling factor has no plan)
    const hvec<int> &lp = hp.fac_one ? hp.F.ptr : hp.L.ptr;
    const hvec<int> &rows = hp.fac_one ? hp.F.rows : hp.L.rows;
    const int nlev = (int)lp.size() - 1, nnz = rp[n];
    const FacPlan &fp = hp.fplan;
    std::vector<char> thin;
    std::string e = seg_levels("factor", fp.segs, nlev, thin);
    if (!e.empty()) return e;
    CHK((int)hp.frow.size() == n && (int)hp.fslev.size() == nlev, "factor: %zu row records, %zu slot levels", hp.frow.size(),
        hp.fslev.size());
    std::vector<int> lev_of_pos((size_t)std::max(nnz, 1), -1);
    for (int l = 0; l < nlev; l++)
        for (int x = lp[(size_t)l]; x < lp[(size_t)l + 1]; x++) {
            const int i = rows[(size_t)x];
            CHK(hp.frow[(size_t)x].i == i && hp.frow[(size_t)x].rs == rp[i] && hp.frow[(size_t)x].re == rp[i + 1],
                "factor: row record %d is not row %d's", x, i);
            for (int p = rp[i]; p < rp[i + 1]; p++) lev_of_pos[(size_t)p] = l;
        }
    // thin runs: every position of their rows is an item of one chunk, once
    std::vector<char> seen((size_t)std::max(nnz, 1), 0);
    for (const rsp::LevelSeg &sg : fp.segs) {
        if (!sg.thin) continue;
        CHK(sg.c0 >= 0 && sg.c1 > sg.c0 && sg.c1 <= (int)fp.chunks.size(), "factor: thin segment [%d, %d): chunks [%d, %d)", sg.lb,
            sg.le, sg.c0, sg.c1);
        long long items = 0, want = 0;
        for (int l = sg.lb; l < sg.le; l++)
            for (int x = lp[(size_t)l]; x < lp[(size_t)l + 1]; x++) want += rp[rows[(size_t)x] + 1] - rp[rows[(size_t)x]];
        for (int c = sg.c0; c < sg.c1; c++) {
            const rsp::RndChunk &ch = fp.chunks[(size_t)c];
            CHK(ch.i0 >= 0 && ch.i1 >= ch.i0 && ch.i1 <= (int)fp.items.size() && ch.p1 >= ch.p0 && ch.p1 <= (int)fp.pairs.size() &&
                    ch.s1 >= ch.s0 && ch.s1 <= (int)fp.staged.size() && ch.r1 >= ch.r0 && ch.r1 <= (int)fp.rounds.size(),
                "factor: chunk %d: ranges outside the plan's arrays", c);
            CHK(ch.i1 - ch.i0 <= rsp::kRndItems && ch.p1 - ch.p0 <= rsp::kRndPairs && ch.s1 - ch.s0 <= rsp::kRndStaged &&
                    ch.r1 - ch.r0 <= rsp::kRndRounds, "factor: chunk %d: %d items %d pairs %d staged %d rounds", c, ch.i1 - ch.i0,
                ch.p1 - ch.p0, ch.s1 - ch.s0, ch.r1 - ch.r0);
            int run = 0;
            for (int q = ch.i0; q < ch.i1; q++) {
                const rsp::RndItem &it = fp.items[(size_t)q];
                CHK(it.pos >= 0 && it.pos < nnz && !seen[(size_t)it.pos] && lev_of_pos[(size_t)it.pos] >= sg.lb &&
                        lev_of_pos[(size_t)it.pos] < sg.le, "factor: chunk %d: item %d (position %d) twice or of another run", c, q, it.pos);
                seen[(size_t)it.pos] = 1;
                const int start = it.u & 0xffff, count = (int)((unsigned)it.u >> 16);
                const int pairs = hp.sym.upd_ptr[(size_t)it.pos + 1] - hp.sym.upd_ptr[(size_t)it.pos];
                CHK(start == run && count == pairs, "factor: item %d: pairs %d + %d, %d + %d wanted", q, start, count, run, pairs);
                run += count;
            }
            CHK(run == ch.p1 - ch.p0, "factor: chunk %d: items hold %d of %d pairs", c, run, ch.p1 - ch.p0);
            items += ch.i1 - ch.i0;
        }
        CHK(items == want, "factor: thin segment [%d, %d): %lld items for %lld positions", sg.lb, sg.le, items, want);
    }
    // slot layout
    std::vector<std::pair<long long, long long>> spans;
    for (int l = 0; l < nlev; l++) {
        const rsp::FacSlotLevel &sl = hp.fslev[(size_t)l];
        if (sl.stride == 0) continue;
        const FacLevel f = fac_level(hp, lp, l);
        const long long cnt = lp[(size_t)l + 1] - lp[(size_t)l];
        CHK(!thin[(size_t)l], "factor: thin level %d in the slot layout", l);
        CHK(sl.rm >= 1 && sl.rm <= rsp::kFacRow && sl.qm >= 1 && sl.qm <= rsp::kFacPairs && sl.rm >= f.rm && sl.qm >= f.qm,
            "factor: slot level %d: rm %d qm %d (rows need %d / %d)", l, sl.rm, sl.qm, f.rm, f.qm);
        CHK(sl.stride >= rsp::fac_pairs_at(sl.rm) + 2 * sl.qm && sl.stride % 4 == 0 && sl.off >= 0 && sl.off % 4 == 0,
            "factor: slot level %d: stride %d at %lld", l, sl.stride, sl.off);
        spans.push_back({sl.off, sl.off + cnt * sl.stride});
    }
    std::sort(spans.begin(), spans.end());
    for (size_t j = 0; j < spans.size(); j++) {
        CHK(j == 0 || spans[j].first >= spans[j - 1].second, "factor: slots overlap at %lld", spans[j].first);
        CHK(spans[j].second <= hp.slot_total, "factor: slots end at %lld, slot_total %lld", spans[j].second, hp.slot_total);
    }
    CHK(hp.slot_total >= 0 && hp.slot_total <= slot_cap, "factor: slot_total %lld past the budget %lld", hp.slot_total, slot_cap);
    // flow runs
    int c_next = 0;
    for (const rsp::FacFlowRun &r : hp.fruns) {
        CHK(r.lb >= 0 && r.le - r.lb >= 2 && r.le <= nlev && r.c0 == c_next && r.c1 - r.c0 == lp[(size_t)r.le] - lp[(size_t)r.lb] &&
                r.c1 <= (int)hp.ffitems.size(), "factor: flow run [%d, %d): items [%d, %d)", r.lb, r.le, r.c0, r.c1);
        c_next = r.c1;
        for (int l = r.lb; l < r.le; l++) {
            const rsp::FacSlotLevel &sl = hp.fslev[(size_t)l];
            CHK(!thin[(size_t)l] && sl.stride > 0 && fac_level(hp, lp, l).global_rows == 0,
                "factor: flow run [%d, %d): level %d is thin, off the slot layout or has global-path rows", r.lb, r.le, l);
            for (int x = lp[(size_t)l]; x < lp[(size_t)l + 1]; x++) {
                const rsp::FacFlowItem &fi = hp.ffitems[(size_t)(r.c0 + x - lp[(size_t)r.lb])];
                CHK((fi.rmqm & 0xffff) == sl.rm && (int)((unsigned)fi.rmqm >> 16) == sl.qm,
                    "factor: flow item of slot %d: rmqm %#x, rm %d qm %d", x, fi.rmqm, sl.rm, sl.qm);
                CHK(fi.off == sl.off + (long long)(x - lp[(size_t)l]) * sl.stride, "factor: flow item of slot %d: offset %lld", x, fi.off);
            }
        }
    }
    return "";
}

void solve_facts(const DagHost &d, long long *f) {
    const SolvePlan &sp = d.sp;
    const hvec<int> &ptr = d.ptr;
    const int nlev = (int)ptr.size() - 1;
    for (int k = 0; k < kFactsPerDag; k++) f[k] = 0;
    if (!d.planned || ptr.empty() || ptr[(size_t)nlev] == 0) return;
    f[0] = nlev;
    f[1] = d.group;
    for (const rsp::LevelSeg &sg : sp.segs) {
        if (!sg.thin) {
            f[sg.c1 > sg.c0 ? 4 : 3]++;
            for (int l = sg.lb; l < sg.le; l++) {
                const int cnt = ptr[(size_t)l + 1] - ptr[(size_t)l];
                f[13] += sp.nshort[(size_t)l];
                f[14] += sp.nwave[(size_t)l] - sp.nshort[(size_t)l];
                f[15] += cnt - sp.nwave[(size_t)l];
                f[19] += sp.sbase[(size_t)l] >= 0;
                f[23]++;
            }
            for (int it = sg.c0; it < sg.c1; it++) {
                const int m = sp.fitems[(size_t)it].n;
                f[m == 64 ? 16 : (m == 0 ? 18 : 17)]++;
                f[21] += m == 1;
                f[24] += sp.fitems[(size_t)it].gate >= 0;
            }
            if (sg.c1 > sg.c0) f[25] = std::max<long long>(f[25], sg.le - sg.lb);
            continue;
        }
        f[2]++;
        f[10] = std::max<long long>(f[10], ptr[(size_t)sg.le] - ptr[(size_t)sg.lb]);
        for (int l = sg.lb; l < sg.le; l++) {
            const int b = ptr[(size_t)l], e = ptr[(size_t)l + 1];
            f[11] += sp.nshort[(size_t)l];
            f[12] += e - b - sp.nshort[(size_t)l];
            f[22]++;
            if (e > b) f[20] = std::max<long long>(f[20], sp.tasks[(size_t)e - 1].t1 - sp.tasks[(size_t)b].t0);
        }
        for (int c = sg.c0; c < sg.c1; c++) {
            const rsp::LevelChunk &ch = sp.chunks[(size_t)c];
            f[5]++;
            f[6] = std::max<long long>(f[6], ch.x1 - ch.x0);
            f[7] = std::max<long long>(f[7], ch.k1 - ch.k0);
            f[8] += ch.st1 - ch.st0;
            for (int k = ch.k0; k < ch.k1; k++) f[9] += sp.src[(size_t)k] < 0 && sp.src[(size_t)k] != rsp::kPadSrc;
        }
    }
}

}  // namespace

std::string check_plans(const int *rp, const int *ci, const IluHostPlan &hp, long long slot_cap) {
    const int n = hp.n;
    const DagView views[3] = {
        {"L", &hp.L,
         [&](int i, TermList &tv) {
             tv.clear();
             for (int o = rp[i]; o < hp.dpos[(size_t)i]; o++) {
                 const int p = hp.lpos.empty() ? o : hp.lpos[(size_t)o];
                 tv.push_back({p, ci[p]});
             }
         },
         [&](int i) { return hp.ne_l.empty() ? 0 : hp.ne_l[(size_t)i]; }, [](int) { return -1; }},
        {"LT", &hp.LT,
         [&](int i, TermList &tv) {
             tv.clear();
             for (int q = hp.ltp[(size_t)i]; q < hp.ltp[(size_t)i + 1]; q++) tv.push_back({hp.lts[(size_t)q], hp.ltc[(size_t)q]});
         },
         [&](int i) { return hp.ne_lt.empty() ? 0 : hp.ne_lt[(size_t)i]; }, [](int) { return -1; }},
        {"U", &hp.U,
         [&](int i, TermList &tv) {
             tv.clear();
             for (int p = hp.dpos[(size_t)i] + hp.hasdiag[(size_t)i]; p < rp[i + 1]; p++) tv.push_back({p, ci[p]});
         },
         [](int) { return 0; }, [&](int i) { return hp.hasdiag[(size_t)i] ? hp.dpos[(size_t)i] : -1; }}};
    for (const DagView &v : views) {
        if (v.d == &hp.U && !hp.U.planned) continue;
        // (L's terms: positions ascending, columns < the row; L^T's: rows that hold the
        // column, descending; U's: columns > the row — what rsp_trsv_* define)
        std::string e = check_solve(n, v);
        if (!e.empty()) return e;
    }
    return check_factor(rp, hp, slot_cap);
}

void plan_facts(const int *rp, const IluHostPlan &hp, long long slot_cap, long long *f) {
    solve_facts(hp.L, f);
    solve_facts(hp.LT, f + kFactsPerDag);
    solve_facts(hp.U, f + 2 * kFactsPerDag);
    long long *q = f + 3 * kFactsPerDag;
    for (int k = 0; k < kFactsFactor; k++) q[k] = 0;
    q[0] = hp.fac_one;
    q[1] = hp.fac_scale;
    if (hp.n == 0 || hp.fac_scale) return;
    const hvec<int> &lp = hp.fac_one ? hp.F.ptr : hp.L.ptr;
    const hvec<int> &rows = hp.fac_one ? hp.F.rows : hp.L.rows;
    const int nlev = (int)lp.size() - 1;
    const long long pad_ratio = std::max(1, env_int("RSP_ILU_SLOT_PAD", 2));
    q[19] = nlev;
    q[21] = -1;
    long long budget_used = 0;  // as the planner walks the levels in order
    for (const rsp::LevelSeg &sg : hp.fplan.segs) {
        for (int l = sg.lb; l < sg.le; l++) {
            long long pos = 0;
            int maxp = 0;
            for (int x = lp[(size_t)l]; x < lp[(size_t)l + 1]; x++) {
                const int i = rows[(size_t)x];
                pos += rp[i + 1] - rp[i];
                for (int p = rp[i]; p < rp[i + 1]; p++)
                    maxp = std::max(maxp, hp.sym.upd_ptr[(size_t)p + 1] - hp.sym.upd_ptr[(size_t)p]);
            }
            const FacLevel fl = fac_level(hp, lp, l);
            if (sg.thin) {
                q[22]++;
                q[24] += fl.global_rows > 0;
                q[25] = std::max<long long>(q[25], lp[(size_t)l + 1] - lp[(size_t)l]);
                q[15] = std::max<long long>(q[15], maxp);
                q[20] = std::max(q[20], pos);
                continue;
            }
            q[3]++;
            q[7] += fl.global_rows;
            q[21] =q[21] < 0 ? pos : std::min(q[21], pos);
            q[23] += fl.global_rows > 0;
            const rsp::FacSlotLevel &sl = hp.fslev[(size_t)l];
            const long long cnt = lp[(size_t)l + 1] - lp[(size_t)l];
            q[16] = std::max<long long>(q[16], fl.rm);
            q[17] = std::max<long long>(q[17], fl.qm);
            if (sl.stride > 0) {
                q[4]++;
                budget_used += cnt * sl.stride;
            } else if (fl.rm > 0) {
                const int stride = (rsp::fac_pairs_at(fl.rm) + 2 * std::max(fl.qm, 1) + 3) & ~3;
                if (cnt * stride > pad_ratio * fl.own) q[5]++;
                else if (budget_used + cnt * stride > slot_cap) q[6]++;
            }
        }
        if (!sg.thin) continue;
        q[2]++;
        for (int c = sg.c0; c < sg.c1; c++) {
            const rsp::RndChunk &ch = hp.fplan.chunks[(size_t)c];
            q[10]++;
            q[11] = std::max<long long>(q[11], ch.i1 - ch.i0);
            q[12] = std::max<long long>(q[12], ch.p1 - ch.p0);
            q[13] = std::max<long long>(q[13], ch.s1 - ch.s0);
            q[14] = std::max<long long>(q[14], ch.r1 - ch.r0);
        }
    }
    if (q[21] < 0) q[21] = 0;
    q[8] = (long long)hp.fruns.size();
    for (const rsp::FacFlowRun &r : hp.fruns) q[9] += r.le - r.lb;
    q[18] = hp.slot_total;
}

}  // namespace rsp_an
