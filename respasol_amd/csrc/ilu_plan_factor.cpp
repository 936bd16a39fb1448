// ilu_plan_factor.cpp — the factor plan of the ILU(0) host analysis (see
// ilu_analysis.h): which levels run thin, the thin runs' rounds, the FacRow
// records, the fat levels' slot layout and the flow runs. No HIP calls here.

#include "ilu_analysis.h"

#include <stdio.h>

#include <algorithm>

namespace rsp_an {

// Which levels of the L DAG the factor runs thin. A level runs thin up to
// kRndFlowItems positions; up to kRndLevelItems when it could not run in a
// flow launch anyway (a row past the slot layout's kFacRow entries /
// kFacPairs pairs: circuit hubs); and never with a position of more than
// kRndItemPairs update pairs. Wider levels are fat: in a flow run they
// spread over all CUs, where a thin run stages every position through one
// (A/B knobs RSP_ILU_THIN_FACTOR_ITEMS / RSP_ILU_THIN_FACTOR_FLOW).
static hvec<char> factor_thin_levels(const int *rp, const hvec<int> &upd_ptr,
                                            const hvec<int> &ptr, const hvec<int> &rows,
                                            int thin_rows, hvec<long long> *items_out) {
    const int nlev = (int)ptr.size() - 1;
    const int thin_items = env_int("RSP_ILU_THIN_FACTOR_ITEMS", rsp::kRndLevelItems);
    const int thin_flow = env_int("RSP_ILU_THIN_FACTOR_FLOW", rsp::kRndFlowItems);
    hvec<long long> litems((size_t)std::max(nlev, 1), 0);
    hvec<char> thin((size_t)std::max(nlev, 1), 0);
    pfor_dyn(nlev, (long long)rows.size(), 1 << 14, [&](int l) {
        long long items = 0;
        int maxp = 0;
        bool hub = false;
        for (int x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; x++) {
            const int i = rows[(size_t)x], rs = rp[(size_t)i], re = rp[(size_t)i + 1];
            items += re - rs;
            for (int p = rs; p < re; p++) maxp = std::max(maxp, upd_ptr[(size_t)p + 1] - upd_ptr[(size_t)p]);
            hub |= re - rs > rsp::kFacRow || upd_ptr[(size_t)re] - upd_ptr[(size_t)rs] > rsp::kFacPairs;
        }
        litems[(size_t)l] = items;
        const int cnt = ptr[(size_t)l + 1] - ptr[(size_t)l];
        const long long lim = hub ? thin_items : std::min(thin_items, thin_flow);
        thin[(size_t)l] = (cnt <= thin_rows && items <= lim && maxp <= rsp::kRndItemPairs) ? 1 : 0;
    });
    if (items_out) items_out->swap(litems);
    return thin;
}

// RSP_ILU_THIN_FACTOR: tuning knob (0 = no thin runs)
static int thin_factor_rows() { return env_int("RSP_ILU_THIN_FACTOR", rsp::kThinFactorRows); }

hvec<int> factor_thin_rows(const int *rp, const IluHostPlan &hp) {
    const hvec<char> thin = factor_thin_levels(rp, hp.sym.upd_ptr, hp.L.ptr, hp.L.rows, thin_factor_rows(),
                                                      nullptr);
    hvec<int> out;
    for (size_t l = 0; l + 1 < hp.L.ptr.size(); l++)
        if (thin[l])
            for (int x = hp.L.ptr[l]; x < hp.L.ptr[l + 1]; x++) out.push_back(hp.L.rows[(size_t)x]);
    return out;
}

// Factor plan of the L DAG (see IluArgs): segments (fat levels: one launch
// each; thin levels: one single-workgroup launch per run) and, for the thin
// runs, ROUNDS: a level's positions ("items") grouped so that a round's items
// are independent — a lower item of intra-row stage s is in round s, a row's
// upper items (diagonal included) in the round after its last lower stage.
// Every item depends only on earlier rounds (its own row's l_ik) and earlier
// levels (u_kj, u_kk). The run's items, in round order, are cut into LDS
// chunks (<= kRndItems items, kRndPairs update pairs, kRndStaged staged
// values, kRndRounds rounds; a round may be split between chunks). An item's
// operands are indices into the kernel's LDS value buffer by class: its own
// chunk's slots, the previous chunk's slots (kept in the other LDS buffer),
// values staged from vals at the chunk start (producers two or more chunks
// back, or before the run), or the zero slot (a missing u_kk).
//
// Built in parallel. A thin segment is cut at level boundaries into pieces
// of about RSP_ILU_PIECE_ITEMS positions (default kRndPieceItems); each
// piece is planned on its own (greedily, as above) and the pieces are joined
// in order with an EMPTY chunk between two pieces of a segment: ilu0_rounds issues a chunk's gathers at
// the previous chunk's switch, so the empty chunk's switch is where the
// earlier piece's last stores are complete before the next piece stages them
// (a piece sees every value before it as staged). Per position, where[] holds
// the chunk key (piece + 1, chunk within the piece) and slot it was placed at:
// keys are unique over the whole plan, so a piece reading a position another
// piece is writing concurrently (never its own chunk or the one before) only
// ever gets "not here" — the relaxed atomics make those reads well defined.
// The staged positions of the current chunk sit in a piece-private hash.
static constexpr int kRndPieceItems = 1 << 16;  // the largest piece (round 4 A/B: 2^17 / 2^16 / 2^15 gave factor 58.58 / 58.58 / 58.73 ms); see build_factor_plan

static void build_factor_plan(int n, const int *rp, const int *ci,
                              const hvec<int> &dpos, const hvec<int> &hasdiag,
                              const IluSymbolic &sym, const hvec<int> &ptr,
                              const hvec<int> &rows, int thin_rows, FacPlan &fp) {
    const int nlev = (int)ptr.size() - 1;
    const int K = rsp::kRndItems, S = rsp::kRndStaged, kZero = 2 * rsp::kRndItems + rsp::kRndStaged;
    const int nnz = rp[(size_t)n];
    const double t0 = now_ms();
    hvec<long long> litems;
    const hvec<char> lthin = factor_thin_levels(rp, sym.upd_ptr, ptr, rows, thin_rows, &litems);
    const double t_thin = now_ms() - t0;
    // piece size: about 1/32 of the thin positions, within [2^15, 2^16] — a
    // function of the pattern only, so the plan is the same on every host
    // (round 5: a fixed 2^16 left the circuits' 7-13 pieces, ~120 ns per
    // position each, as the analysis' longest step; each extra piece adds an
    // empty chunk to the factor, ~1.5 us: a 2^14 floor gave config-3 analysis
    // -15 ms for +0.6 % on the circuits' factor, profiles/r05_piece_ab.txt)
    long long thin_total = 0;
    for (int l = 0; l < nlev; l++)
        if (lthin[(size_t)l]) thin_total += litems[(size_t)l];
    const long long piece_items = std::max(
        1LL, (long long)env_int("RSP_ILU_PIECE_ITEMS",
                                (int)std::min<long long>(kRndPieceItems, std::max<long long>(1 << 15, thin_total / 32))));
    // pairs of position p of thin row i (packed, see IluSymbolic::pair_base)
    auto pair_off = [&](int i) {
        return sym.pair_base.empty() ? 0 : sym.pair_base[(size_t)i] - sym.upd_ptr[(size_t)rp[(size_t)i]];
    };
    fp.segs.clear();
    for (int l = 0; l < nlev; l++) {
        const int thin = lthin[(size_t)l];
        if (!fp.segs.empty() && fp.segs.back().thin == thin && fp.segs.back().le == l)
            fp.segs.back().le = l + 1;
        else
            fp.segs.push_back({l, l + 1, thin, 0, 0, rsp::kThinThreads});
    }
    struct Piece {
        int seg, lb, le;
        FacPlan out;  // chunk records relative to the piece's own arrays
    };
    hvec<Piece> pieces;
    for (int s = 0; s < (int)fp.segs.size(); s++) {
        const rsp::LevelSeg &sg = fp.segs[(size_t)s];
        if (!sg.thin) continue;
        long long acc = 0;
        int lb = sg.lb;
        for (int l = sg.lb; l < sg.le; l++) {
            acc += litems[(size_t)l];
            if (acc >= piece_items && l + 1 < sg.le) {
                pieces.push_back({s, lb, l + 1, FacPlan()});
                lb = l + 1;
                acc = 0;
            }
        }
        pieces.push_back({s, lb, sg.le, FacPlan()});
    }
    hvec<unsigned long long> where((size_t)std::max(nnz, 1), 0ull);
    const double t_where = now_ms() - t0;
    auto wload = [&](int q) { return __atomic_load_n(&where[(size_t)q], __ATOMIC_RELAXED); };
    pfor_dyn((int)pieces.size(), nnz, 1 << 15, [&](int pi) {
        Piece &pc = pieces[(size_t)pi];
        FacPlan &o = pc.out;
        // staged positions of the current chunk: open addressing, epoch-stamped
        constexpr int kH = 4 * rsp::kRndStaged;
        hvec<int> hkey(kH), hval(kH), hep(kH, 0);
        int epoch = 0, nstg = 0;
        auto hslot = [&](int q) { return (int)(((unsigned)q * 2654435761u) >> 18) & (kH - 1); };
        auto hfind = [&](int q) {
            for (int h = hslot(q);; h = (h + 1) & (kH - 1)) {
                if (hep[(size_t)h] != epoch) return -1;
                if (hkey[(size_t)h] == q) return hval[(size_t)h];
            }
        };
        auto hput = [&](int q, int v) {
            int h = hslot(q);
            while (hep[(size_t)h] == epoch) h = (h + 1) & (kH - 1);
            hep[(size_t)h] = epoch;
            hkey[(size_t)h] = q;
            hval[(size_t)h] = v;
        };
        const unsigned long long pkey = (unsigned long long)(pi + 1) << 28;
        int c = -1;  // chunk within the piece
        unsigned long long ckey = 0;
        rsp::RndChunk ch{};
        auto open_chunk = [&]() {
            epoch++;
            nstg = 0;
            c = (int)o.chunks.size();
            ckey = pkey | (unsigned long long)c;
            ch = rsp::RndChunk{(int)o.items.size(), (int)o.items.size(), (int)o.pairs.size(), (int)o.pairs.size(),
                               (int)o.staged.size(), (int)o.staged.size(), (int)o.rounds.size(), (int)o.rounds.size()};
            o.chunks.push_back(ch);
        };
        auto close_chunk = [&]() {
            ch.i1 = (int)o.items.size();
            ch.p1 = (int)o.pairs.size();
            ch.s1 = (int)o.staged.size();
            ch.r1 = (int)o.rounds.size();
            o.chunks[(size_t)c] = ch;
        };
        // this item's not-yet-staged operands (fresh), looked up by a second
        // epoch-stamped hash: an item of a hub row has up to kRndItemPairs
        // pairs, and a linear search of its fresh list was quadratic in them
        constexpr int kF = 4 * rsp::kRndItemPairs;  // >= 2 x the 2 kRndItemPairs operands
        hvec<int> fkey(kF), fval(kF), fep(kF, 0);
        int fepoch = 0;
        // first slot of the item's round in its chunk: a position placed at
        // or after it is computed in the same round, so it is no operand
        // slot. Only a one-level factor (IluHostPlan::fac_one) reads such a
        // position — a u_kk of a row without lower entries, final from the
        // start — and stages its input instead; in an L-level plan every
        // operand lies in an earlier round, so this never triggers there.
        int rstart = 0;
        auto ref = [&](int q, hvec<int> &fresh) {
            const unsigned long long w = wload(q), wk = w >> 12;
            if (wk == ckey && (int)(w & 0xfff) < rstart) return (int)(w & 0xfff);
            if (c > 0 && wk == ckey - 1) return K + (int)(w & 0xfff);
            const int st = hfind(q);
            if (st >= 0) return 2 * K + st;
            int h = (int)(((unsigned)q * 2654435761u) >> 20) & (kF - 1);
            for (; fep[(size_t)h] == fepoch; h = (h + 1) & (kF - 1))
                if (fkey[(size_t)h] == q) return 2 * K + (int)(nstg + fval[(size_t)h]);
            fep[(size_t)h] = fepoch;
            fkey[(size_t)h] = q;
            fval[(size_t)h] = (int)fresh.size();
            fresh.push_back(q);
            return 2 * K + (int)(nstg + fresh.size() - 1);
        };
        struct RItem {
            int round, pos, row;
        };
        hvec<RItem> ritems, rsorted;
        hvec<int> rcount, fresh, ipairs;
        open_chunk();
        long long last_round_key = -1;
        int last_round_level = -1;  // level of the chunk's last round (-1: none yet)
        for (int l = pc.lb; l < pc.le; l++) {
            ritems.clear();
            for (int x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; x++) {
                const int i = rows[(size_t)x], rs = rp[(size_t)i], di = dpos[(size_t)i];
                int nst = 0;
                for (int p = rs; p < di; p++) {
                    ritems.push_back({sym.stage[(size_t)p], p, i});
                    nst = std::max(nst, sym.stage[(size_t)p] + 1);
                }
                for (int p = di; p < rp[(size_t)i + 1]; p++) ritems.push_back({nst, p, i});
            }
            {  // stable counting sort by round
                int rmax = 0;
                for (const RItem &ri : ritems) rmax = std::max(rmax, ri.round);
                rcount.assign((size_t)rmax + 2, 0);
                for (const RItem &ri : ritems) rcount[(size_t)ri.round + 1]++;
                for (int r = 0; r <= rmax; r++) rcount[(size_t)r + 1] += rcount[(size_t)r];
                rsorted.resize(ritems.size());
                for (const RItem &ri : ritems) rsorted[(size_t)rcount[(size_t)ri.round]++] = ri;
                ritems.swap(rsorted);
            }
            for (const RItem &ri : ritems) {
                const int p = ri.pos, i = ri.row;
                const long long key = (long long)(l - pc.lb) * 1000000007LL + ri.round;
                const bool lower = p < dpos[(size_t)i];
                for (int attempt = 0; attempt < 2; attempt++) {
                    fresh.clear();
                    fepoch++;
                    ipairs.clear();
                    rstart = key != last_round_key ? (int)o.items.size() - ch.i0
                                                   : (o.rounds.back() & ~rsp::kRndLevelStart);
                    const int po = pair_off(i);
                    for (int u = sym.upd_ptr[(size_t)p]; u < sym.upd_ptr[(size_t)p + 1]; u++) {
                        const int lc = ref(sym.upd_l[(size_t)(u + po)], fresh), uc = ref(sym.upd_u[(size_t)(u + po)], fresh);
                        ipairs.push_back(lc | uc << 16);
                    }
                    int d = -1;
                    if (lower) {
                        const int k = ci[(size_t)p];
                        d = hasdiag[(size_t)k] ? ref(dpos[(size_t)k], fresh) : kZero;
                    }
                    const int slot = (int)o.items.size() - ch.i0;
                    const bool new_round = key != last_round_key;
                    const bool fits = slot < K && (int)(o.pairs.size() - ch.p0 + ipairs.size()) <= rsp::kRndPairs &&
                                      nstg + (int)fresh.size() <= S &&
                                      (int)(o.rounds.size() - ch.r0) + (new_round ? 1 : 0) <= rsp::kRndRounds;
                    if (!fits && attempt == 0 && slot > 0) {
                        close_chunk();
                        open_chunk();
                        last_round_key = -1;
                        last_round_level = -1;
                        continue;
                    }
                    for (int q : fresh) {
                        hput(q, nstg++);
                        o.staged.push_back(q);
                    }
                    if (new_round) {  // flagged where it opens a level in this chunk
                        o.rounds.push_back(slot | (l != last_round_level ? rsp::kRndLevelStart : 0));
                        last_round_key = key;
                        last_round_level = l;
                    }
                    const int pstart = (int)o.pairs.size() - ch.p0;
                    o.pairs.insert(o.pairs.end(), ipairs.begin(), ipairs.end());
                    const int zr = (!lower && p == dpos[(size_t)i] && hasdiag[(size_t)i]) ? i : -1;
                    o.items.push_back({p, pstart | (int)ipairs.size() << 16, d, zr});
                    __atomic_store_n(&where[(size_t)p], ckey << 12 | (unsigned long long)slot, __ATOMIC_RELAXED);
                    break;
                }
            }
        }
        close_chunk();
    });
    const double t_pieces = now_ms() - t0;
    // join: pieces in order, an empty chunk between two pieces of a segment
    fp.chunks.clear();
    fp.items.clear();
    fp.pairs.clear();
    fp.staged.clear();
    fp.rounds.clear();
    size_t ni = 0, np = 0, ns = 0, nr = 0, nc = 0;
    for (const Piece &pc : pieces) {
        ni += pc.out.items.size();
        np += pc.out.pairs.size();
        ns += pc.out.staged.size();
        nr += pc.out.rounds.size();
        nc += pc.out.chunks.size() + 1;
    }
    fp.items.reserve(ni);
    fp.pairs.reserve(np);
    fp.staged.reserve(ns);
    fp.rounds.reserve(nr);
    fp.chunks.reserve(nc);
    for (size_t q = 0; q < pieces.size(); q++) {
        const Piece &pc = pieces[q];
        rsp::LevelSeg &sg = fp.segs[(size_t)pc.seg];
        const int bi = (int)fp.items.size(), bp = (int)fp.pairs.size(), bs = (int)fp.staged.size(),
                  br = (int)fp.rounds.size();
        if (q == 0 || pieces[q - 1].seg != pc.seg)
            sg.c0 = (int)fp.chunks.size();
        else
            fp.chunks.push_back(rsp::RndChunk{bi, bi, bp, bp, bs, bs, br, br});  // the separator
        for (rsp::RndChunk r : pc.out.chunks) {
            r.i0 += bi, r.i1 += bi, r.p0 += bp, r.p1 += bp, r.s0 += bs, r.s1 += bs, r.r0 += br, r.r1 += br;
            fp.chunks.push_back(r);
        }
        fp.items.insert(fp.items.end(), pc.out.items.begin(), pc.out.items.end());
        fp.pairs.insert(fp.pairs.end(), pc.out.pairs.begin(), pc.out.pairs.end());
        fp.staged.insert(fp.staged.end(), pc.out.staged.begin(), pc.out.staged.end());
        fp.rounds.insert(fp.rounds.end(), pc.out.rounds.begin(), pc.out.rounds.end());
        sg.c1 = (int)fp.chunks.size();
    }
    if (fp.items.empty()) fp.items.push_back({0, 0, -1, -1});
    for (hvec<int> *v : {&fp.pairs, &fp.staged, &fp.rounds})
        if (v->empty()) v->push_back(0);
    if (fp.chunks.empty()) fp.chunks.push_back(rsp::RndChunk{});
    if (env_int("RSP_ILU_TIMING", 0) >= 3)
        fprintf(stderr, "rsp_ilu0_analysis n=%d     factor plan: thin levels %.2f where %.2f pieces (%zu) %.2f join %.2f ms\n",
                n, t_thin, t_where, pieces.size(), t_pieces, now_ms() - t0);
}

void plan_factor(const int *rp, const int *ci, long long slot_cap, IluHostPlan &hp) {
    const int n = hp.n, nnz_s = hp.nnz_s;
    const hvec<int> &dpos = hp.dpos, &hasdiag = hp.hasdiag;
    const int thin_factor = thin_factor_rows();
    IluSymbolic &sym = hp.sym;
    hp.fac_batch = chain_batch((long long)sym.upd_ptr[(size_t)nnz_s], nnz_s);
    // No update pairs at all (a stored lower triangle): the factor is
    // l_ik = a_ik / a_kk for every lower position and nothing else, and the
    // a_kk are never written with other bits, so every row goes in ONE level
    // (IluHostPlan::F) instead of the L DAG's — for G2_circuit 5 799 levels.
    // The positions' arithmetic is unchanged (same division, same operands):
    // same bits. In that level a row may read a u_kk that the row k's own
    // work item rewrites concurrently with identical bits (fat kernels) or
    // that a thin run has not placed yet (its rounds are in order: lower
    // items in round 0, a row's diagonal in round 1, so a round-0 item finds
    // the divisor "not here" and stages the input). No flow run (one level).
    // RSP_ILU_FAC_ONE=0 keeps L's levels (A/B).
    hp.fac_one = n > 0 && sym.upd_ptr[(size_t)nnz_s] == 0 && env_int("RSP_ILU_FAC_ONE", 1) != 0;
    if (hp.fac_one) {
        hp.F.ptr = hvec<int>{0, n};
        hp.F.rows.resize((size_t)n);
        pfor(n, 1 << 16, [&](long long a, long long b) {
            for (long long x = a; x < b; x++) hp.F.rows[(size_t)x] = (int)x;
        });
    } else {
        hp.F = DagHost();
    }
    hp.fac_scale = hp.fac_one && env_int("RSP_ILU_FAC_SCALE", 1) != 0;
    if (hp.fac_scale) {  // ilu0_scale_lower needs no plan
        hp.fplan = FacPlan();
        hp.frow.assign(1, rsp::FacRow{});
        hp.fslev.clear();
        hp.slot_desc.clear();
        hp.slot_offs.clear();
        hp.slot_total = 0;
        hp.fruns.clear();
        hp.ffitems.assign(1, rsp::FacFlowItem{0, 0, -1});
        return;
    }
    const hvec<int> &lp = hp.fac_one ? hp.F.ptr : hp.L.ptr;
    const hvec<int> &rows_l = hp.fac_one ? hp.F.rows : hp.L.rows;
    timed_plan(n, "factor", [&] {
        build_factor_plan(n, rp, ci, dpos, hasdiag, sym, lp, rows_l, thin_factor, hp.fplan);
    });
    const long long nx = (long long)rows_l.size();
    hp.frow.assign(std::max<size_t>(rows_l.size(), 1), rsp::FacRow{});
    pfor(nx, 1 << 14, [&](long long a, long long b) {
        for (long long x = a; x < b; x++) {
            const int i = rows_l[(size_t)x], rs = rp[(size_t)i], re = rp[(size_t)i + 1];
            hp.frow[(size_t)x] = rsp::FacRow{i, rs, dpos[(size_t)i], re, sym.upd_ptr[(size_t)rs],
                                             sym.upd_ptr[(size_t)re], hasdiag[(size_t)i], 0};
        }
    });
    // fat factor levels in the slot layout (rsp::FacSlotLevel): each row's
    // structure at a fixed stride, so ilu0_level_slot reads it in one round
    // trip. A level whose padded slots would take more than twice its rows'
    // own structure (one large row among many small ones), or past the
    // budget, keeps the FacRow path. Per level (parallel): the largest
    // LDS-path row and pair count, the rows' own structure size, whether
    // every row fits the LDS path (flow runs); then the offsets in order.
    const int nlev = (int)lp.size() - 1;
    hp.fslev.assign((size_t)std::max(nlev, 0), rsp::FacSlotLevel{0, 0, 0, 0, 0});
    struct LevStat {
        int rm, qm, all_lds, fat;
        long long own;
    };
    hvec<LevStat> ls((size_t)std::max(nlev, 1), LevStat{0, 0, 0, 0, 0});
    for (const rsp::LevelSeg &sg : hp.fplan.segs)
        if (!sg.thin)
            for (int l = sg.lb; l < sg.le; l++) ls[(size_t)l].fat = 1;
    pfor_dyn(nlev, nx, 1 << 14, [&](int l) {
        LevStat &st = ls[(size_t)l];
        if (!st.fat) return;
        st.all_lds = 1;
        for (int x = lp[(size_t)l]; x < lp[(size_t)l + 1]; x++) {
            const rsp::FacRow &fr = hp.frow[(size_t)x];
            const int nr = fr.re - fr.rs, nq = fr.q1 - fr.q0;
            if (nr <= rsp::kFacRow && nq <= rsp::kFacPairs) {
                st.rm = std::max(st.rm, nr);
                st.qm = std::max(st.qm, nq);
            } else {
                st.all_lds = 0;
            }
            st.own += (rsp::fac_pairs_at(std::min(nr, rsp::kFacRow)) + 2 * std::min(nq, rsp::kFacPairs) + 3) & ~3;
        }
    });
    long long total = 0;
    hvec<int> slot_levels;
    // RSP_ILU_SLOT_PAD: A/B knob, the padded size a level may take over its
    // rows' own structure (2 / 4 / 16: config-3 fp64 factor 58.6 / 58.7 /
    // 58.6 ms; the ~280 single fat levels per run left on the FacRow path
    // are hub-row levels, not padding-dominated ones)
    const long long pad_ratio = std::max(1, env_int("RSP_ILU_SLOT_PAD", 2));
    for (int l = 0; l < nlev; l++) {
        const LevStat &st = ls[(size_t)l];
        if (!st.fat || st.rm == 0) continue;
        // a level without update pairs keeps one (padding) pair slot per row:
        // the kernels' pair loads are clamped to the level's qm - 1
        const int qm = std::max(st.qm, 1);
        const int stride = (rsp::fac_pairs_at(st.rm) + 2 * qm + 3) & ~3;
        const long long cnt = lp[(size_t)l + 1] - lp[(size_t)l];
        if (cnt * stride > pad_ratio * st.own) continue;  // padding would dominate
        if (total + cnt * stride > slot_cap) continue;
        hp.fslev[(size_t)l] = rsp::FacSlotLevel{total, stride, st.rm, qm, 0};
        total += cnt * stride;
        slot_levels.push_back(l);
    }
    hp.slot_total = total;
    // flow runs: maximal runs of >= 2 slot-layout fat levels without
    // global-path rows; items in level order, gated like the solve's
    hp.fruns.clear();
    hp.ffitems.clear();
    if (env_int("RSP_ILU_FLOW_PLAN", 1) != 0) {
        const int gate_d = env_int("RSP_ILU_FLOW_GATE", 3);
        auto flowable = [&](int l) { return hp.fslev[(size_t)l].stride > 0 && ls[(size_t)l].all_lds; };
        for (const rsp::LevelSeg &sg : hp.fplan.segs) {
            if (sg.thin) continue;
            for (int l = sg.lb; l < sg.le;) {
                if (!flowable(l)) {
                    l++;
                    continue;
                }
                int e = l + 1;
                while (e < sg.le && flowable(e)) e++;
                if (e - l >= 2) {
                    const int c0 = hp.fruns.empty() ? 0 : hp.fruns.back().c1;
                    hp.fruns.push_back(rsp::FacFlowRun{l, e, c0, c0 + lp[(size_t)e] - lp[(size_t)l]});
                }
                l = e;
            }
        }
        hp.ffitems.resize(hp.fruns.empty() ? 0 : (size_t)hp.fruns.back().c1);
        for (const rsp::FacFlowRun &r : hp.fruns)
            pfor_dyn(r.le - r.lb, lp[(size_t)r.le] - lp[(size_t)r.lb], 1 << 14, [&](int j) {
                const int v = r.lb + j;
                const rsp::FacSlotLevel &sl = hp.fslev[(size_t)v];
                const int lg = v - gate_d;
                const int gate = gate_d > 0 && lg >= r.lb && lp[(size_t)lg + 1] > lp[(size_t)lg]
                                     ? rows_l[(size_t)lp[(size_t)lg + 1] - 1] : -1;
                for (int x = lp[(size_t)v]; x < lp[(size_t)v + 1]; x++)
                    hp.ffitems[(size_t)(r.c0 + x - lp[(size_t)r.lb])] =
                        rsp::FacFlowItem{sl.off + (long long)(x - lp[(size_t)v]) * sl.stride, sl.rm | sl.qm << 16, gate};
            });
    }
    if (hp.ffitems.empty()) hp.ffitems.push_back({0, 0, -1});  // keep the device array non-empty
    hvec<long long> sd0(slot_levels.size() + 1, 0);
    for (size_t j = 0; j < slot_levels.size(); j++)
        sd0[j + 1] = sd0[j] + lp[(size_t)slot_levels[j] + 1] - lp[(size_t)slot_levels[j]];
    hp.slot_desc.resize((size_t)sd0.back());
    hp.slot_offs.resize((size_t)sd0.back());
    pfor_dyn((int)slot_levels.size(), sd0.back(), 1 << 14, [&](int j) {
        const int l = slot_levels[(size_t)j];
        const rsp::FacSlotLevel &sl = hp.fslev[(size_t)l];
        for (int x = lp[(size_t)l]; x < lp[(size_t)l + 1]; x++) {
            const size_t o = (size_t)(sd0[(size_t)j] + x - lp[(size_t)l]);
            hp.slot_desc[o] = int4{x, sl.rm, sl.qm, 0};
            hp.slot_offs[o] = sl.off + (long long)(x - lp[(size_t)l]) * sl.stride;
        }
    });
}

}  // namespace rsp_an
