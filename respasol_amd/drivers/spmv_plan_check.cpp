// spmv_plan_check.cpp — stand-alone check of the SpMV planner (spmv_plan.h;
// never shipped): for fp64 and fp32 and for the default options, each
// non-default option alone and the split schedule together with spreading, it
// builds the plan of a pattern twice (the planner is parallel: the two digests
// must agree) and verifies it with rsp_plan::plan_verify. One line per plan:
// name, type, options, tiles, 16-bit entries, staged entries, packed tiles,
// digest. Exit 0 = every plan verified. The plan-time knobs (RSP_SPMV_PACK,
// RSP_SPMV_STAGE_LIST, RSP_SPMV_STAGE_PCT, RSP_SPMV_LIST_CAP) come from the
// environment as everywhere else. Built by `make -C respasol_amd/csrc
// tsan-plan` (ThreadSanitizer) and `asan-plan` (Address +
// UndefinedBehaviorSanitizer); tests/test_sanitize.py runs both.
//     spmv_plan_check <surrogate> [scale]
//     spmv_plan_check @<file> <name>    a pattern as int32 {rows, cols, rowptr[rows + 1], colidx[nnz]}
//                                       (scripts/spmv_plan_digest.py writes it)
//     spmv_plan_check --mutate <either form>
// --mutate: the verifier must reject what it claims to check. For fp64 and
// fp32, the default plan of the pattern (and its split plan, for the interior
// count) is corrupted in one place at a time (kMutants below) and plan_verify
// must return false for each; a corruption whose field the plan does not have
// is reported as absent. One line per type: the corruptions applied (all
// rejected), then the absent ones. Exit 5 = a corrupted plan verified.
#include "spmv_plan.h"
#include "rsp_host.h"
#include "spmv_pack.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

static bool read_pattern(const char *path, int *m, int *cols, std::vector<int> &rp, std::vector<int> &ci) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int hdr[2] = {0, 0};
    bool ok = fread(hdr, sizeof(int), 2, f) == 2 && hdr[0] >= 0 && hdr[1] >= 0;
    if (ok) {
        rp.assign((size_t)hdr[0] + 1, 0);
        ok = fread(rp.data(), sizeof(int), rp.size(), f) == rp.size() && rp[0] == 0 && rp.back() >= 0;
    }
    if (ok) {
        ci.resize((size_t)rp.back());
        ok = fread(ci.data(), sizeof(int), ci.size(), f) == ci.size();
    }
    fclose(f);
    *m = hdr[0];
    *cols = hdr[1];
    return ok;
}

namespace {

using rsp_plan::PlanOptions;
using rsp_plan::TilePlan;

const char *const kMutants[] = {"c16", "cbase", "run-col", "run-slot", "sentinel", "slot-swap", "list-ofs",
                                "list-u", "pack-pad", "pack-field", "pack-row", "poff", "nint", "tile-swap"};
constexpr int kNumMutants = (int)(sizeof(kMutants) / sizeof(kMutants[0]));

struct Geo {
    int vw, iw, nwt, fields;
};
Geo geo_of(rsp_datatype_t t) {
    const int vw = t == RSP_R_64F ? 2 : 4, fields = rsp::kSpmvIter * vw;
    return {vw, rsp_pack::index_words(rsp::kSpmvThreads, fields), rsp_pack::words_per_thread(fields), fields};
}

// Field f of thread tid of a record: clear it, then OR `v` in.
void set_field(uint32_t *rec, const Geo &g, int tid, int f, uint32_t v) {
    uint32_t *w = rec + (size_t)tid * g.nwt;
    const int b = f * rsp_pack::kBits, i = b >> 5, sh = b & 31;
    w[i] &= ~(rsp_pack::kMask << sh);
    if (sh > 32 - rsp_pack::kBits) w[i + 1] &= ~(rsp_pack::kMask >> (32 - sh));
    rsp_pack::put_field(w, f, v);
}

// Corruption `mut` of the valid plan `p` into `q` (a copy of p); false: p has
// no such field. `o`: p's options.
bool mutate(int mut, const int *rp, const PlanOptions &o, const TilePlan &p, TilePlan &q) {
    using namespace rsp_plan;
    const Geo g = geo_of(o.type);
    const size_t nt = p.blocks.size();
    auto runs_tile = [&](size_t t) { return staged(p.cbase[t]) && !stage_decode(p.cbase[t]).list(); };
    auto list_tile = [&](size_t t) { return staged(p.cbase[t]) && stage_decode(p.cbase[t]).list(); };
    auto record = [&](size_t t) { return reinterpret_cast<uint32_t *>(q.runs.data()) + pack_decode(p.poff[t]).word; };
    for (size_t t = 0; t < nt; t++) {
        const rsp::SpmvBlock &b = p.blocks[t];
        const int len = b.k1 - b.k0, cb = p.cbase[t], po = p.poff[t];
        const int kb = b.k0 & ~(g.vw - 1);
        int *r = staged(cb) ? q.runs.data() + 2 * (size_t)stage_decode(cb).off : nullptr;
        const int nr = staged(cb) ? stage_decode(cb).nr : 0;
        switch (mut) {
            case 0:  // one 16-bit offset of a gathered tile + 1
                if (cb < 0 || len < 1) break;
                q.c16[(size_t)b.k0 + (size_t)len / 2]++;
                return true;
            case 1:  // a gathered tile's column base + 1
                if (cb < 0 || len < 1) break;
                q.cbase[t]++;
                return true;
            case 2:  // a run's first column + 1 (the last run's, so the runs stay apart)
                if (!runs_tile(t)) break;
                r[2 * (nr - 1)]++;
                return true;
            case 3:  // a run's first slot + 1 (run 1 where there is one)
                if (!runs_tile(t)) break;
                r[2 * (nr > 1 ? 1 : 0) + 1]++;
                return true;
            case 4:  // the sentinel's slot count - 1
                if (!runs_tile(t)) break;
                r[2 * nr + 1]--;
                return true;
            case 5:  // two neighbouring entries of different columns trade slots (in the 16-bit array and the record)
                if (!runs_tile(t)) break;
                for (int k = b.k0; k + 1 < b.k1; k++)
                    if (p.c16[(size_t)k] != p.c16[(size_t)k + 1]) {
                        std::swap(q.c16[(size_t)k], q.c16[(size_t)k + 1]);
                        if (po != kNoPack)
                            for (int e = k; e < k + 2; e++) {
                                const int v = (e - kb) / g.vw;
                                set_field(record(t), g, v % rsp::kSpmvThreads,
                                          (v / rsp::kSpmvThreads) * g.vw + (e - kb) % g.vw, q.c16[(size_t)e]);
                            }
                        return true;
                    }
                break;
            case 6:  // a listed offset + 1, onto its successor
                if (!list_tile(t)) break;
                for (int u = 0; u + 1 < r[1]; u++) {
                    uint16_t *ofs = reinterpret_cast<uint16_t *>(r + 2);
                    if (ofs[u] + 1 == ofs[u + 1]) {
                        ofs[u]++;
                        return true;
                    }
                }
                break;
            case 7:  // a list header's column count + 1
                if (!list_tile(t)) break;
                r[1]++;
                return true;
            case 8:  // a field outside [k0, k1) of a packed record = 1: entry kb's, or the last (k0 == kb: k1 - kb < kSlots)
                if (po == kNoPack) break;
                if (b.k0 > kb)
                    set_field(record(t), g, 0, 0, 1);
                else
                    set_field(record(t), g, rsp::kSpmvThreads - 1, g.fields - 1, 1);
                return true;
            case 9: {  // the field of a packed tile's middle entry + 1
                if (po == kNoPack) break;
                const int e = b.k0 + len / 2, v = (e - kb) / g.vw;
                const int tid = v % rsp::kSpmvThreads, f = (v / rsp::kSpmvThreads) * g.vw + (e - kb) % g.vw;
                set_field(record(t), g, tid, f, rsp_pack::get_field(record(t) + (size_t)tid * g.nwt, f) + 1);
                return true;
            }
            case 10:  // a packed row offset + 1 (the tile's last)
                if (po == kNoPack || !pack_decode(po).rows) break;
                record(t)[g.iw + ((b.r1 - b.r0) >> 1)] += 1u << (16 * ((b.r1 - b.r0) & 1));
                return true;
            case 11: {  // a correct record for a staged tile too small to be packed
                if (!staged(cb) || b.r1 < 0 || len < 1 || o.pack_mode == 0 ||
                    rsp_pack::eligible(rsp::kSpmvThreads, g.fields, len))
                    break;
                const size_t word = (q.runs.size() + 3) & ~(size_t)3;
                const bool rows = o.pack_mode >= 2;
                q.runs.resize(word + (size_t)g.iw + (rows ? rsp_pack::row_words(b.r1 - b.r0) : 0) + 4, 0);
                uint32_t *rec = reinterpret_cast<uint32_t *>(q.runs.data()) + word;
                rsp_pack::pack_slots(p.c16.data(), b.k0, b.k1, g.vw, rsp::kSpmvIter, rsp::kSpmvThreads, rec);
                if (rows) rsp_pack::pack_rows(rp, b.r0, b.r1 - b.r0, kb, rec + g.iw);
                q.poff[t] = pack_encode((int64_t)word, rows);
                q.tiles_packed++;
                q.nnz_packed += len;
                return true;
            }
            case 12:  // one interior tile more than there are (split schedules only)
                if (o.local_cols < 0) break;
                q.nint++;
                return true;
            case 13:  // two neighbouring tiles of one part trade places, codes and all
                if (t + 1 >= nt || (o.local_cols >= 0 && t + 1 == (size_t)p.nint)) break;
                std::swap(q.blocks[t], q.blocks[t + 1]);
                std::swap(q.cbase[t], q.cbase[t + 1]);
                std::swap(q.poff[t], q.poff[t + 1]);
                return true;
        }
    }
    return false;
}

int run_mutants(const char *name, int m, int cols, const std::vector<int> &rp, const std::vector<int> &ci) {
    for (const rsp_datatype_t type : {RSP_R_64F, RSP_R_32F}) {
        std::string applied, absent;
        for (int mut = 0; mut < kNumMutants; mut++) {
            PlanOptions o = rsp_plan::plan_options(type);
            if (mut == 12) o.local_cols = cols / 2;
            TilePlan p;
            rsp_plan::make_tile_plan(rp.data(), ci.data(), m, (int64_t)ci.size(), o, p);
            if (!rsp_plan::plan_verify(rp.data(), ci.data(), m, o, p)) {
                fprintf(stderr, "%s: plan_verify failed\n", name);
                return 3;
            }
            TilePlan q = p;
            if (!mutate(mut, rp.data(), o, p, q)) {
                absent += std::string(" ") + kMutants[mut];
                continue;
            }
            if (rsp_plan::plan_verify(rp.data(), ci.data(), m, o, q)) {
                fprintf(stderr, "%s %s: the corrupted plan '%s' verified\n", name, type == RSP_R_64F ? "f64" : "f32",
                        kMutants[mut]);
                return 5;
            }
            applied += std::string(" ") + kMutants[mut];
        }
        printf("%s %s rejected%s absent%s\n", name, type == RSP_R_64F ? "f64" : "f32", applied.c_str(), absent.c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const bool mutants = argc > 1 && strcmp(argv[1], "--mutate") == 0;
    if (mutants) {
        argc--;
        argv++;
    }
    const char *name = argc > 1 ? argv[1] : "dc1";
    int m = 0, cols = 0;
    std::vector<int> rp, ci;
    if (name[0] == '@') {
        if (argc < 3 || !read_pattern(name + 1, &m, &cols, rp, ci)) return 2;
        name = argv[2];
    } else {
        const double scale = argc > 2 ? atof(argv[2]) : 0.02;
        if (rsp_surrogate_rows(name, scale, &m) != 0) return 2;
        cols = m;
        std::vector<int> len((size_t)m);
        rp.assign((size_t)m + 1, 0);
        if (rsp_surrogate_rowlens(name, scale, 0, 0, m, len.data()) != 0) return 2;
        for (int i = 0; i < m; i++) rp[(size_t)i + 1] = rp[(size_t)i] + len[(size_t)i];
        ci.resize((size_t)rp[(size_t)m]);
        std::vector<double> v(ci.size());
        if (rsp_surrogate_fill(name, scale, 0, 0, m, rp.data(), ci.data(), v.data()) != 0) return 2;
    }
    if (mutants) return run_mutants(name, m, cols, rp, ci);
    const char *tags[] = {"default", "spread1024", "local", "align16", "noc16", "nostage", "local+spread1024"};
    for (const rsp_datatype_t type : {RSP_R_64F, RSP_R_32F})
        for (int s = 0; s < 7; s++) {
            rsp_plan::PlanOptions o = rsp_plan::plan_options(type);
            if (s == 1 || s == 6) o.spread = 1024;
            if (s == 2 || s == 6) o.local_cols = cols / 2;
            if (s == 3) o.row_align = 16;
            if (s == 4) o.use_c16 = false;
            if (s == 5) o.use_stage = false;
            rsp_plan::TilePlan p, p2;
            rsp_plan::make_tile_plan(rp.data(), ci.data(), m, (int64_t)ci.size(), o, p);
            rsp_plan::make_tile_plan(rp.data(), ci.data(), m, (int64_t)ci.size(), o, p2);
            const unsigned long long d = rsp_plan::digest(p);
            if (d != rsp_plan::digest(p2)) {
                fprintf(stderr, "%s %s: digest differs\n", name, tags[s]);
                return 4;
            }
            if (!rsp_plan::plan_verify(rp.data(), ci.data(), m, o, p)) {
                fprintf(stderr, "%s %s: plan_verify failed\n", name, tags[s]);
                return 3;
            }
            printf("%s %s %s tiles %lld e16 %lld staged %lld packed %lld digest %016llx\n", name,
                   type == RSP_R_64F ? "f64" : "f32", tags[s], (long long)p.blocks.size(), (long long)p.nnz_c16,
                   (long long)p.nnz_staged, (long long)p.tiles_packed, d);
        }
    return 0;
}
