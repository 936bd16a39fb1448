// an_host_check.cpp — sanitizer driver for the ILU analysis' host half
// (never shipped): builds the plan of a surrogate twice (the second time with
// the U plan too) through rsp_an::plan_host — the worker pool, the concurrent
// L / L^T / factor plans, the factor pieces' shared position table and the
// block cache all run — and checks the two digests agree. Prints the plan
// digest last and, before the word "digest", a hash of the U plan (the arrays
// rsp_an::digest covers for L), which the plan digest leaves out. Built by
// `make -C respasol_amd/csrc tsan` (ThreadSanitizer) and `asan-an`
// (Address + UndefinedBehaviorSanitizer); tests/test_sanitize.py runs both.
//     an_host_check <surrogate> [scale]
// Second mode (tests/test_lvl_cases.py): the plan check of ilu_plan_check.cpp
// tested on itself. The pattern comes from a file of int32: n, n + 1 row
// offsets, the column indices (base 0).
//     an_host_check --pattern <file>
// plan_host's plans (U included; the budget as rsp_ilu0_plan_facts_host takes
// it) must pass rsp_an::check_plans; then a copy of the valid plan is
// corrupted four ways, each in the first of L / L^T / U that has a target,
// and the check must reject every one:
//   window   a window term's source moved to the neighbouring slot;
//   staged   one staged term dropped from its chunk;
//   chunk    a chunk's x1 moved so that it holds kChunkRows + 1 rows;
//   short    a flow item's short-row count raised to 65.
// One line per corruption: "<name> rejected: <the check's words>" or "<name>
// absent" (the plan has no such thing to corrupt). Exit 0 unless the valid
// plan fails (5) or a corruption passes (6).
#include "ilu_analysis.h"
#include "rsp_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>

static int check_pattern(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    int n = -1;
    if (fread(&n, sizeof n, 1, f) != 1 || n < 0) return 2;
    std::vector<int> rp((size_t)n + 1);
    if (fread(rp.data(), sizeof(int), rp.size(), f) != rp.size() || rp[0] != 0 || rp[(size_t)n] < 0) return 2;
    std::vector<int> ci((size_t)rp[(size_t)n]);
    if (fread(ci.data(), sizeof(int), ci.size(), f) != ci.size()) return 2;
    fclose(f);
    const long long cap_mb = rsp_an::env_int("RSP_ILU_SLOT_CAP_MB", -1);
    const long long cap = cap_mb >= 0 ? cap_mb * (1LL << 20) / 4 : 1LL << 29;
    rsp_an::IluHostPlan hp;
    rsp_an::Phases ph;
    ph.start();
    if (rsp_an::plan_host(n, rp.data(), ci.data(), cap, true, hp, ph) != RSP_STATUS_SUCCESS) return 3;
    const std::string ok = rsp_an::check_plans(rp.data(), ci.data(), hp, cap);
    if (!ok.empty()) {
        fprintf(stderr, "the valid plan fails: %s\n", ok.c_str());
        return 5;
    }
    // a corruption: true if it found its target in this DAG's plan
    using Corrupt = std::function<bool(rsp_an::SolvePlan &)>;
    const std::pair<const char *, Corrupt> corruptions[] = {
        {"window", [](rsp_an::SolvePlan &sp) {
             for (int &s : sp.src)
                 if (s < 0 && s != rsp::kPadSrc) {
                     s = -(((-s - 1 + 1) & (rsp::kYWin - 1)) + 1);
                     return true;
                 }
             return false;
         }},
        {"staged", [](rsp_an::SolvePlan &sp) {
             for (size_t c = 0; c < sp.chunks.size(); c++)
                 if (sp.chunks[c].st1 > sp.chunks[c].st0) {  // the chunk's last record goes; later chunks move up
                     sp.stg.erase(sp.stg.begin() + (sp.chunks[c].st1 - 1));
                     sp.chunks[c].st1--;
                     for (size_t d = c + 1; d < sp.chunks.size(); d++) sp.chunks[d].st0--, sp.chunks[d].st1--;
                     return true;
                 }
             return false;
         }},
        {"chunk", [](rsp_an::SolvePlan &sp) {
             for (const rsp::LevelSeg &sg : sp.segs)
                 if (sg.thin) {
                     sp.chunks[(size_t)sg.c0].x1 = sp.chunks[(size_t)sg.c0].x0 + rsp::kChunkRows + 1;
                     return true;
                 }
             return false;
         }},
        {"short", [](rsp_an::SolvePlan &sp) {
             for (const rsp::LevelSeg &sg : sp.segs) {
                 if (sg.thin) continue;
                 for (int it = sg.c0; it < sg.c1; it++)
                     if (sp.fitems[(size_t)it].n > 0) {
                         sp.fitems[(size_t)it].n = 65;
                         return true;
                     }
             }
             return false;
         }}};
    int rc = 0;
    for (const auto &c : corruptions) {
        bool found = false;
        for (int dag = 0; dag < 3 && !found; dag++) {
            rsp_an::IluHostPlan bad = hp;
            rsp_an::SolvePlan &sp = dag == 0 ? bad.L.sp : (dag == 1 ? bad.LT.sp : bad.U.sp);
            if (!c.second(sp)) continue;
            found = true;
            const std::string why = rsp_an::check_plans(rp.data(), ci.data(), bad, cap);
            if (why.empty()) {
                printf("%s PASSED the check\n", c.first);
                rc = 6;
            } else {
                printf("%s rejected: %s\n", c.first, why.c_str());
            }
        }
        if (!found) printf("%s absent\n", c.first);
    }
    return rc;
}

int main(int argc, char **argv) {
    if (argc > 2 && strcmp(argv[1], "--pattern") == 0) return check_pattern(argv[2]);
    const char *name = argc > 1 ? argv[1] : "dc1";
    const double scale = argc > 2 ? atof(argv[2]) : 0.02;
    int m = 0;
    if (rsp_surrogate_rows(name, scale, &m) != 0) return 2;
    std::vector<int> len((size_t)m), rp((size_t)m + 1, 0);
    if (rsp_surrogate_rowlens(name, scale, 0, 0, m, len.data()) != 0) return 2;
    for (int i = 0; i < m; i++) rp[(size_t)i + 1] = rp[(size_t)i] + len[(size_t)i];
    std::vector<int> ci((size_t)rp[(size_t)m]);
    std::vector<double> v((size_t)rp[(size_t)m]);
    if (rsp_surrogate_fill(name, scale, 0, 0, m, rp.data(), ci.data(), v.data()) != 0) return 2;
    unsigned long long d0 = 0;
    rsp_an::Fnv fu;
    for (int rep = 0; rep < 2; rep++) {
        rsp_an::IluHostPlan hp;
        rsp_an::Phases ph;
        ph.start();
        if (rsp_an::plan_host(m, rp.data(), ci.data(), 1LL << 26, rep == 1, hp, ph) != RSP_STATUS_SUCCESS) return 3;
        const unsigned long long d = rsp_an::digest(hp);
        if (rep == 0) d0 = d; else if (d != d0) { fprintf(stderr, "digest differs\n"); return 4; }
        const rsp_an::SolvePlan &sp = hp.U.sp;  // (empty arrays at rep 0)
        fu = rsp_an::Fnv();
        fu.vec(hp.U.ptr), fu.vec(hp.U.rows), fu.vec(sp.tasks), fu.vec(sp.tpos), fu.vec(sp.src), fu.vec(sp.segs);
        fu.vec(sp.chunks), fu.vec(sp.trow), fu.vec(sp.sid), fu.vec(sp.stg), fu.vec(sp.nshort), fu.vec(sp.nwave);
        fu.vec(sp.sbase), fu.vec(sp.fitems);
    }
    printf("%s n=%d U %016llx digest %016llx\n", name, m, (unsigned long long)fu.h, d0);
    return 0;
}
