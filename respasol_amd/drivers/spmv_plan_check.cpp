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
#include "spmv_plan.h"
#include "rsp_host.h"
#include <stdio.h>
#include <stdlib.h>
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

int main(int argc, char **argv) {
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
