// api_ilu_solve.cpp — the ILU(0) factor and the triangular solves of
// include/rsp.h: the launches of the kernels in ilu0.hip / trsv.hip / trsv_blocks.hip
// over the plans of api_ilu_analysis.cpp, and the recovery of a call whose
// flow wait gave up (the two *_zero_pivot calls). Mirrors the factor and
// solve calls of the reference driver (GPU/ilu0.cu:254-310).

#include "rsp_internal.h"

using namespace rsp_api;

// Flow launch control of one call (rsp::FlowCtl): status word and generation,
// give-up bound, the info's claim counter.
static rsp::FlowCtl flow_ctl(rsp_ilu0_info *f, int word, int gen) {
    rsp::FlowCtl c;
    c.status = f->d_zero + word;
    c.gen = gen;
    const long long us = std::max(env_int("RSP_ILU_FLOW_TIMEOUT_US", 200000), 0);
    c.ticks = (unsigned long long)us * 100ull;  // 100 MHz wall clock
    c.claim = reinterpret_cast<unsigned long long *>(f->d_zero + 6);
    c.claim_host = &f->claim_host;
    c.mode = env_int("RSP_ILU_FLOW_MODE", rsp::kFlowTickets);
    c.done = f->d_fdone;
    c.tickets = f->d_tk;
    c.grid_x = std::max(env_int("RSP_ILU_FLOW_GRID_X", 1), 1);
    c.tk_seq = &f->tk_seq;
    // (2^32 calls of one info before an epoch repeats; 0 is the array's initial value)
    if (++f->flow_epoch == 0) f->flow_epoch = 1;
    c.epoch = f->flow_epoch;
    return c;
}

// A DAG's plan for one call: its device arrays as uploaded (Dag::plan), the
// host arrays' addresses as they are now (a Dag may have been assigned since).
static rsp::LevelPlan level_plan(const rsp_ilu0_info::Dag &d, const rsp_an::hvec<rsp::LevelSeg> &segs, int batch) {
    rsp::LevelPlan p = d.plan;
    p.ptr_host = d.ptr.data();
    p.nlev = (int)d.ptr.size() - 1;
    p.segs = segs.data();
    p.nseg = (int)segs.size();
    p.batch = batch;
    p.group = d.group;
    p.nterms = d.nterms;
    p.nshort_host = d.nshort.data();
    p.nwave_host = d.nwave.empty() ? nullptr : d.nwave.data();
    p.sbase_host = d.sbase.empty() ? nullptr : d.sbase.data();
    p.has_flow = 0;
    for (const rsp::LevelSeg &sg : segs) p.has_flow |= !sg.thin && sg.c1 > sg.c0;
    return p;
}

static bool flow_recover() { return env_int("RSP_ILU_FLOW_RECOVER", 1) != 0; }

// One factor call (flow_ok = false: no flow launch, every fat level its own
// launch — the recovery run of rsp_ilu0_zero_pivot).
static rsp_status_t ilu_factor_run(rsp_handle_t h, rsp_ilu0_info *f, rsp_datatype_t value_type, void *d_values,
                                   bool flow_ok) {
    RSP_CHECK_HIP(hipMemsetD32Async(f->d_zero, INT_MAX, 1, h->stream));
    rsp::IluArgs a = f->fac;  // the pattern, the symbolic arrays, the factor plan; this call's:
    a.vals = d_values;
    a.fslev = f->fslev.empty() ? nullptr : f->fslev.data();
    a.fat_slots = a.fslots && env_int("RSP_ILU_FAT_SLOT", 1) != 0;
    a.fat_lds = env_int("RSP_ILU_FAT_LDS", 1) != 0;
    a.defer_rounds = env_int("RSP_ILU_DEFER", 8);  // A/B knob (thin factor runs)
    a.narrow_waves = std::min(std::max(env_int("RSP_ILU_FNARROW_WAVES", 4), 1), rsp::kThinThreads / 64);
    a.plan = level_plan(f->fdag(), f->fac_segs, f->fac_batch);
    a.fruns = f->fruns.empty() ? nullptr : f->fruns.data();
    a.nfruns = a.fat_slots ? (int)f->fruns.size() : 0;
    if (f->fac_gen >= (1 << 30)) {  // generations wrap
        RSP_CHECK_HIP(hipMemsetD32Async(f->d_zero + 1, 0, 1, h->stream));  // no stale give-up
        f->fac_gen = 0;
    }
    a.gen = ++f->fac_gen;
    a.flow = flow_ok && env_int("RSP_ILU_FLOW", 1) != 0;
    a.flow_grid = h->num_cus * std::min(std::max(env_int("RSP_ILU_FLOW_WPC", 4), 4), 16) / 4;
    a.flow_cus = h->num_cus;
    a.flow_sleep = std::min(std::max(env_int("RSP_ILU_FLOW_SLEEP", 1), 1), 64);
    a.fc = flow_ctl(f, 1, a.gen);
    // diagnostics: RSP_ILU_FTRACE=<file> appends per-chunk shader-clock stamps
    // of the thin factor runs (host-blocking; never set in timed runs)
    const char *trace_file = getenv("RSP_ILU_FTRACE");
    unsigned long long *&d_trace = h->d_ftrace;
    const int trace_cap = 1 << 22;
    if (trace_file) {
        if (!d_trace) RSP_CHECK_HIP(hipMalloc((void **)&d_trace, trace_cap * sizeof(unsigned long long)));
        RSP_CHECK_HIP(hipMemsetAsync(d_trace, 0, trace_cap * sizeof(unsigned long long), h->stream));
        a.trace = d_trace;
        a.trace_cap = trace_cap;
    }
    hipError_t e;
    if (value_type == RSP_R_64F)
        e = rsp_k::ilu0_factor_f64(a, h->stream);
    else
        e = h->ftz ? rsp_k_ftz::ilu0_factor_f32(a, h->stream) : rsp_k::ilu0_factor_f32(a, h->stream);
    if (trace_file && e == hipSuccess) {
        rsp_an::hvec<unsigned long long> t(trace_cap);
        RSP_CHECK_HIP(hipMemcpyAsync(t.data(), d_trace, t.size() * sizeof(t[0]), hipMemcpyDeviceToHost,
                                     h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        if (FILE *fp = fopen(trace_file, "a")) {
            fprintf(fp, "# factor n=%d\n", f->n);
            for (int c = 0; c < trace_cap / 4; c++)
                if (t[4 * (size_t)c])
                    fprintf(fp, "%d %llu %llu %llu %llu %llu\n", c, t[4 * (size_t)c], t[4 * (size_t)c + 1],
                            t[4 * (size_t)c + 2], t[4 * (size_t)c + 3] & 0xffffffffull, t[4 * (size_t)c + 3] >> 32);
            fclose(fp);
        }
    }
    f->factored = 1;
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

// rsp_ilu0_factor: the input values kept for a recovery run, then the factor.
static rsp_status_t ilu0_factor(rsp_handle_t h, rsp_ilu0_info *f, rsp_datatype_t value_type, void *d_values) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!f || !f->analysed || (f->nnz_s > 0 && !d_values)) return RSP_STATUS_INVALID_VALUE;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    // a factor with flow runs keeps its input values for a recovery run
    // (rsp_ilu0_info::fbackup): one device copy of the values per call
    f->last_fac.valid = 0;
    const bool flows = !f->fruns.empty() && f->fac.fslots && env_int("RSP_ILU_FLOW", 1) != 0 &&
                       env_int("RSP_ILU_FAT_SLOT", 1) != 0;
    if (flows && f->nnz_s > 0 && flow_recover()) {
        const size_t bytes = (size_t)f->nnz_s * elem_size(value_type);
        if (f->fbackup_bytes < bytes) {
            f->fbackup = DevMem();
            f->fbackup_bytes = 0;
            RSP_CHECK_HIP(hipMalloc(&f->fbackup.p, bytes));
            f->fbackup_bytes = bytes;
        }
        RSP_CHECK_HIP(hipMemcpyAsync(f->fbackup.p, d_values, bytes, hipMemcpyDeviceToDevice, h->stream));
        f->last_fac.valid = 1;
        f->last_fac.seq = ++f->call_seq;
        f->last_fac.ftz = h->ftz;
        f->last_fac.type = value_type;
        f->last_fac.vals = d_values;
    }
    return ilu_factor_run(h, f, value_type, d_values, true);
}

static rsp::TrsvArgs trsv_args(rsp_handle_t h, rsp_ilu0_info *f, const void *alpha, rsp_datatype_t t,
                               const void *vals, const void *x, void *y) {
    rsp::TrsvArgs a;
    a.n = f->n;
    a.rowptr = f->fac.rowptr;
    a.colidx = f->fac.colidx;
    a.dpos = f->fac.dpos;
    a.hasdiag = f->fac.hasdiag;
    a.vals = vals;
    a.x = x;
    a.y = y;
    a.alpha = (t == RSP_R_64F) ? *(const double *)alpha : (double)*(const float *)alpha;
    a.plan = level_plan(f->L, f->L.segs, f->L.batch);
    a.sval = f->d_sval;
    a.sx = f->d_sx;
    a.sdg = f->d_sdg;
    a.trace = nullptr;
    a.trace_cap = 0;
    a.trace_clk = 0;
    a.wave_lds = env_int("RSP_ILU_WAVE_LDS", 1);
    a.narrow_waves = std::min(std::max(env_int("RSP_ILU_NARROW_WAVES", 4), 1), rsp::kThinThreads / 64);
    a.narrow_split = env_int("RSP_ILU_NARROW_SPLIT", 0) != 0;  // (default off: slower)
    a.narrow_pairs = env_int("RSP_ILU_NARROW_PAIRS", -1);  // -1: by the DAG's level width (launcher)
    a.loaders = env_int("RSP_ILU_LOADERS", 1);
    a.flow = env_int("RSP_ILU_FLOW", 1) != 0;
    // 256-thread workgroups, RSP_ILU_FLOW_WPC waves per CU: 8 for the solves
    // (config 3, start tickets: solve 34.34 -> 33.95 ms against 4; the
    // factor's flow stays at 4: 40.11 vs 40.15 ms); no residency is needed
    // with start tickets, the static walk (RSP_ILU_FLOW_MODE=0) needs the
    // whole grid resident (flow_grid caps it by the occupancy query)
    a.flow_grid = h->num_cus * std::min(std::max(env_int("RSP_ILU_FLOW_WPC", 8), 4), 16) / 4;
    a.flow_cus = h->num_cus;
    a.flow_sleep = std::min(std::max(env_int("RSP_ILU_FLOW_SLEEP", 1), 1), 64);
    return a;
}

// A solve call of kind `which` (RSP_TRSV_*): its generation (status word
// 2 + which; generations restart with the factor's wrap-around below 2^30).
static hipError_t trsv_begin(rsp_handle_t h, rsp_ilu0_info *f, int which, rsp::TrsvArgs &a) {
    int &g = f->solve_gen[which];
    if (g >= (1 << 30)) {  // wrap: no stale give-up may match a new generation
        const hipError_t e = hipMemsetD32Async(f->d_zero + 2 + which, 0, 1, h->stream);
        if (e != hipSuccess) return e;
        g = 0;
    }
    a.fc = flow_ctl(f, 2 + which, ++g);
    return hipSuccess;
}

// A solve call's arguments, kept for its recovery run (rsp_ilu0_info::last_solve).
static void remember_solve(rsp_handle_t h, rsp_ilu0_info *f, int which, rsp_operation_t op, const void *alpha,
                           rsp_datatype_t t, const void *vals, const void *x, void *y) {
    rsp_ilu0_info::SolveCall &c = f->last_solve[which];
    c.seq = ++f->call_seq;
    c.valid = 1;
    c.ftz = h->ftz;
    c.op = op;
    c.alpha = t == RSP_R_64F ? *(const double *)alpha : (double)*(const float *)alpha;
    c.type = t;
    c.vals = vals;
    c.x = x;
    c.y = y;
}

// flow_ok = false: the recovery run of rsp_trsv_zero_pivot (no flow launch)
rsp_status_t rsp_api::rsp_trsv_lower_unit_impl(rsp_handle_t h, rsp_operation_t op, const void *alpha,
                                               rsp_ilu0_info *f, rsp_datatype_t value_type,
                                               const void *d_values, const void *d_x, void *d_y, bool flow_ok) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!f || !f->analysed || !alpha) return RSP_STATUS_INVALID_VALUE;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (f->n > 0 && (!d_x || !d_y || d_x == d_y)) return RSP_STATUS_INVALID_VALUE;
    if (op != RSP_OPERATION_NON_TRANSPOSE && op != RSP_OPERATION_TRANSPOSE) return RSP_STATUS_INVALID_VALUE;
    {
        const rsp_status_t st = ilu_solves_ready(h, f);  // (rsp_trsv_analysis not called: done here)
        if (st != RSP_STATUS_SUCCESS) return st;
    }
    remember_solve(h, f, op == RSP_OPERATION_NON_TRANSPOSE ? RSP_TRSV_L : RSP_TRSV_LT, op, alpha, value_type,
                   d_values, d_x, d_y);
    rsp::TrsvArgs a = trsv_args(h, f, alpha, value_type, d_values, d_x, d_y);
    a.flow = a.flow && flow_ok;
    // diagnostics: RSP_ILU_TRACE=<file> appends per-chunk timestamps of the
    // prefetching thin kernel (host-blocking; never set in timed runs)
    const char *trace_file = getenv("RSP_ILU_TRACE");
    unsigned long long *&d_trace = h->d_strace;
    const int trace_cap = 4 << 20;
    if (trace_file) {
        if (!d_trace) RSP_CHECK_HIP(hipMalloc((void **)&d_trace, trace_cap * sizeof(unsigned long long)));
        RSP_CHECK_HIP(hipMemsetAsync(d_trace, 0, trace_cap * sizeof(unsigned long long), h->stream));
        a.trace = d_trace;
        a.trace_cap = trace_cap;
        a.trace_clk = env_int("RSP_ILU_TRACE_CLK", 0);
    }
    hipError_t e;
    const bool f64 = value_type == RSP_R_64F, ftz = h->ftz != 0;
    RSP_CHECK_HIP(trsv_begin(h, f, op == RSP_OPERATION_NON_TRANSPOSE ? RSP_TRSV_L : RSP_TRSV_LT, a));
    // a deep DAG: the block-inverse solve (trsv_blocks.hip; RSP_ILU_BLOCKS=0
    // at solve time runs the level-scheduled solve of the same analysis)
    const rsp_ilu0_info::BlkDag &bd = op == RSP_OPERATION_NON_TRANSPOSE ? f->Lb : f->LTb;
    if (bd.on && env_int("RSP_ILU_BLOCKS", -1) != 0) {
        rsp::BlkArgs b = bd.args;  // the plan and its scratch; this call's:
        b.segs = bd.segs.data();
        b.nseg = (int)bd.segs.size();
        b.vals = d_values;
        b.x = d_x;
        b.y = d_y;
        b.alpha = a.alpha;
        e = f64 ? rsp_k::trsv_blocks_f64(b, h->stream)
                : (ftz ? rsp_k_ftz::trsv_blocks_f32(b, h->stream) : rsp_k::trsv_blocks_f32(b, h->stream));
        return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
    }
    if (op == RSP_OPERATION_NON_TRANSPOSE) {
        e = f64 ? rsp_k::trsv_lower_n_f64(a, h->stream)
                : (ftz ? rsp_k_ftz::trsv_lower_n_f32(a, h->stream) : rsp_k::trsv_lower_n_f32(a, h->stream));
    } else {
        a.plan = level_plan(f->LT, f->LT.segs, f->LT.batch);
        e = f64 ? rsp_k::trsv_lower_t_f64(a, h->stream)
                : (ftz ? rsp_k_ftz::trsv_lower_t_f32(a, h->stream) : rsp_k::trsv_lower_t_f32(a, h->stream));
    }
    if (trace_file && e == hipSuccess) {
        rsp_an::hvec<unsigned long long> t(trace_cap);
        RSP_CHECK_HIP(hipMemcpyAsync(t.data(), d_trace, t.size() * sizeof(t[0]), hipMemcpyDeviceToHost,
                                     h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        if (FILE *fp = fopen(trace_file, "a")) {
            fprintf(fp, "# solve op=%d n=%d\n", (int)op, f->n);
            for (int l = 0; l < trace_cap / 2; l++)
                if (t[(size_t)trace_cap / 2 + l])
                    fprintf(fp, "L %d %llu\n", l, t[(size_t)trace_cap / 2 + l]);
            for (int c = 0; c < trace_cap / 16; c++)
                if (t[8 * (size_t)c] || t[8 * (size_t)c + 3])
                    fprintf(fp, "%d %llu %llu %llu %llu %llu %llu\n", c, t[8 * (size_t)c],
                            t[8 * (size_t)c + 1], t[8 * (size_t)c + 2], t[8 * (size_t)c + 3],
                            t[8 * (size_t)c + 4], t[8 * (size_t)c + 5]);
            fclose(fp);
        }
    }
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

rsp_status_t rsp_api::rsp_trsv_upper_impl(rsp_handle_t h, const void *alpha, rsp_ilu0_info *f,
                                          rsp_datatype_t value_type, const void *d_values, const void *d_x,
                                          void *d_y, bool flow_ok) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!f || !f->analysed || !alpha) return RSP_STATUS_INVALID_VALUE;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (f->n > 0 && (!d_x || !d_y || d_x == d_y)) return RSP_STATUS_INVALID_VALUE;
    rsp_status_t st = ilu_solves_ready(h, f);  // (the solve streams)
    if (st != RSP_STATUS_SUCCESS) return st;
    st = ilu_plan_u(h, f);  // planned on first use
    if (st != RSP_STATUS_SUCCESS) return st;
    remember_solve(h, f, RSP_TRSV_U, RSP_OPERATION_NON_TRANSPOSE, alpha, value_type, d_values, d_x, d_y);
    rsp::TrsvArgs a = trsv_args(h, f, alpha, value_type, d_values, d_x, d_y);
    a.flow = a.flow && flow_ok;
    a.plan = level_plan(f->U, f->U.segs, f->U.batch);
    a.sval = f->d_usval;
    RSP_CHECK_HIP(trsv_begin(h, f, RSP_TRSV_U, a));
    hipError_t e;
    if (value_type == RSP_R_64F)
        e = rsp_k::trsv_upper_f64(a, h->stream);
    else
        e = h->ftz ? rsp_k_ftz::trsv_upper_f32(a, h->stream) : rsp_k::trsv_upper_f32(a, h->stream);
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

/* ------- recovery of a flow give-up (rsp_ilu0_info::fbackup / last_solve) */

// Re-run one recorded solve without flow launches (rsp_ilu0_info::last_solve).
static rsp_status_t rerun_solve(rsp_handle_t h, rsp_ilu0_info *f, int which) {
    const rsp_ilu0_info::SolveCall c = f->last_solve[which];
    const double a64 = c.alpha;
    const float a32 = (float)c.alpha;
    const void *al = c.type == RSP_R_64F ? (const void *)&a64 : (const void *)&a32;
    const int ftz = h->ftz;
    h->ftz = c.ftz;  // the mode of the call being re-run
    const rsp_status_t st = which == RSP_TRSV_U
                                ? rsp_trsv_upper_impl(h, al, f, c.type, c.vals, c.x, c.y, false)
                                : rsp_trsv_lower_unit_impl(h, c.op, al, f, c.type, c.vals, c.x, c.y, false);
    h->ftz = ftz;
    return st;
}

// The recorded solves made after call `seq`, in call order (their inputs
// came from the call being recovered).
struct LaterSolves {
    int w[3];
    int k = 0;
};
static LaterSolves later_solves(const rsp_ilu0_info *f, long long seq) {
    LaterSolves l;
    for (int w = 0; w < 3; w++)
        if (f->last_solve[w].valid && f->last_solve[w].seq > seq) l.w[l.k++] = w;
    std::sort(l.w, l.w + l.k, [&](int a, int b) { return f->last_solve[a].seq < f->last_solve[b].seq; });
    return l;
}
// Whether a re-run of `first` (a solve kind, or -1 for the factor) and then
// of the solves `l` reads the inputs the original calls read: no recorded
// call after a re-run call may have written (its y) over that call's x or
// values. The ping-pong pattern (L solve r -> z, then L^T z -> r) overwrites
// the L solve's x, so its re-run would read the L^T result: not recoverable.
static bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const char *p = (const char *)a, *q = (const char *)b;
    return p && q && p < q + nb && q < p + na;
}
static bool rerun_inputs_intact(const rsp_ilu0_info *f, int first, const LaterSolves &l) {
    int seq[4], k = 0;
    if (first >= 0) seq[k++] = first;
    for (int j = 0; j < l.k; j++) seq[k++] = l.w[j];
    for (int a = 0; a < k; a++) {
        const rsp_ilu0_info::SolveCall &c = f->last_solve[seq[a]];
        const size_t ny = (size_t)f->n * elem_size(c.type), nv = (size_t)f->nnz_s * elem_size(c.type);
        for (int b = a + 1; b < k; b++) {
            const rsp_ilu0_info::SolveCall &d = f->last_solve[seq[b]];
            if (overlaps(d.y, (size_t)f->n * elem_size(d.type), c.x, ny) ||
                overlaps(d.y, (size_t)f->n * elem_size(d.type), c.vals, nv))
                return false;
        }
    }
    if (first < 0 && f->last_fac.valid)  // the factor's values are restored from the copy, but a
        for (int a = 0; a < k; a++) {    // later solve must not have written into them
            const rsp_ilu0_info::SolveCall &d = f->last_solve[seq[a]];
            if (overlaps(d.y, (size_t)f->n * elem_size(d.type), f->last_fac.vals,
                         (size_t)f->nnz_s * elem_size(f->last_fac.type)))
                return false;
        }
    return true;
}

static rsp_status_t rerun_solves(rsp_handle_t h, rsp_ilu0_info *f, const LaterSolves &l) {
    for (int j = 0; j < l.k; j++) {
        const rsp_status_t st = rerun_solve(h, f, l.w[j]);
        if (st != RSP_STATUS_SUCCESS) return st;
    }
    return RSP_STATUS_SUCCESS;
}

// rsp_ilu0_zero_pivot: the structural or numerical zero pivot of the last
// factor, after the recovery of a factor whose flow wait gave up.
static rsp_status_t ilu0_zero_pivot(rsp_handle_t h, rsp_ilu0_info *f, int *position) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!f || !position) return RSP_STATUS_INVALID_VALUE;
    *position = -1;
    if (!f->analysed) return RSP_STATUS_INVALID_VALUE;
    int pos = f->structural_zero;
    int z[2] = {INT_MAX, 0};  // zero pivot, give-up generation of the factor calls
    RSP_CHECK_HIP(hipMemcpyAsync(z, f->d_zero, sizeof(z), hipMemcpyDeviceToHost, h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    // the last factor's flow wait gave up: its values are wrong. Recovered
    // (rsp_ilu0_info::fbackup): the input values restored, the factor run
    // again without flow launches; else reported.
    if (f->factored && f->fac_gen > 0 && z[1] == f->fac_gen) {
        if (!f->last_fac.valid || !flow_recover()) return RSP_STATUS_EXECUTION_FAILED;
        const LaterSolves later = later_solves(f, f->last_fac.seq);
        if (!rerun_inputs_intact(f, -1, later)) return RSP_STATUS_EXECUTION_FAILED;
        f->last_fac.valid = 0;
        RSP_CHECK_HIP(hipMemcpyAsync(f->last_fac.vals, f->fbackup.p, (size_t)f->nnz_s * elem_size(f->last_fac.type),
                                     hipMemcpyDeviceToDevice, h->stream));
        const int ftz = h->ftz;
        h->ftz = f->last_fac.ftz;  // the mode of the call being re-run
        rsp_status_t st = ilu_factor_run(h, f, f->last_fac.type, f->last_fac.vals, false);
        h->ftz = ftz;
        if (st == RSP_STATUS_SUCCESS) st = rerun_solves(h, f, later);
        if (st != RSP_STATUS_SUCCESS) return st;
        RSP_CHECK_HIP(hipMemcpyAsync(z, f->d_zero, sizeof(z), hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        if (z[1] == f->fac_gen) return RSP_STATUS_EXECUTION_FAILED;
    }
    if (f->factored && z[0] != INT_MAX && (pos < 0 || z[0] < pos)) pos = z[0];
    if (pos >= 0) {
        *position = pos;
        return RSP_STATUS_ZERO_PIVOT;
    }
    return RSP_STATUS_SUCCESS;
}

// cusparseXcsrsv2_zeroPivot for the solves (reference: the csrsv2 info
// objects of GPU/ilu0.cu:143-150). Host-blocking. EXECUTION_FAILED: the last
// solve of that kind gave up a flow wait (its y is wrong; never expected, a
// bound instead of a GPU hang). The unit-lower solves have no pivots; the U
// solve (extension) reports the factor's zero pivot, which it divides by.
static rsp_status_t trsv_zero_pivot(rsp_handle_t h, rsp_ilu0_info *f, int which, int *position) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!f || !position || which < RSP_TRSV_L || which > RSP_TRSV_U) return RSP_STATUS_INVALID_VALUE;
    *position = -1;
    if (!f->analysed) return RSP_STATUS_INVALID_VALUE;
    int z[5];
    RSP_CHECK_HIP(hipMemcpyAsync(z, f->d_zero, sizeof(z), hipMemcpyDeviceToHost, h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    const int g = f->solve_gen[which];
    if (g > 0 && z[2 + which] == g) {  // recovered: the solve (and the solves after it) run again
        if (!f->last_solve[which].valid || !flow_recover()) return RSP_STATUS_EXECUTION_FAILED;
        const LaterSolves later = later_solves(f, f->last_solve[which].seq);
        if (!rerun_inputs_intact(f, which, later)) return RSP_STATUS_EXECUTION_FAILED;
        rsp_status_t st = rerun_solve(h, f, which);
        if (st == RSP_STATUS_SUCCESS) st = rerun_solves(h, f, later);
        if (st != RSP_STATUS_SUCCESS) return st;
        RSP_CHECK_HIP(hipMemcpyAsync(z, f->d_zero, sizeof(z), hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        if (z[2 + which] == f->solve_gen[which]) return RSP_STATUS_EXECUTION_FAILED;
    }
    if (which == RSP_TRSV_U) {
        int pos = f->structural_zero;
        if (f->factored && z[0] != INT_MAX && (pos < 0 || z[0] < pos)) pos = z[0];
        if (pos >= 0) {
            *position = pos;
            return RSP_STATUS_ZERO_PIVOT;
        }
    }
    return RSP_STATUS_SUCCESS;
}

extern "C" {

rsp_status_t rsp_ilu0_factor(rsp_handle_t h, rsp_ilu0_info_t f, rsp_datatype_t value_type,
                             void *d_values) {
    return guarded([&] { return ilu0_factor(h, f, value_type, d_values); });
}

rsp_status_t rsp_trsv_lower_unit(rsp_handle_t h, rsp_operation_t op, const void *alpha,
                                 rsp_ilu0_info_t f, rsp_datatype_t value_type,
                                 const void *d_values, const void *d_x, void *d_y) {
    return guarded([&] { return rsp_trsv_lower_unit_impl(h, op, alpha, f, value_type, d_values, d_x, d_y, true); });
}

rsp_status_t rsp_trsv_upper(rsp_handle_t h, const void *alpha, rsp_ilu0_info_t f,
                            rsp_datatype_t value_type, const void *d_values, const void *d_x,
                            void *d_y) {
    return guarded([&] { return rsp_trsv_upper_impl(h, alpha, f, value_type, d_values, d_x, d_y, true); });
}

rsp_status_t rsp_ilu0_zero_pivot(rsp_handle_t h, rsp_ilu0_info_t f, int *position) {
    return guarded([&] { return ilu0_zero_pivot(h, f, position); });
}

rsp_status_t rsp_trsv_zero_pivot(rsp_handle_t h, rsp_ilu0_info_t f, int which, int *position) {
    return guarded([&] { return trsv_zero_pivot(h, f, which, position); });
}

}  // the C ABI
