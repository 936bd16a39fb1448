// rsp_internal.h — what the host units of librsp.so share: the three structs
// behind the opaque handles of include/rsp.h, the status macros, guarded()
// and the few functions one unit calls in another (namespace rsp_api).
//   rsp_api.cpp           handle, matrix descriptor, SpMV (plan upload, run, batch)
//   spmv_plan.cpp         the SpMV planner (spmv_plan.h; no HIP calls)
//   api_ilu_analysis.cpp  ILU(0) analysis, the solve plans, the plan queries
//   api_ilu_solve.cpp     factor and triangular solves, flow give-up recovery
//   api_krylov.cpp        BiCGStab, GMRES, rsp_dot, rsp_orthogonalize
#pragma once

#include "rsp.h"

#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <vector>

#include "rsp_kernels.h"
#include "ilu_analysis.h"
#include "spmv_plan.h"

struct rsp_context {
    int device;
    hipStream_t stream;
    int ftz;
    int spmv_variant;  // RSP_SPMV_VARIANT (tuning knob, default 0)
    int num_cus;
    // diagnostic trace buffers (RSP_ILU_FTRACE / RSP_ILU_TRACE), allocated
    // on the handle's device on first use, freed by rsp_destroy
    unsigned long long *d_ftrace;
    unsigned long long *d_strace;
    // rsp_dot: a Krylov block (rsp::kKryBlockDoubles) and its pinned mirror of
    // the partials, allocated on first use, freed by rsp_destroy
    double *d_dot;
    double *h_dot;
    // rsp_orthogonalize: a GMRES block (rsp::kGmBlockDoubles) and its pinned
    // mirror (h, h' and the norm's partials), as d_dot / h_dot
    double *d_gm;
    double *h_gm;
};

// The SpMV schedule lives in device memory owned by the matrix descriptor
// (d_plan), not in the caller's workspace: it is built once, at
// rsp_spmv_buffer_size time (where the reference calls
// cusparseSpMV_bufferSize, GPU/spmv.cu:159-164, outside its timed loop), so
// the reference's exact call sequence create_csr -> bufferSize -> malloc ->
// 50x SpMV pays no planning inside a timed call, and any number of matrices
// may share one workspace without re-planning.
struct rsp_spmat {
    int64_t rows, cols, nnz;
    int *rowptr;
    int *colidx;
    void *vals;
    rsp_datatype_t type;
    // schedule state
    int planned;                // d_plan holds a schedule for plan_type / local_cols
    int plan_device;            // device d_plan was allocated on
    void *d_plan;               // [tiles | long rows | partials | col bases | record offsets | 16-bit offsets | runs, records]
    size_t plan_cap;            // bytes allocated at d_plan
    rsp_datatype_t plan_type;
    int nblocks, nlong, nslots;
    int nnz_s;                  // rowptr[rows] seen by the planner
    rsp_plan::SpmvLayout lay;   // byte offsets inside d_plan
    int64_t nnz_c16;            // entries read through 16-bit column offsets or slot indices
    int64_t nnz_staged;         // ... of which in staged tiles (x staged in LDS)
    int64_t local_cols;         // rsp_spmat_set_local_cols (-1: not split)
    int nint;                   // interior tiles at the front of the schedule
    unsigned long long plan_gen;  // unique per plan / value rebind (batch staleness key)
};

struct rsp_ilu0_info {
    int analysed;
    int n, nnz_s;
    const int *rowptr, *colidx;  // device pattern captured at analysis
    int structural_zero;         // -1 = none
    int factored;
    int *d_dpos, *d_hasdiag;
    int *d_upd_ptr, *d_upd_l, *d_upd_u, *d_lord, *d_lend, *d_udiv;
    // d_zero: [0] numerical zero pivot (atomicMin), [1] generation of the
    // last factor call whose flow wait gave up, [2..4] the same for the L,
    // L^T and U solves (rsp::FlowCtl), [6..7] the flow claim counter
    int *d_zero;
    unsigned long long claim_host = 0;  // flow claims issued (rsp::FlowCtl)
    int *d_fdone = nullptr;             // ticket flow launches: per item, the epoch that finished it (rsp::FlowCtl)
    unsigned *d_tk = nullptr;           // ticket flow launches: two slots of counters (rsp::FlowCtl::tickets)
    unsigned long long tk_seq = 0;      // ticket flow launches enqueued (rsp::FlowCtl::tk_seq)
    unsigned flow_epoch = 0;            // epochs handed out (rsp::FlowCtl)
    int solve_gen[3] = {0, 0, 0};       // per solve kind: generation of the last call
    long long n_updates;
    // one level set per DAG: L (factor + L solve), L^T, U
    struct Dag {
        rsp_an::hvec<int> ptr;                  // host level pointers
        int *d_rows = nullptr, *d_ptr = nullptr;
        rsp::RowTask *d_tasks = nullptr;       // solve: task per level-order slot
        int *d_tpos = nullptr, *d_src = nullptr;  // solve: flat terms
        rsp::LevelChunk *d_chunks = nullptr;   // solve: LDS-staged chunks of thin runs
        rsp::ThinRowPlan *d_trow = nullptr;    // solve: thin-run row records
        int *d_sid = nullptr;                  // solve: thin-run y indices per term
        rsp::StagedTerm *d_stg = nullptr;      // solve: thin-run staged terms
        rsp::FlowItem *d_fitems = nullptr;     // solve: flow segments' work items
        int nterms = 0;                        // solve: flat terms
        int *d_nshort = nullptr;               // solve: short rows per level (device)
        rsp_an::hvec<int> nshort;               // (host)
        rsp_an::hvec<int> nwave;                // solve: short + wave rows per level (host)
        rsp_an::hvec<int> sbase;                // solve: padded short rows' first term per level (host)
        rsp_an::hvec<rsp::LevelSeg> segs;       // thread-per-row solve plan
        int batch = 8;                         // solve fma-chain batch
        int group = 4;                         // thin-run term groups (2 or 4)
    } L, LT, U, F;  // F: the factor's one level when fac_one (ptr, d_rows, d_ptr; rsp_an::IluHostPlan::F)
    // block-inverse solve plans of deep L / L^T DAGs (rsp_an::plan_blocks,
    // trsv_blocks.hip); on = false: the level-scheduled solve runs
    struct BlkDag {
        bool on = false;
        int nb = 0, lds_elems = 0, lds_words = 0, entries = 0, nlong = 0;
        rsp_an::hvec<rsp::BlkSeg> segs;  // host
        int *d_order = nullptr, *d_ref = nullptr, *d_vpos = nullptr, *d_lptr = nullptr, *d_rptr = nullptr;
        rsp::BlkDesc *d_desc = nullptr;
        rsp::BlkRow *d_rows = nullptr;
        unsigned *d_eord = nullptr, *d_rit = nullptr;
        void *d_ev = nullptr, *d_yp = nullptr;  // scratch, fp64-sized
        void *d_rc = nullptr;  // block records (fp64-sized: 64 x 144 B per block)
    } Lb, LTb;
    bool fac_one = false, fac_scale = false;  // fac_scale: the factor is ilu0_scale_lower (IluHostPlan::fac_scale)
    const Dag &fdag() const { return fac_one ? F : L; }  // the factor's level sets
    rsp_an::hvec<rsp::LevelSeg> fac_segs;       // wave-per-row factor plan over fdag()
    void *d_sval = nullptr, *d_sx = nullptr, *d_sdg = nullptr;  // solve streams (trsv_stream)
    rsp::RndChunk *d_rchunks = nullptr;        // round-based factor chunks (thin runs)
    rsp::RndItem *d_ritems = nullptr;
    rsp::FacRow *d_frow = nullptr;
    int *d_fslots = nullptr;                   // fat factor levels, slot layout (ilu0_level_slot)
    rsp_an::hvec<rsp::FacFlowRun> fruns;        // factor flow runs (ilu0_flow)
    rsp::FacFlowItem *d_ffitems = nullptr;
    void *d_forig = nullptr;                   // flow rows' upper input values (ilu0_flow_prep), fp64-sized
    int fac_gen = 0;
    rsp_an::hvec<rsp::FacSlotLevel> fslev;      // per factor level (stride 0: FacRow path)
    int *d_rpairs = nullptr, *d_rstaged = nullptr, *d_rrounds = nullptr;
    int fac_batch;
    void *d_arena = nullptr;    // one allocation holding the analysis' arrays (Arena)
    void *d_arena_u = nullptr;  // the U plan's (built on first use)
    void *d_arena_sym = nullptr;    // device analysis: dpos, hasdiag, upd_ptr, lord, lend, udiv, scratch
    void *d_arena_pairs = nullptr;  // device analysis: upd_l, upd_u
    void *d_usval = nullptr;    // U solve term values (trsv_stream), in d_arena_u
    unsigned long long digest = 0;  // rsp_an::digest of the host plan
    std::unique_ptr<rsp_an::IluHostPlan> host;  // kept for the solve plans and the U plan
    rsp_an::hvec<int> host_rp, host_ci;
    // The L and L^T solve plans (the reference's two csrsv2_analysis calls,
    // GPU/ilu0.cu:228-252): built on a worker thread that rsp_ilu0_analysis
    // starts once the levels exist and leaves running; ilu_solves_ready
    // (rsp_trsv_analysis, or the first solve) joins it and uploads them.
    // (Declared after host / host_rp / host_ci, which it reads: destroyed,
    // i.e. joined, before them.)
    std::unique_ptr<rsp_an::Task> solves_task;
    bool solves_ready = false;
    bool dev_terms = true;      // the per-term half of the solve plans is built on the device
    void *d_arena_s = nullptr;  // the solve plans' allocation
    rsp_handle_t han = nullptr; // the handle of the analysis (its stream uploads the solve plans)
    // Recovery of a call whose flow wait gave up (a co-running kernel kept
    // some of the flow launch's workgroups from being scheduled past the
    // give-up bound): rsp_ilu0_zero_pivot / rsp_trsv_zero_pivot re-run it
    // without flow launches (every level its own launch: no co-residency
    // needed), from the factor's input values — copied before every factor
    // that has flow runs — or the solve's unchanged x. RSP_ILU_FLOW_RECOVER=0
    // reports EXECUTION_FAILED instead (the round-4 behaviour).
    // A recovered call's output feeds the calls made after it (the L^T solve
    // reads the L solve's y; a solve reads the factor's values), so those are
    // re-run too, in call order (seq).
    void *d_fbackup = nullptr;
    size_t fbackup_bytes = 0;
    long long call_seq = 0;
    struct FacCall {
        long long seq = 0;
        int valid = 0;
        int ftz = 0;  // the handle's FTZ mode at the call
        rsp_datatype_t type = RSP_R_64F;
        void *vals = nullptr;
    } last_fac;
    struct SolveCall {
        long long seq = 0;
        int valid = 0;
        int ftz = 0;
        rsp_operation_t op = RSP_OPERATION_NON_TRANSPOSE;
        double alpha = 1.0;
        rsp_datatype_t type = RSP_R_64F;
        const void *vals = nullptr, *x = nullptr;
        void *y = nullptr;
    } last_solve[3];
};

#define RSP_CHECK_HIP(call)                                                     \
    do {                                                                        \
        hipError_t e_ = (call);                                                 \
        if (e_ != hipSuccess)                                                   \
            return e_ == hipErrorOutOfMemory ? RSP_STATUS_ALLOC_FAILED          \
                                             : RSP_STATUS_EXECUTION_FAILED;     \
    } while (0)

#define RSP_TRY(call)                                   \
    do {                                                \
        const rsp_status_t st_ = (call);                \
        if (st_ != RSP_STATUS_SUCCESS) return st_;      \
    } while (0)

namespace rsp_api {

using rsp_an::env_int;

// C-ABI entry points never let a C++ exception out (std::bad_alloc from the
// host plans' pools, say): it becomes a status, after `cleanup`.
template <typename F, typename C>
rsp_status_t guarded(F body, C cleanup) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        cleanup();
        return RSP_STATUS_ALLOC_FAILED;
    } catch (...) {
        cleanup();
        return RSP_STATUS_INTERNAL_ERROR;
    }
}
template <typename F>
rsp_status_t guarded(F body) {
    return guarded(body, [] {});
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t elem_size(rsp_datatype_t t) { return t == RSP_R_64F ? 8 : 4; }

// rsp_api.cpp
// Build the schedule of `mat` for `compute_type` into the matrix's own device
// memory (host-blocking; see struct rsp_spmat).
rsp_status_t spmv_plan(rsp_handle_t h, rsp_spmat_t mat, rsp_datatype_t compute_type);
// One SpMV launch (part 0: the whole schedule; 1, 2: rsp_spmv_part).
rsp_status_t spmv_run(rsp_handle_t h, rsp_operation_t op, const void *alpha, rsp_spmat_t mat, const void *d_x,
                      const void *beta, void *d_y, rsp_datatype_t compute_type, void *d_buffer, int part);

// api_ilu_analysis.cpp
// The L and L^T solve plans, joined and uploaded once per analysis; may throw
// what the planning thread threw.
rsp_status_t ilu_solves_ready(rsp_handle_t h, rsp_ilu0_info *f);
// The U DAG's plan, on first use.
rsp_status_t ilu_plan_u(rsp_handle_t h, rsp_ilu0_info *f);

// api_ilu_solve.cpp
// The solves behind rsp_trsv_lower_unit / rsp_trsv_upper (flow_ok = false: the
// recovery run, no flow launch).
rsp_status_t rsp_trsv_lower_unit_impl(rsp_handle_t h, rsp_operation_t op, const void *alpha, rsp_ilu0_info_t f,
                                      rsp_datatype_t value_type, const void *d_values, const void *d_x, void *d_y,
                                      bool flow_ok);
rsp_status_t rsp_trsv_upper_impl(rsp_handle_t h, const void *alpha, rsp_ilu0_info_t f, rsp_datatype_t value_type,
                                 const void *d_values, const void *d_x, void *d_y, bool flow_ok);

}  // namespace rsp_api
