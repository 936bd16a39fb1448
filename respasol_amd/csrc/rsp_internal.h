// rsp_internal.h — what the host units of librsp.so share: the three structs
// behind the opaque handles of include/rsp.h (the ILU(0) info is the state of
// one analysis, reset whole by the next), the status macros, guarded() and the
// few functions one unit calls in another (namespace rsp_api).
//   rsp_api.cpp           handle, matrix descriptor, SpMV (plan upload, run, batch)
//   spmv_plan.cpp         the SpMV planner (spmv_plan.h; no HIP calls)
//   csr_transpose.cpp     the pattern transposer (csr_transpose.h; no HIP calls)
//   api_ilu_analysis.cpp  ILU(0) analysis, the solve plans, the plan queries
//   api_ilu_solve.cpp     factor and triangular solves, flow give-up recovery
//   api_krylov.cpp        BiCGStab, CG, GMRES, rsp_dot, rsp_orthogonalize, iterative refinement
//   api_cheby.cpp         the Chebyshev polynomial preconditioner
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
#include "csr_transpose.h"

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
struct rsp_spmat_tside;
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
    rsp_spmat_tside *tside;     // the transposed side, built by the first op = TRANSPOSE use (else null)
};

// A hipMalloc'ed allocation, freed with its owner (move-only).
struct DevMem {
    void *p = nullptr;
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem &operator=(DevMem &&o) noexcept {
        std::swap(p, o.p);  // (the old allocation goes with o)
        return *this;
    }
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
};

// What rsp_spmv(op = TRANSPOSE) keeps in a matrix: the CSR pattern of A^T in
// the order of csr_transpose.h, the permutation that carries A's values into
// it, the permuted values (refilled by every call) and a descriptor over them
// whose schedule spmv_plan builds as for any matrix. Host-blocking to build
// (rsp_api.cpp tside_build); freed on the device it was built on.
struct rsp_spmat_tside {
    int device = 0;
    DevMem pattern;  // [t_rowptr (cols + 1) | t_colidx (nnz_s) | perm (nnz_s)], each 256-B aligned
    DevMem vt;       // nnz_s values of child.type
    int *perm = nullptr;
    rsp_spmat child{};  // A^T: cols x rows over pattern and vt; its d_plan is freed here
    rsp_spmat_tside() = default;
    rsp_spmat_tside(const rsp_spmat_tside &) = delete;
    rsp_spmat_tside &operator=(const rsp_spmat_tside &) = delete;
    ~rsp_spmat_tside() {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        if (child.d_plan) (void)hipFree(child.d_plan);
        pattern = DevMem();
        vt = DevMem();
        (void)hipSetDevice(cur);
    }
};

// Everything one rsp_ilu0_analysis produces and the calls on it change:
// nothing in the info outlives an analysis, and reset() drops it.
// Each plan array's device pointer lives in the kernel-argument struct it is
// passed in (fac, Dag::plan, BlkDag::args), filled where the array is uploaded.
// Member order is the destruction order's reverse: the planning task is
// declared after host / host_rp / host_ci, which it reads, so it is destroyed
// (joined) before them; nothing depends on the order of the rest.
struct rsp_ilu0_info {
    int analysed = 0, factored = 0;
    int n = 0, nnz_s = 0;
    int structural_zero = -1;  // -1 = none
    rsp_handle_t han = nullptr;  // the handle of the analysis (its stream uploads the solve plans)
    long long n_updates = 0;
    // The factor's arguments but for those of one call (ilu_factor_run): the
    // pattern captured at analysis, the symbolic arrays, the factor plan.
    rsp::IluArgs fac{};
    // d_zero: [0] numerical zero pivot (atomicMin), [1] generation of the
    // last factor call whose flow wait gave up, [2..4] the same for the L,
    // L^T and U solves (rsp::FlowCtl), [6..7] the flow claim counter
    int *d_zero = nullptr;
    unsigned long long claim_host = 0;  // flow claims issued (rsp::FlowCtl)
    int *d_fdone = nullptr;             // ticket flow launches: per item, the epoch that finished it (rsp::FlowCtl)
    unsigned *d_tk = nullptr;           // ticket flow launches: two slots of counters (rsp::FlowCtl::tickets)
    unsigned long long tk_seq = 0;      // ticket flow launches enqueued (rsp::FlowCtl::tk_seq)
    unsigned flow_epoch = 0;            // epochs handed out (rsp::FlowCtl)
    int fac_gen = 0;
    int solve_gen[3] = {0, 0, 0};       // per solve kind: generation of the last call
    // one level set per DAG: L (factor + L solve), L^T, U
    struct Dag {
        rsp::LevelPlan plan{};                  // the device arrays (the host fields: level_plan, per call)
        rsp_an::hvec<int> ptr;                  // host level pointers
        int nterms = 0;                         // solve: flat terms
        rsp_an::hvec<int> nshort;               // solve: short rows per level
        rsp_an::hvec<int> nwave;                // solve: short + wave rows per level
        rsp_an::hvec<int> sbase;                // solve: padded short rows' first term per level
        rsp_an::hvec<rsp::LevelSeg> segs;       // thread-per-row solve plan
        int batch = 8;                          // solve fma-chain batch
        int group = 4;                          // thin-run term groups (2 or 4)
    } L, LT, U, F;  // F: the factor's one level when fac_one (ptr, rows, ptr_dev; rsp_an::IluHostPlan::F)
    // block-inverse solve plans of deep L / L^T DAGs (rsp_an::plan_blocks,
    // trsv_blocks.hip); on = false: the level-scheduled solve runs
    struct BlkDag {
        bool on = false;
        rsp::BlkArgs args{};             // the plan and its scratch (the call's fields: the solve)
        rsp_an::hvec<rsp::BlkSeg> segs;  // host
    } Lb, LTb;
    bool fac_one = false;  // the factor walks F (fac.fac_one: it is ilu0_scale_lower, IluHostPlan::fac_scale)
    const Dag &fdag() const { return fac_one ? F : L; }  // the factor's level sets
    rsp_an::hvec<rsp::LevelSeg> fac_segs;       // wave-per-row factor plan over fdag()
    int fac_batch = 8;
    rsp_an::hvec<rsp::FacFlowRun> fruns;        // factor flow runs (ilu0_flow)
    rsp_an::hvec<rsp::FacSlotLevel> fslev;      // per factor level (stride 0: FacRow path)
    void *d_sval = nullptr, *d_sx = nullptr, *d_sdg = nullptr;  // solve streams (trsv_stream)
    void *d_usval = nullptr;    // U solve term values (trsv_stream), in arena_u
    DevMem arena;        // one allocation holding the analysis' arrays (Arena)
    DevMem arena_sym;    // device analysis: dpos, hasdiag, upd_ptr, lord, lend, udiv, scratch
    DevMem arena_pairs;  // device analysis: upd_l, upd_u
    DevMem arena_s;      // the solve plans'
    DevMem arena_u;      // the U plan's (built on first use)
    DevMem fslots;       // fat factor levels, slot layout (ilu0_level_slot; fac.fslots once built)
    unsigned long long digest = 0;  // rsp_an::digest of the host plan (RSP_ILU_DIGEST; 0: none)
    std::unique_ptr<rsp_an::IluHostPlan> host;  // kept for the solve plans and the U plan
    rsp_an::hvec<int> host_rp, host_ci;
    // The L and L^T solve plans (the reference's two csrsv2_analysis calls,
    // GPU/ilu0.cu:228-252): built on a worker thread that rsp_ilu0_analysis
    // starts once the levels exist and leaves running; ilu_solves_ready
    // (rsp_trsv_analysis, or the first solve) joins it and uploads them.
    std::unique_ptr<rsp_an::Task> solves_task;
    bool solves_ready = false;
    bool dev_terms = true;      // the per-term half of the solve plans is built on the device
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
    DevMem fbackup;
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

    // Drop the analysis: as rsp_create_ilu0_info made it. (Never by a bare
    // assignment: memberwise, that frees the buffers before joining the task.)
    void reset() {
        solves_task.reset();
        *this = rsp_ilu0_info();
    }
};

// A Chebyshev polynomial preconditioner (api_cheby.cpp; include/rsp.h): the
// matrix it is built on (of type P), the bounds, the coefficients rounded to P
// and one allocation holding dinv (JACOBI only) and the work vectors d and w.
struct rsp_cheby {
    int device = 0;
    rsp_spmat_t A = nullptr;
    rsp_datatype_t P = RSP_R_64F;
    long long n = 0;
    int degree = 1;
    double lmin = 0.0, lmax = 0.0;
    double c0 = 0.0, a[RSP_CHEBY_MAX_DEGREE] = {}, b[RSP_CHEBY_MAX_DEGREE] = {};  // values of P; a[j], b[j]: term j
    void *d_mem = nullptr;
    void *dinv = nullptr, *d = nullptr, *w = nullptr;  // dinv null: RSP_CHEBY_SCALE_NONE
    ~rsp_cheby() {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        if (d_mem) (void)hipFree(d_mem);
        (void)hipSetDevice(cur);
    }
};

#define RSP_CHECK_HIP(call)                                                    \
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
rsp_status_t rsp_trsv_lower_unit_impl(rsp_handle_t h, rsp_operation_t op, const void *alpha, rsp_ilu0_info *f,
                                      rsp_datatype_t value_type, const void *d_values, const void *d_x, void *d_y,
                                      bool flow_ok);
rsp_status_t rsp_trsv_upper_impl(rsp_handle_t h, const void *alpha, rsp_ilu0_info *f, rsp_datatype_t value_type,
                                 const void *d_values, const void *d_x, void *d_y, bool flow_ok);

// api_cheby.cpp
// z = p_k(D^-1 A) D^-1 r on the handle's stream (rsp_cheby_apply without the guard).
rsp_status_t cheby_apply(rsp_handle_t h, rsp_cheby *c, const void *d_r, void *d_z);

}  // namespace rsp_api
