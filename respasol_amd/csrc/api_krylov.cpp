// api_krylov.cpp — the Krylov solvers of include/rsp.h: BiCGStab, CG and
// restarted flexible GMRES(m) preconditioned by ILU(0) or by the Chebyshev
// polynomial of api_cheby.cpp (the *_create_cheby calls), and the building
// blocks they expose (rsp_dot, rsp_orthogonalize, rsp_gmres_lsq_host), and
// mixed-precision iterative refinement over them (rsp_refine_*,
// rsp_convert_scaled, rsp_refine_update). Host
// loops over the kernels of krylov.hip, spmv_run (rsp_api.cpp) and the
// triangular solves (api_ilu_solve.cpp); what the solvers share is KrylovCommon.

#include "rsp_internal.h"

using namespace rsp_api;

/* ------------------------------------------------- what both solvers share */

// The operator, the preconditioner (M = L U of info, or the polynomial cheby;
// both null: M = I) and its apply's buffers, the device block and the pinned
// mirror the checks land in.
struct KrylovCommon {
    int device = 0;
    rsp_spmat_t A = nullptr;
    rsp_ilu0_info_t info = nullptr;  // M = L U
    rsp_cheby_t cheby = nullptr;     // M^-1 = the polynomial (never with info); both null: M = I
    rsp_datatype_t T = RSP_R_64F, P = RSP_R_64F;
    const void *factor = nullptr;
    long long n = 0;
    void *d_arena = nullptr;  // [device block | the solver's type-T vectors | the apply's type-P vectors]
    void *pin = nullptr, *pmid = nullptr, *pout = nullptr;  // the preconditioner's input / L result / U result (type P)
    double *d_blk = nullptr;
    double *h_pin = nullptr;
    hipEvent_t ev = nullptr;
    std::vector<double> history;
    int gen0[2] = {0, 0};  // the L and U solves' generations when the running solve call began
    bool precond() const { return info || cheby; }
    bool mixed() const { return precond() && P != T; }
    int kry_type() const { return T == RSP_R_32F ? rsp::kKryF32 : (mixed() ? rsp::kKryF64Copy32 : rsp::kKryF64); }
    size_t tbytes() const { return align256((size_t)n * elem_size(T)); }  // one type-T vector in the arena
    ~KrylovCommon() {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        if (d_arena) (void)hipFree(d_arena);
        if (h_pin) (void)hipHostFree(h_pin);
        if (ev) (void)hipEventDestroy(ev);
        (void)hipSetDevice(cur);
    }
};

static const double kOne64 = 1.0, kZero64 = 0.0;
static const float kOne32 = 1.0f, kZero32 = 0.0f;
static const void *one_of(rsp_datatype_t t) { return t == RSP_R_64F ? (const void *)&kOne64 : (const void *)&kOne32; }
static const void *zero_of(rsp_datatype_t t) { return t == RSP_R_64F ? (const void *)&kZero64 : (const void *)&kZero32; }

// What both solvers' create calls check and finish before they allocate: the
// arguments, A's schedule, the L and U solve plans, the factor's zero pivot.
static rsp_status_t krylov_create_checks(rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info,
                                         rsp_datatype_t precond_type, const void *d_factor, rsp_cheby_t cheby) {
    if (!A || A->rows != A->cols || A->rows < 1) return RSP_STATUS_INVALID_VALUE;
    if (cheby && (cheby->n != A->rows || (A->type == RSP_R_32F && cheby->P == RSP_R_64F)))
        return RSP_STATUS_INVALID_VALUE;
    if (info) {
        if (precond_type != RSP_R_64F && precond_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
        if (!info->analysed || info->n != A->rows || !d_factor) return RSP_STATUS_INVALID_VALUE;
        if (A->type == RSP_R_32F && precond_type == RSP_R_64F) return RSP_STATUS_INVALID_VALUE;
    }
    if (!A->planned || A->plan_type != A->type) RSP_TRY(spmv_plan(h, A, A->type));
    if (info) {
        RSP_TRY(ilu_solves_ready(h, info));
        RSP_TRY(ilu_plan_u(h, info));
        int pos = -1;
        RSP_TRY(rsp_ilu0_zero_pivot(h, info, &pos));  // U divides by its diagonal
    }
    return RSP_STATUS_SUCCESS;
}

// The checked arguments into a new solver.
static void krylov_bind(KrylovCommon &s, rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info,
                        rsp_datatype_t precond_type, const void *d_factor, rsp_cheby_t cheby) {
    s.device = h->device;
    s.A = A;
    s.info = info;
    s.cheby = cheby;
    s.T = A->type;
    s.P = cheby ? cheby->P : (info ? precond_type : A->type);
    s.factor = d_factor;
    s.n = A->rows;
}

// The solver's one allocation: the device block of `blk` bytes, `tvec_bytes`
// of type-T vectors (returned in *tvecs for the solver to lay out) and, at the
// tail, the apply's type-P vectors (with M = L U: pmid; mixed: pin, pmid, pout;
// the polynomial has its own work vectors: mixed only, pin and pout).
// Then the pinned mirror of `mirror_doubles` and the event of the checks.
static rsp_status_t krylov_alloc(KrylovCommon &s, size_t blk, size_t tvec_bytes, size_t mirror_doubles,
                                 char **tvecs) {
    const size_t pb = align256((size_t)s.n * elem_size(s.P));
    const int nmid = s.info ? 1 : 0;
    const int np = s.mixed() ? 2 + nmid : nmid;
    RSP_CHECK_HIP(hipMalloc(&s.d_arena, blk + tvec_bytes + np * pb));
    char *at = (char *)s.d_arena;
    s.d_blk = (double *)at;
    *tvecs = at + blk;
    at += blk + tvec_bytes;
    if (s.mixed()) {
        s.pin = at;
        s.pmid = nmid ? at + pb : nullptr;
        s.pout = at + (1 + nmid) * pb;
    } else if (s.info) {
        s.pmid = at;
    }
    RSP_CHECK_HIP(hipHostMalloc((void **)&s.h_pin, mirror_doubles * sizeof(double), hipHostMallocDefault));
    RSP_CHECK_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    return RSP_STATUS_SUCCESS;
}

static rsp_status_t krylov_spmv(rsp_handle_t h, const KrylovCommon &s, const void *x, void *y) {
    return spmv_run(h, RSP_OPERATION_NON_TRANSPOSE, one_of(s.T), s.A, x, zero_of(s.T), y, s.T, nullptr, 0);
}

// z = M^-1 y with M = L U: y -> L -> pmid -> U -> z, or the polynomial's apply;
// in mixed mode y's fp32 copy (written by the kernel that made y) is the input
// and the fp32 result is widened into z for the fp64 SpMV.
static rsp_status_t krylov_apply(rsp_handle_t h, const KrylovCommon &s, const void *y, void *z, bool ftz) {
    const void *one = one_of(s.P);
    const void *in = s.mixed() ? s.pin : y;
    void *res = s.mixed() ? s.pout : z;
    if (s.cheby) {
        RSP_TRY(cheby_apply(h, s.cheby, in, res));
    } else {
        RSP_TRY(rsp_trsv_lower_unit_impl(h, RSP_OPERATION_NON_TRANSPOSE, one, s.info, s.P, s.factor, in, s.pmid, true));
        RSP_TRY(rsp_trsv_upper_impl(h, one, s.info, s.P, s.factor, s.pmid, res, true));
    }
    if (!s.mixed()) return RSP_STATUS_SUCCESS;
    rsp::KryArgs a{};
    a.n = s.n;
    a.blk = s.d_blk;
    a.b = res;
    a.copy32 = z;
    const hipError_t e = ftz ? rsp_k_ftz::krylov(rsp::kKryWiden, rsp::kKryF64Copy32, a, h->stream)
                             : rsp_k::krylov(rsp::kKryWiden, rsp::kKryF64Copy32, a, h->stream);
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

// A solve call's argument checks and the initial state of its outputs.
static rsp_status_t krylov_solve_begin(rsp_handle_t h, KrylovCommon *s, const void *d_b, void *d_x, double rtol,
                                       int max_iters, int check_every, int *iters, double *relres,
                                       rsp_solve_reason_t *reason) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!s || !d_b || !d_x || !iters || !relres || !reason) return RSP_STATUS_INVALID_VALUE;
    if (max_iters < 0 || check_every < 1 || !(rtol >= 0.0)) return RSP_STATUS_INVALID_VALUE;
    *iters = 0;
    *relres = 0.0;
    *reason = RSP_SOLVE_MAX_ITERS;
    s->history.clear();
    s->gen0[0] = s->info ? s->info->solve_gen[RSP_TRSV_L] : 0;
    s->gen0[1] = s->info ? s->info->solve_gen[RSP_TRSV_U] : 0;
    return RSP_STATUS_SUCCESS;
}

// cusparseXcsrsv2_zeroPivot of the L and U solves, for every apply of a solve
// call (of `iters` iterations) at once: a flow launch that gave up a wait left
// its generation in the solve's status word. The solver's buffers are reused
// every iteration, so the recovery of rsp_trsv_zero_pivot (re-running the
// recorded solves) cannot apply: reported. (A polynomial has nothing to read.)
static rsp_status_t krylov_solve_end(rsp_handle_t h, const KrylovCommon &s, int iters) {
    if (!s.info || iters <= 0) return RSP_STATUS_SUCCESS;
    int z[5];
    RSP_CHECK_HIP(hipMemcpyAsync(z, s.info->d_zero, sizeof(z), hipMemcpyDeviceToHost, h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    if (z[2 + RSP_TRSV_L] > s.gen0[0] || z[2 + RSP_TRSV_U] > s.gen0[1]) return RSP_STATUS_EXECUTION_FAILED;
    return RSP_STATUS_SUCCESS;
}

static rsp_status_t krylov_history(const KrylovCommon *s, int cap, double *relres, int *count) {
    if (!s || !count || cap < 0 || (cap > 0 && !relres)) return RSP_STATUS_INVALID_VALUE;
    *count = (int)s->history.size();
    for (int k = 0; k < cap && k < *count; k++) relres[k] = s->history[k];
    return RSP_STATUS_SUCCESS;
}

/* ------------------------------------------------------ BiCGStab + dot */

// One solver: the work vectors, the scalar / partial block (rsp::kKry*) and
// the pinned mirror (kKryScalars + 2 kKryMaxGrid doubles) the convergence
// read-back lands in.
struct rsp_bicgstab : KrylovCommon {
    void *r = nullptr, *rhat = nullptr, *p = nullptr, *v = nullptr, *s = nullptr, *t = nullptr;
    void *phat = nullptr, *shat = nullptr;  // type T (M = I: p and s themselves)
};

static rsp_status_t bicgstab_create(rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info,
                                    rsp_datatype_t precond_type, const void *d_factor, rsp_cheby_t cheby,
                                    rsp_bicgstab_t *out) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!out) return RSP_STATUS_INVALID_VALUE;
    *out = nullptr;
    RSP_TRY(krylov_create_checks(h, A, info, precond_type, d_factor, cheby));
    std::unique_ptr<rsp_bicgstab> s(new rsp_bicgstab);  // (a half-built solver is freed on every way out)
    krylov_bind(*s, h, A, info, precond_type, d_factor, cheby);
    // r, rhat, p, v, s, t; with M: phat, shat (T) and the apply's vectors (P)
    const size_t tb = s->tbytes();
    const int nt = s->precond() ? 8 : 6;
    char *at = nullptr;
    RSP_TRY(krylov_alloc(*s, align256(rsp::kKryBlockDoubles * sizeof(double)), nt * tb,
                         rsp::kKryScalars + 2 * (size_t)rsp::kKryMaxGrid, &at));
    void **tv[] = {&s->r, &s->rhat, &s->p, &s->v, &s->s, &s->t, &s->phat, &s->shat};
    for (int k = 0; k < nt; k++, at += tb) *tv[k] = at;
    if (!s->precond()) {
        s->phat = s->p;
        s->shat = s->s;
    }
    *out = s.release();
    return RSP_STATUS_SUCCESS;
}

static rsp_status_t bicgstab_solve(rsp_handle_t h, rsp_bicgstab_t s, const void *d_b, void *d_x, double rtol,
                                   int max_iters, int check_every, int *iters, double *relres,
                                   rsp_solve_reason_t *reason) {
    RSP_TRY(krylov_solve_begin(h, s, d_b, d_x, rtol, max_iters, check_every, iters, relres, reason));
    s->history.reserve((size_t)max_iters / check_every + 2);
    const int type = s->kry_type();
    const bool ftz = h->ftz != 0 && type != rsp::kKryF64;
    const int G = rsp::kry_grid(s->n).grid;
    rsp::KryArgs a{};
    a.n = s->n;
    a.blk = s->d_blk;
    a.b = d_b;
    a.x = d_x;
    a.r = s->r;
    a.rhat = s->rhat;
    a.p = s->p;
    a.v = s->v;
    a.s = s->s;
    a.t = s->t;
    a.phat = s->phat;
    a.shat = s->shat;
    a.copy32 = s->mixed() ? s->pin : nullptr;
    auto kern = [&](rsp::KryOp op) {
        const hipError_t e = ftz ? rsp_k_ftz::krylov(op, type, a, h->stream) : rsp_k::krylov(op, type, a, h->stream);
        return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
    };
    // the one host wait of an iteration: scalars + the (r,r) partials, one
    // async copy into the pinned mirror, one event
    double *hp = s->h_pin;
    auto read_back = [&]() -> rsp_status_t {
        RSP_CHECK_HIP(hipMemcpyAsync(hp, s->d_blk, (rsp::kKryScalars + (size_t)G) * sizeof(double),
                                     hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipEventRecord(s->ev, h->stream));
        RSP_CHECK_HIP(hipEventSynchronize(s->ev));
        return RSP_STATUS_SUCCESS;
    };
    // r = b - A x0, rhat = r, (b,b), (r,r)
    RSP_TRY(krylov_spmv(h, *s, d_x, s->v));
    RSP_TRY(kern(rsp::kKryInit));
    RSP_CHECK_HIP(hipMemcpyAsync(hp + rsp::kKryScalars + rsp::kKryMaxGrid,
                                 s->d_blk + rsp::kKryScalars + (size_t)rsp::kKryPartBB * rsp::kKryMaxGrid,
                                 (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RSP_TRY(read_back());
    const double bb = rsp::kry_combine_host(hp + rsp::kKryScalars + rsp::kKryMaxGrid, G);
    double rr = rsp::kry_combine_host(hp + rsp::kKryScalars, G);
    const double bnorm = sqrt(bb);
    if (bb == 0.0) {  // x = 0 solves it
        RSP_TRY(kern(rsp::kKryZero));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        *reason = RSP_SOLVE_CONVERGED;
        return RSP_STATUS_SUCCESS;
    }
    if (!std::isfinite(bb) || !std::isfinite(rr)) {  // b or x0 not finite: nothing to iterate on
        *relres = sqrt(rr) / bnorm;
        *reason = RSP_SOLVE_BREAKDOWN;
        return RSP_STATUS_SUCCESS;
    }
    double rel = sqrt(rr) / bnorm;
    *relres = rel;
    int done = 0;
    if (rel <= rtol) {
        *reason = RSP_SOLVE_CONVERGED;
    } else {
        for (int it = 1; it <= max_iters; it++) {
            a.it = it;
            RSP_TRY(kern(rsp::kKryPUpdate));
            if (s->precond()) RSP_TRY(krylov_apply(h, *s, s->p, s->phat, ftz));
            RSP_TRY(krylov_spmv(h, *s, s->phat, s->v));
            RSP_TRY(kern(rsp::kKryDotRhV));
            RSP_TRY(kern(rsp::kKrySUpdate));
            if (s->precond()) RSP_TRY(krylov_apply(h, *s, s->s, s->shat, ftz));
            RSP_TRY(krylov_spmv(h, *s, s->shat, s->t));
            RSP_TRY(kern(rsp::kKryDotTS));
            RSP_TRY(kern(rsp::kKryXUpdate));
            done = it;
            if (it % check_every != 0 && it != max_iters) continue;
            RSP_TRY(read_back());
            rr = rsp::kry_combine_host(hp + rsp::kKryScalars, G);
            rel = sqrt(rr) / bnorm;
            const int flag = (int)hp[rsp::kKryFlag];
            if (flag) done = (int)hp[rsp::kKryFlagIt] - 1;  // x, r and p stand as that iteration found them
            s->history.push_back(rel);
            if (rel <= rtol) {
                *reason = RSP_SOLVE_CONVERGED;
                break;
            }
            if (flag) {
                *reason = RSP_SOLVE_BREAKDOWN;
                break;
            }
        }
    }
    *iters = done;
    *relres = rel;
    return krylov_solve_end(h, *s, done);
}

static rsp_status_t krylov_dot(rsp_handle_t h, rsp_datatype_t value_type, int64_t n, const void *d_x, const void *d_y,
                               double *result) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (!result || n < 0 || (n > 0 && (!d_x || !d_y))) return RSP_STATUS_INVALID_VALUE;
    *result = 0.0;
    if (n == 0) return RSP_STATUS_SUCCESS;
    if (!h->d_dot) RSP_CHECK_HIP(hipMalloc((void **)&h->d_dot, rsp::kKryBlockDoubles * sizeof(double)));
    if (!h->h_dot)
        RSP_CHECK_HIP(hipHostMalloc((void **)&h->h_dot, rsp::kKryMaxGrid * sizeof(double), hipHostMallocDefault));
    rsp::KryArgs a{};
    a.n = n;
    a.blk = h->d_dot;
    a.b = d_x;
    a.c = d_y;
    const int type = value_type == RSP_R_64F ? rsp::kKryF64 : rsp::kKryF32;
    const hipError_t e = (h->ftz && type == rsp::kKryF32) ? rsp_k_ftz::krylov(rsp::kKryDot, type, a, h->stream)
                                                          : rsp_k::krylov(rsp::kKryDot, type, a, h->stream);
    if (e != hipSuccess) return RSP_STATUS_EXECUTION_FAILED;
    const int G = rsp::kry_grid(n).grid;
    RSP_CHECK_HIP(hipMemcpyAsync(h->h_dot, h->d_dot + rsp::kKryScalars + (size_t)rsp::kKryPartRR * rsp::kKryMaxGrid,
                                 (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    *result = rsp::kry_combine_host(h->h_dot, G);
    return RSP_STATUS_SUCCESS;
}

/* ------------------------------------------------------------------- CG */

// One solver: r, p, q and, with M, z (type T); the scalar / partial block and
// the pinned mirror are BiCGStab's.
struct rsp_cg : KrylovCommon {
    void *r = nullptr, *p = nullptr, *q = nullptr;
    void *z = nullptr;  // M = I: r itself
};

static rsp_status_t cg_create(rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info, rsp_datatype_t precond_type,
                              const void *d_factor, rsp_cheby_t cheby, rsp_cg_t *out) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!out) return RSP_STATUS_INVALID_VALUE;
    *out = nullptr;
    RSP_TRY(krylov_create_checks(h, A, info, precond_type, d_factor, cheby));
    std::unique_ptr<rsp_cg> s(new rsp_cg);  // (a half-built solver is freed on every way out)
    krylov_bind(*s, h, A, info, precond_type, d_factor, cheby);
    const size_t tb = s->tbytes();
    const int nt = s->precond() ? 4 : 3;
    char *at = nullptr;
    RSP_TRY(krylov_alloc(*s, align256(rsp::kKryBlockDoubles * sizeof(double)), nt * tb,
                         rsp::kKryScalars + 2 * (size_t)rsp::kKryMaxGrid, &at));
    void **tv[] = {&s->r, &s->p, &s->q, &s->z};
    for (int k = 0; k < nt; k++, at += tb) *tv[k] = at;
    if (!s->precond()) s->z = s->r;
    *out = s.release();
    return RSP_STATUS_SUCCESS;
}

static rsp_status_t cg_solve(rsp_handle_t h, rsp_cg_t s, const void *d_b, void *d_x, double rtol, int max_iters,
                             int check_every, int *iters, double *relres, rsp_solve_reason_t *reason) {
    RSP_TRY(krylov_solve_begin(h, s, d_b, d_x, rtol, max_iters, check_every, iters, relres, reason));
    s->history.reserve((size_t)max_iters / check_every + 2);
    const int type = s->kry_type();
    const bool ftz = h->ftz != 0 && type != rsp::kKryF64;
    const int G = rsp::kry_grid(s->n).grid;
    rsp::KryArgs a{};
    a.n = s->n;
    a.blk = s->d_blk;
    a.b = d_b;
    a.x = d_x;
    a.r = s->r;
    a.z = s->z;
    a.p = s->p;
    a.v = s->q;
    a.copy32 = s->mixed() ? s->pin : nullptr;
    auto kern = [&](rsp::KryOp op) {
        const hipError_t e = ftz ? rsp_k_ftz::krylov(op, type, a, h->stream) : rsp_k::krylov(op, type, a, h->stream);
        return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
    };
    // the one host wait of an iteration, as bicgstab_solve's
    double *hp = s->h_pin;
    auto read_back = [&]() -> rsp_status_t {
        RSP_CHECK_HIP(hipMemcpyAsync(hp, s->d_blk, (rsp::kKryScalars + (size_t)G) * sizeof(double),
                                     hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipEventRecord(s->ev, h->stream));
        RSP_CHECK_HIP(hipEventSynchronize(s->ev));
        return RSP_STATUS_SUCCESS;
    };
    // r = b - A x0 (mixed: and its fp32 copy), (b,b), (r,r)
    RSP_TRY(krylov_spmv(h, *s, d_x, s->q));
    RSP_TRY(kern(rsp::kKryCgInit));
    RSP_CHECK_HIP(hipMemcpyAsync(hp + rsp::kKryScalars + rsp::kKryMaxGrid,
                                 s->d_blk + rsp::kKryScalars + (size_t)rsp::kKryPartBB * rsp::kKryMaxGrid,
                                 (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RSP_TRY(read_back());
    const double bb = rsp::kry_combine_host(hp + rsp::kKryScalars + rsp::kKryMaxGrid, G);
    double rr = rsp::kry_combine_host(hp + rsp::kKryScalars, G);
    const double bnorm = sqrt(bb);
    if (bb == 0.0) {  // x = 0 solves it
        RSP_TRY(kern(rsp::kKryZero));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        *reason = RSP_SOLVE_CONVERGED;
        return RSP_STATUS_SUCCESS;
    }
    if (!std::isfinite(bb) || !std::isfinite(rr)) {  // b or x0 not finite: nothing to iterate on
        *relres = sqrt(rr) / bnorm;
        *reason = RSP_SOLVE_BREAKDOWN;
        return RSP_STATUS_SUCCESS;
    }
    double rel = sqrt(rr) / bnorm;
    *relres = rel;
    int done = 0;
    if (rel <= rtol) {
        *reason = RSP_SOLVE_CONVERGED;
    } else {
        for (int it = 1; it <= max_iters; it++) {
            a.it = it;
            if (s->precond()) {
                RSP_TRY(krylov_apply(h, *s, s->r, s->z, ftz));
                RSP_TRY(kern(rsp::kKryCgDotRZ));
            }
            RSP_TRY(kern(rsp::kKryCgPUpdate));
            RSP_TRY(krylov_spmv(h, *s, s->p, s->q));
            RSP_TRY(kern(rsp::kKryCgDotPQ));
            RSP_TRY(kern(rsp::kKryCgXUpdate));
            done = it;
            if (it % check_every != 0 && it != max_iters) continue;
            RSP_TRY(read_back());
            rr = rsp::kry_combine_host(hp + rsp::kKryScalars, G);
            rel = sqrt(rr) / bnorm;
            const int flag = (int)hp[rsp::kKryFlag];
            if (flag) done = (int)hp[rsp::kKryFlagIt] - 1;  // x and r stand as that iteration found them
            s->history.push_back(rel);
            if (rel <= rtol) {  // (before the flag: r == 0 exactly is flagged by the next iteration's rho)
                *reason = RSP_SOLVE_CONVERGED;
                break;
            }
            if (flag) {
                *reason = RSP_SOLVE_BREAKDOWN;
                break;
            }
        }
    }
    *iters = done;
    *relres = rel;
    return krylov_solve_end(h, *s, done);
}

/* ------------------------------------------------ FGMRES + orthogonalize */

// One solver: the basis V (m + 1 columns), w and Z (m columns, with M), the
// device block (rsp::kGm*) and the pinned mirror (kGmHead + 2 kKryMaxGrid
// doubles) the checks land in.
struct rsp_gmres : KrylovCommon {
    long long ld = 0;  // elements between columns of V / Z
    int m = 0;
    char *V = nullptr, *Z = nullptr;  // (M = I: Z = V)
    void *w = nullptr;
};

static rsp_status_t gmres_create(rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info, rsp_datatype_t precond_type,
                                 const void *d_factor, rsp_cheby_t cheby, int restart, rsp_gmres_t *out) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!out) return RSP_STATUS_INVALID_VALUE;
    *out = nullptr;
    if (restart < 1 || restart > RSP_GMRES_MAX_RESTART) return RSP_STATUS_INVALID_VALUE;
    RSP_TRY(krylov_create_checks(h, A, info, precond_type, d_factor, cheby));
    std::unique_ptr<rsp_gmres> s(new rsp_gmres);  // (a half-built solver is freed on every way out)
    krylov_bind(*s, h, A, info, precond_type, d_factor, cheby);
    s->m = restart;
    const size_t tb = s->tbytes();
    s->ld = (long long)(tb / elem_size(s->T));
    // V (m + 1), w; with M: Z (m) and the apply's vectors (P)
    const size_t nt = (size_t)s->m + 2 + (s->precond() ? s->m : 0);
    char *at = nullptr;
    RSP_TRY(krylov_alloc(*s, align256(rsp::kGmBlockDoubles * sizeof(double)), nt * tb,
                         rsp::kGmHead + 2 * (size_t)rsp::kKryMaxGrid, &at));
    s->V = at;
    at += ((size_t)s->m + 1) * tb;
    s->w = at;
    at += tb;
    s->Z = s->precond() ? at : s->V;
    *out = s.release();
    return RSP_STATUS_SUCCESS;
}

static rsp_status_t gmres_solve(rsp_handle_t h, rsp_gmres_t s, const void *d_b, void *d_x, double rtol,
                                int max_iters, int check_every, int *iters, double *relres,
                                rsp_solve_reason_t *reason) {
    RSP_TRY(krylov_solve_begin(h, s, d_b, d_x, rtol, max_iters, check_every, iters, relres, reason));
    s->history.reserve((size_t)max_iters / check_every + (size_t)max_iters / s->m + 2);
    const int type = s->kry_type();
    const bool ftz = h->ftz != 0 && type != rsp::kKryF64;
    const int G = rsp::kry_grid(s->n).grid;
    const size_t tb = (size_t)s->ld * elem_size(s->T);
    rsp::GmArgs a{};
    a.n = s->n;
    a.blk = s->d_blk;
    a.b = d_b;
    a.x = d_x;
    a.V = s->V;
    a.ldv = s->ld;
    a.Z = s->Z;
    a.ldz = s->ld;
    a.w = s->w;
    a.copy32 = s->mixed() ? s->pin : nullptr;
    auto kern = [&](rsp::GmOp op, int j, int first) {
        a.j = j;
        a.first = first;
        const hipError_t e = ftz ? rsp_k_ftz::gmres(op, type, a, h->stream) : rsp_k::gmres(op, type, a, h->stream);
        return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
    };
    // a check: the head (scalars + estimates), at a cycle end the (r,r)
    // partials too; async copies into the pinned mirror, one event
    double *hp = s->h_pin;
    auto read_back = [&](bool rr, bool bb) -> rsp_status_t {
        RSP_CHECK_HIP(hipMemcpyAsync(hp, s->d_blk, rsp::kGmHead * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (rr)
            RSP_CHECK_HIP(hipMemcpyAsync(hp + rsp::kGmHead, s->d_blk + rsp::kGmSmall + (size_t)rsp::kGmPartRR * rsp::kKryMaxGrid,
                                         (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (bb)
            RSP_CHECK_HIP(hipMemcpyAsync(hp + rsp::kGmHead + rsp::kKryMaxGrid,
                                         s->d_blk + rsp::kGmSmall + (size_t)rsp::kGmPartBB * rsp::kKryMaxGrid,
                                         (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipEventRecord(s->ev, h->stream));
        RSP_CHECK_HIP(hipEventSynchronize(s->ev));
        return RSP_STATUS_SUCCESS;
    };
    // w = b - A x0, (b,b), (r,r)
    RSP_TRY(krylov_spmv(h, *s, d_x, s->w));
    RSP_TRY(kern(rsp::kGmResid, 0, 1));
    RSP_TRY(read_back(true, true));
    const double bb = rsp::kry_combine_host(hp + rsp::kGmHead + rsp::kKryMaxGrid, G);
    double rr = rsp::kry_combine_host(hp + rsp::kGmHead, G);
    const double bnorm = sqrt(bb);
    if (bb == 0.0) {  // x = 0 solves it
        rsp::KryArgs k{};
        k.n = s->n;
        k.x = d_x;
        const hipError_t e = ftz ? rsp_k_ftz::krylov(rsp::kKryZero, type, k, h->stream)
                                 : rsp_k::krylov(rsp::kKryZero, type, k, h->stream);
        if (e != hipSuccess) return RSP_STATUS_EXECUTION_FAILED;
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        *reason = RSP_SOLVE_CONVERGED;
        return RSP_STATUS_SUCCESS;
    }
    if (!std::isfinite(bb) || !std::isfinite(rr)) {  // b or x0 not finite: nothing to iterate on
        *relres = sqrt(rr) / bnorm;
        *reason = RSP_SOLVE_BREAKDOWN;
        return RSP_STATUS_SUCCESS;
    }
    double rel = sqrt(rr) / bnorm;
    int total = 0;
    bool first = true;
    if (rel <= rtol) {
        *reason = RSP_SOLVE_CONVERGED;
    } else {
        while (total < max_iters) {
            // one cycle, from the residual in w
            RSP_TRY(kern(rsp::kGmNormalise, -1, first ? 1 : 0));
            first = false;
            int cols = 0;           // columns launched
            bool by_est = false;
            while (cols < s->m && total + cols < max_iters) {
                const int j = cols;
                // z_j = M^-1 v_j (mixed: from v_j's fp32 copy, written by the kernel that made v_j)
                if (s->precond()) RSP_TRY(krylov_apply(h, *s, s->V + (size_t)j * tb, s->Z + (size_t)j * tb, ftz));
                RSP_TRY(krylov_spmv(h, *s, s->Z + (size_t)j * tb, s->w));
                RSP_TRY(kern(rsp::kGmMultiDot, j, 0));
                RSP_TRY(kern(rsp::kGmUpdate1, j, 0));
                RSP_TRY(kern(rsp::kGmUpdate2, j, 0));
                RSP_TRY(kern(rsp::kGmNormalise, j, 0));
                cols++;
                if (cols == s->m || total + cols == max_iters) break;  // the cycle's end is the check
                if ((total + cols) % check_every != 0) continue;
                RSP_TRY(read_back(false, false));
                if (hp[rsp::kGmFlag] != 0.0 || hp[rsp::kGmStop] != 0.0) break;
                rel = hp[rsp::kGmEst + j];
                s->history.push_back(rel);
                if (rel <= rtol) {
                    by_est = true;
                    break;
                }
            }
            // x += Z y over the columns the device completed
            RSP_TRY(kern(rsp::kGmCombine, cols - 1, 0));
            if (by_est) {
                RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
                total += cols;
                *reason = RSP_SOLVE_CONVERGED;
                break;
            }
            RSP_TRY(krylov_spmv(h, *s, d_x, s->w));
            RSP_TRY(kern(rsp::kGmResid, 0, 0));
            RSP_TRY(read_back(true, false));
            rr = rsp::kry_combine_host(hp + rsp::kGmHead, G);
            rel = sqrt(rr) / bnorm;
            const int flag = (int)hp[rsp::kGmFlag];
            total += (int)hp[rsp::kGmDone];
            s->history.push_back(rel);
            if (rel <= rtol) {
                *reason = RSP_SOLVE_CONVERGED;
                break;
            }
            if (flag || !std::isfinite(rel)) {
                *reason = RSP_SOLVE_BREAKDOWN;
                break;
            }
        }
    }
    *iters = total;
    *relres = rel;
    return krylov_solve_end(h, *s, total);
}

static rsp_status_t orthogonalize(rsp_handle_t h, rsp_datatype_t value_type, int64_t n, int k, const void *d_V,
                                  int64_t ldv, void *d_w, double *hh) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (!hh || n < 0 || k < 1 || k > RSP_GMRES_MAX_RESTART || ldv < n) return RSP_STATUS_INVALID_VALUE;
    if (n > 0 && (!d_V || !d_w)) return RSP_STATUS_INVALID_VALUE;
    for (int i = 0; i <= k; i++) hh[i] = 0.0;
    if (n == 0) return RSP_STATUS_SUCCESS;
    const size_t mirror = 2 * (size_t)rsp::kGmLd + rsp::kKryMaxGrid;
    if (!h->d_gm) {
        RSP_CHECK_HIP(hipMalloc((void **)&h->d_gm, rsp::kGmBlockDoubles * sizeof(double)));
        // (flag and stop words clear: the three kernels read them and never set them)
        RSP_CHECK_HIP(hipMemsetAsync(h->d_gm, 0, rsp::kGmSmall * sizeof(double), h->stream));
    }
    if (!h->h_gm) RSP_CHECK_HIP(hipHostMalloc((void **)&h->h_gm, mirror * sizeof(double), hipHostMallocDefault));
    rsp::GmArgs a{};
    a.n = n;
    a.blk = h->d_gm;
    a.j = k - 1;
    a.V = const_cast<void *>(d_V);
    a.ldv = ldv;
    a.w = d_w;
    const int type = value_type == RSP_R_64F ? rsp::kKryF64 : rsp::kKryF32;
    const bool ftz = h->ftz && type == rsp::kKryF32;
    for (rsp::GmOp op : {rsp::kGmMultiDot, rsp::kGmUpdate1, rsp::kGmUpdate2}) {
        const hipError_t e = ftz ? rsp_k_ftz::gmres(op, type, a, h->stream) : rsp_k::gmres(op, type, a, h->stream);
        if (e != hipSuccess) return RSP_STATUS_EXECUTION_FAILED;
    }
    const int G = rsp::kry_grid(n).grid;
    static_assert(rsp::kGmH2 == rsp::kGmH1 + rsp::kGmLd, "h and h' are read back as one range");
    RSP_CHECK_HIP(hipMemcpyAsync(h->h_gm, h->d_gm + rsp::kGmH1, 2 * (size_t)rsp::kGmLd * sizeof(double),
                                 hipMemcpyDeviceToHost, h->stream));
    RSP_CHECK_HIP(hipMemcpyAsync(h->h_gm + 2 * rsp::kGmLd,
                                 h->d_gm + rsp::kGmSmall + (size_t)rsp::kGmPartNrm * rsp::kKryMaxGrid,
                                 (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    for (int i = 0; i < k; i++) hh[i] = h->h_gm[i] + h->h_gm[rsp::kGmLd + i];
    hh[k] = sqrt(rsp::kry_combine_host(h->h_gm + 2 * rsp::kGmLd, G));
    return RSP_STATUS_SUCCESS;
}

/* ------------------------------------------------- iterative refinement */

static rsp_status_t ref_kernel(rsp_handle_t h, rsp::RefOp op, const rsp::RefArgs &a) {
    const hipError_t e = h->ftz ? rsp_k_ftz::refine(op, a, h->stream) : rsp_k::refine(op, a, h->stream);
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

static bool is_type(rsp_datatype_t t) { return t == RSP_R_64F || t == RSP_R_32F; }

static rsp_status_t convert_scaled(rsp_handle_t h, int64_t n, rsp_datatype_t src_type, const void *d_src, int exp2,
                                   rsp_datatype_t dst_type, void *d_dst) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (n < 0 || !is_type(src_type) || !is_type(dst_type) || exp2 < -1022 || exp2 > 1022)
        return RSP_STATUS_INVALID_VALUE;
    if (n > 0 && (!d_src || !d_dst)) return RSP_STATUS_INVALID_VALUE;
    if (d_src == d_dst && src_type != dst_type && n > 0) return RSP_STATUS_INVALID_VALUE;
    rsp::RefArgs a{};
    a.n = n;
    a.scale = ldexp(1.0, exp2);
    a.src_f32 = src_type == RSP_R_32F;
    a.dst_f32 = dst_type == RSP_R_32F;
    a.src = d_src;
    a.dst = d_dst;
    return ref_kernel(h, rsp::kRefConvert, a);
}

static rsp_status_t refine_update(rsp_handle_t h, int64_t n, const float *d_d, int exp2, double *d_x,
                                  double *d_x_old) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (n < 0 || exp2 < -1022 || exp2 > 1022) return RSP_STATUS_INVALID_VALUE;
    if (n > 0 && (!d_d || !d_x || d_x_old == d_x)) return RSP_STATUS_INVALID_VALUE;
    rsp::RefArgs a{};
    a.n = n;
    a.scale = ldexp(1.0, exp2);
    a.src = d_d;
    a.dst = d_x;
    a.x_old = d_x_old;
    return ref_kernel(h, rsp::kRefUpdate, a);
}

// One refinement: the fp64 side (r, v = A x, x_old), the fp32 right-hand side
// and correction of the inner solve, the inner solver itself (one of the three,
// made by its public create call over A_low) and the Krylov block and mirror
// the residual's norm is read back through (KrylovCommon with T = fp64, M = I).
struct rsp_refine : KrylovCommon {
    rsp_refine_method_t method = RSP_REFINE_GMRES;
    rsp_bicgstab_t bicgstab = nullptr;
    rsp_cg_t cg = nullptr;
    rsp_gmres_t gmres = nullptr;
    double *r = nullptr, *v = nullptr, *x_old = nullptr;
    float *r32 = nullptr, *d = nullptr;
    std::vector<int> inner_history;  // per history entry: the inner iterations that produced that x
    ~rsp_refine() {
        if (bicgstab) (void)rsp_bicgstab_destroy(bicgstab);
        if (cg) (void)rsp_cg_destroy(cg);
        if (gmres) (void)rsp_gmres_destroy(gmres);
    }
};

static rsp_status_t refine_create(rsp_handle_t h, rsp_spmat_t A, rsp_spmat_t A_low, rsp_ilu0_info_t info,
                                  const void *d_factor_low, rsp_cheby_t cheby, rsp_refine_method_t method,
                                  int restart, rsp_refine_t *out) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!out) return RSP_STATUS_INVALID_VALUE;
    *out = nullptr;
    if (!A || !A_low || (info && !d_factor_low)) return RSP_STATUS_INVALID_VALUE;
    if (A->type != RSP_R_64F || A_low->type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (cheby && cheby->P != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (A->rows != A->cols || A->rows < 1 || A_low->rows != A->rows || A_low->cols != A->cols)
        return RSP_STATUS_INVALID_VALUE;
    if (method != RSP_REFINE_BICGSTAB && method != RSP_REFINE_CG && method != RSP_REFINE_GMRES)
        return RSP_STATUS_INVALID_VALUE;
    if (method == RSP_REFINE_GMRES && (restart < 1 || restart > RSP_GMRES_MAX_RESTART))
        return RSP_STATUS_INVALID_VALUE;
    if (!A->planned || A->plan_type != A->type) RSP_TRY(spmv_plan(h, A, A->type));
    std::unique_ptr<rsp_refine> s(new rsp_refine);  // (a half-built one is freed on every way out, its inner solver too)
    krylov_bind(*s, h, A, nullptr, RSP_R_64F, nullptr, nullptr);
    s->method = method;
    switch (method) {
        case RSP_REFINE_BICGSTAB:
            RSP_TRY(cheby ? rsp_bicgstab_create_cheby(h, A_low, cheby, &s->bicgstab)
                          : rsp_bicgstab_create(h, A_low, info, RSP_R_32F, d_factor_low, &s->bicgstab));
            break;
        case RSP_REFINE_CG:
            RSP_TRY(cheby ? rsp_cg_create_cheby(h, A_low, cheby, &s->cg)
                          : rsp_cg_create(h, A_low, info, RSP_R_32F, d_factor_low, &s->cg));
            break;
        default:
            RSP_TRY(cheby ? rsp_gmres_create_cheby(h, A_low, cheby, restart, &s->gmres)
                          : rsp_gmres_create(h, A_low, info, RSP_R_32F, d_factor_low, restart, &s->gmres));
            break;
    }
    // r, v, x_old (fp64), then r32, d (fp32)
    const size_t tb = s->tbytes(), lb = align256((size_t)s->n * sizeof(float));
    char *at = nullptr;
    RSP_TRY(krylov_alloc(*s, align256(rsp::kKryBlockDoubles * sizeof(double)), 3 * tb + 2 * lb,
                         rsp::kKryScalars + 2 * (size_t)rsp::kKryMaxGrid, &at));
    s->r = (double *)at;
    s->v = (double *)(at + tb);
    s->x_old = (double *)(at + 2 * tb);
    s->r32 = (float *)(at + 3 * tb);
    s->d = (float *)(at + 3 * tb + lb);
    *out = s.release();
    return RSP_STATUS_SUCCESS;
}

static rsp_status_t refine_inner(rsp_handle_t h, rsp_refine_t s, double rtol, int max_iters, int check_every,
                                 int *iters, rsp_solve_reason_t *reason) {
    double rel = 0.0;
    switch (s->method) {
        case RSP_REFINE_BICGSTAB:
            return rsp_bicgstab_solve(h, s->bicgstab, s->r32, s->d, rtol, max_iters, check_every, iters, &rel, reason);
        case RSP_REFINE_CG:
            return rsp_cg_solve(h, s->cg, s->r32, s->d, rtol, max_iters, check_every, iters, &rel, reason);
        default:
            return rsp_gmres_solve(h, s->gmres, s->r32, s->d, rtol, max_iters, check_every, iters, &rel, reason);
    }
}

static rsp_status_t refine_solve(rsp_handle_t h, rsp_refine_t s, const void *d_b, void *d_x, double rtol,
                                 int max_steps, double inner_rtol, int inner_max_iters, int check_every, int *steps,
                                 int *inner_iters, double *relres, rsp_solve_reason_t *reason) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!inner_iters) return RSP_STATUS_INVALID_VALUE;
    if (inner_max_iters < 0 || !(inner_rtol >= 0.0)) return RSP_STATUS_INVALID_VALUE;
    RSP_TRY(krylov_solve_begin(h, s, d_b, d_x, rtol, max_steps, check_every, steps, relres, reason));
    *inner_iters = 0;
    s->inner_history.clear();
    const int G = rsp::kry_grid(s->n).grid;
    const size_t xbytes = (size_t)s->n * sizeof(double);
    rsp::KryArgs a{};
    a.n = s->n;
    a.blk = s->d_blk;
    a.b = d_b;
    a.v = s->v;
    a.r = s->r;
    double *hp = s->h_pin;
    // the one host wait of a step: the (r,r) partials (step 0: and (b,b)), as cg_solve's
    auto residual = [&](bool bb, double *rr) -> rsp_status_t {
        RSP_TRY(krylov_spmv(h, *s, d_x, s->v));
        if (rsp_k::krylov(rsp::kKryCgInit, rsp::kKryF64, a, h->stream) != hipSuccess)  // r = b - v; (b,b), (r,r)
            return RSP_STATUS_EXECUTION_FAILED;
        if (bb)
            RSP_CHECK_HIP(hipMemcpyAsync(hp + rsp::kKryScalars + rsp::kKryMaxGrid,
                                         s->d_blk + rsp::kKryScalars + (size_t)rsp::kKryPartBB * rsp::kKryMaxGrid,
                                         (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipMemcpyAsync(hp, s->d_blk, (rsp::kKryScalars + (size_t)G) * sizeof(double),
                                     hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipEventRecord(s->ev, h->stream));
        RSP_CHECK_HIP(hipEventSynchronize(s->ev));
        *rr = rsp::kry_combine_host(hp + rsp::kKryScalars, G);
        return RSP_STATUS_SUCCESS;
    };
    auto restore = [&]() -> rsp_status_t {  // the rejected step's x gives way to the one before it
        RSP_CHECK_HIP(hipMemcpyAsync(d_x, s->x_old, xbytes, hipMemcpyDeviceToDevice, h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        return RSP_STATUS_SUCCESS;
    };
    double bnorm = 0.0, rn_prev = 0.0;
    int inner_last = 0;
    for (int k = 0;; k++) {
        double rr = 0.0;
        RSP_TRY(residual(k == 0, &rr));
        if (k == 0) {
            const double bb = rsp::kry_combine_host(hp + rsp::kKryScalars + rsp::kKryMaxGrid, G);
            bnorm = sqrt(bb);
            if (bb == 0.0) {  // x = 0 solves it
                rsp::KryArgs z{};
                z.n = s->n;
                z.x = d_x;
                if (rsp_k::krylov(rsp::kKryZero, rsp::kKryF64, z, h->stream) != hipSuccess)
                    return RSP_STATUS_EXECUTION_FAILED;
                RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
                *reason = RSP_SOLVE_CONVERGED;
                return RSP_STATUS_SUCCESS;
            }
        }
        const double rn = sqrt(rr), rel = rn / bnorm;
        s->history.push_back(rel);
        s->inner_history.push_back(inner_last);
        if (!std::isfinite(rn) || !std::isfinite(bnorm)) {  // k = 0: b or x0 not finite; later: the correction was not
            *reason = RSP_SOLVE_BREAKDOWN;
            if (k > 0) RSP_TRY(restore());
            *steps = k > 0 ? k - 1 : 0;
            *relres = k > 0 ? s->history[k - 1] : rel;
            return RSP_STATUS_SUCCESS;
        }
        if (rel <= rtol) {
            *reason = RSP_SOLVE_CONVERGED;
            *steps = k;
            *relres = rel;
            return RSP_STATUS_SUCCESS;
        }
        if (k > 0 && rn >= rn_prev) {  // the step gained nothing: the floor of this A, A_low and inner solve
            RSP_TRY(restore());
            *reason = RSP_SOLVE_STAGNATED;
            *steps = k - 1;
            *relres = s->history[k - 1];
            return RSP_STATUS_SUCCESS;
        }
        *steps = k;
        *relres = rel;
        if (k == max_steps) return RSP_STATUS_SUCCESS;  // (*reason is MAX_ITERS)
        rn_prev = rn;
        // r32 = fp32(r * 2^-e) with ||r|| = m * 2^e, 0.5 <= m < 1; d = 0
        int e = 0;
        (void)frexp(rn, &e);
        e = std::min(std::max(e, -1022), 1022);
        rsp::RefArgs c{};
        c.n = s->n;
        c.scale = ldexp(1.0, -e);
        c.src = s->r;
        c.dst = s->r32;
        c.zero = s->d;
        RSP_TRY(ref_kernel(h, rsp::kRefNarrowZero, c));
        rsp_solve_reason_t ir = RSP_SOLVE_MAX_ITERS;
        RSP_TRY(refine_inner(h, s, inner_rtol, inner_max_iters, check_every, &inner_last, &ir));
        *inner_iters += inner_last;
        if (ir == RSP_SOLVE_BREAKDOWN && inner_last == 0) {  // nothing to add
            *reason = RSP_SOLVE_BREAKDOWN;
            RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
            return RSP_STATUS_SUCCESS;
        }
        RSP_TRY(refine_update(h, s->n, s->d, e, (double *)d_x, s->x_old));
    }
}

static rsp_status_t refine_history(const rsp_refine *s, int cap, double *relres, int *inner_iters, int *count) {
    if (!s || !count || cap < 0 || (cap > 0 && (!relres || !inner_iters))) return RSP_STATUS_INVALID_VALUE;
    *count = (int)s->history.size();
    for (int k = 0; k < cap && k < *count; k++) {
        relres[k] = s->history[k];
        inner_iters[k] = s->inner_history[k];
    }
    return RSP_STATUS_SUCCESS;
}

extern "C" {

rsp_status_t rsp_refine_create(rsp_handle_t h, rsp_spmat_t A, rsp_spmat_t A_low, rsp_ilu0_info_t info,
                               const void *d_factor_low, rsp_refine_method_t method, int restart, rsp_refine_t *s) {
    return guarded([&] { return refine_create(h, A, A_low, info, d_factor_low, nullptr, method, restart, s); });
}

rsp_status_t rsp_refine_create_cheby(rsp_handle_t h, rsp_spmat_t A, rsp_spmat_t A_low, rsp_cheby_t c,
                                     rsp_refine_method_t method, int restart, rsp_refine_t *s) {
    return guarded([&] {
        if (h && s && !c) {
            *s = nullptr;
            return RSP_STATUS_INVALID_VALUE;
        }
        return refine_create(h, A, A_low, nullptr, nullptr, c, method, restart, s);
    });
}

rsp_status_t rsp_refine_solve(rsp_handle_t h, rsp_refine_t s, const void *d_b, void *d_x, double rtol, int max_steps,
                              double inner_rtol, int inner_max_iters, int check_every, int *steps, int *inner_iters,
                              double *relres, rsp_solve_reason_t *reason) {
    return guarded([&] {
        return refine_solve(h, s, d_b, d_x, rtol, max_steps, inner_rtol, inner_max_iters, check_every, steps,
                            inner_iters, relres, reason);
    });
}

rsp_status_t rsp_refine_history(rsp_refine_t s, int cap, double *relres, int *inner_iters, int *count) {
    return refine_history(s, cap, relres, inner_iters, count);
}

rsp_status_t rsp_refine_destroy(rsp_refine_t s) {
    if (!s) return RSP_STATUS_INVALID_VALUE;
    delete s;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_convert_scaled(rsp_handle_t h, int64_t n, rsp_datatype_t src_type, const void *d_src, int exp2,
                                rsp_datatype_t dst_type, void *d_dst) {
    return guarded([&] { return convert_scaled(h, n, src_type, d_src, exp2, dst_type, d_dst); });
}

rsp_status_t rsp_refine_update(rsp_handle_t h, int64_t n, const float *d_d, int exp2, double *d_x, double *d_x_old) {
    return guarded([&] { return refine_update(h, n, d_d, exp2, d_x, d_x_old); });
}

rsp_status_t rsp_bicgstab_create(rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info,
                                 rsp_datatype_t precond_type, const void *d_factor, rsp_bicgstab_t *s) {
    return guarded([&] { return bicgstab_create(h, A, info, precond_type, d_factor, nullptr, s); });
}

rsp_status_t rsp_bicgstab_create_cheby(rsp_handle_t h, rsp_spmat_t A, rsp_cheby_t c, rsp_bicgstab_t *s) {
    return guarded([&] {
        if (h && s && !c) {
            *s = nullptr;
            return RSP_STATUS_INVALID_VALUE;
        }
        return bicgstab_create(h, A, nullptr, RSP_R_64F, nullptr, c, s);
    });
}

rsp_status_t rsp_bicgstab_solve(rsp_handle_t h, rsp_bicgstab_t s, const void *d_b, void *d_x, double rtol,
                                int max_iters, int check_every, int *iters, double *relres,
                                rsp_solve_reason_t *reason) {
    return guarded([&] { return bicgstab_solve(h, s, d_b, d_x, rtol, max_iters, check_every, iters, relres, reason); });
}

rsp_status_t rsp_bicgstab_history(rsp_bicgstab_t s, int cap, double *relres, int *count) {
    return krylov_history(s, cap, relres, count);
}

rsp_status_t rsp_bicgstab_destroy(rsp_bicgstab_t s) {
    if (!s) return RSP_STATUS_INVALID_VALUE;
    delete s;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_dot(rsp_handle_t h, rsp_datatype_t value_type, int64_t n, const void *d_x, const void *d_y,
                     double *result) {
    return guarded([&] { return krylov_dot(h, value_type, n, d_x, d_y, result); });
}

rsp_status_t rsp_cg_create(rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info, rsp_datatype_t precond_type,
                           const void *d_factor, rsp_cg_t *s) {
    return guarded([&] { return cg_create(h, A, info, precond_type, d_factor, nullptr, s); });
}

rsp_status_t rsp_cg_create_cheby(rsp_handle_t h, rsp_spmat_t A, rsp_cheby_t c, rsp_cg_t *s) {
    return guarded([&] {
        if (h && s && !c) {
            *s = nullptr;
            return RSP_STATUS_INVALID_VALUE;
        }
        return cg_create(h, A, nullptr, RSP_R_64F, nullptr, c, s);
    });
}

rsp_status_t rsp_cg_solve(rsp_handle_t h, rsp_cg_t s, const void *d_b, void *d_x, double rtol, int max_iters,
                          int check_every, int *iters, double *relres, rsp_solve_reason_t *reason) {
    return guarded([&] { return cg_solve(h, s, d_b, d_x, rtol, max_iters, check_every, iters, relres, reason); });
}

rsp_status_t rsp_cg_history(rsp_cg_t s, int cap, double *relres, int *count) {
    return krylov_history(s, cap, relres, count);
}

rsp_status_t rsp_cg_destroy(rsp_cg_t s) {
    if (!s) return RSP_STATUS_INVALID_VALUE;
    delete s;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_gmres_create(rsp_handle_t h, rsp_spmat_t A, rsp_ilu0_info_t info, rsp_datatype_t precond_type,
                              const void *d_factor, int restart, rsp_gmres_t *s) {
    return guarded([&] { return gmres_create(h, A, info, precond_type, d_factor, nullptr, restart, s); });
}

rsp_status_t rsp_gmres_create_cheby(rsp_handle_t h, rsp_spmat_t A, rsp_cheby_t c, int restart, rsp_gmres_t *s) {
    return guarded([&] {
        if (h && s && !c) {
            *s = nullptr;
            return RSP_STATUS_INVALID_VALUE;
        }
        return gmres_create(h, A, nullptr, RSP_R_64F, nullptr, c, restart, s);
    });
}

rsp_status_t rsp_gmres_solve(rsp_handle_t h, rsp_gmres_t s, const void *d_b, void *d_x, double rtol, int max_iters,
                             int check_every, int *iters, double *relres, rsp_solve_reason_t *reason) {
    return guarded([&] { return gmres_solve(h, s, d_b, d_x, rtol, max_iters, check_every, iters, relres, reason); });
}

rsp_status_t rsp_gmres_history(rsp_gmres_t s, int cap, double *relres, int *count) {
    return krylov_history(s, cap, relres, count);
}

rsp_status_t rsp_gmres_destroy(rsp_gmres_t s) {
    if (!s) return RSP_STATUS_INVALID_VALUE;
    delete s;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_orthogonalize(rsp_handle_t h, rsp_datatype_t value_type, int64_t n, int k, const void *d_V,
                               int64_t ldv, void *d_w, double *hh) {
    return guarded([&] { return orthogonalize(h, value_type, n, k, d_V, ldv, d_w, hh); });
}

rsp_status_t rsp_gmres_lsq_host(int k, int ldh, const double *H, double beta, double *y, double *est) {
    return guarded([&] {
        if (k < 1 || k > RSP_GMRES_MAX_RESTART || ldh < k + 1 || !H || !y || !est) return RSP_STATUS_INVALID_VALUE;
        std::vector<double> R((size_t)rsp::kGmLd * k), cs(k), sn(k), g(k + 1, 0.0);
        g[0] = beta;
        for (int j = 0; j < k; j++) {
            double *col = R.data() + (size_t)j * rsp::kGmLd;
            for (int i = 0; i <= j + 1; i++) col[i] = H[i + (size_t)j * ldh];
            if (rsp::gmres_lsq(col, j, cs.data(), sn.data(), g.data(), nullptr, 0, 0, nullptr))
                return RSP_STATUS_INVALID_VALUE;
            est[j] = fabs(g[j + 1]);
        }
        rsp::gmres_lsq(nullptr, 0, nullptr, nullptr, g.data(), R.data(), rsp::kGmLd, k, y);
        return RSP_STATUS_SUCCESS;
    });
}

}  // the C ABI
