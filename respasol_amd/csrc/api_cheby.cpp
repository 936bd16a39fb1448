// api_cheby.cpp — the Chebyshev polynomial preconditioner of include/rsp.h
// (rsp_cheby_*): the coefficients on the host, the one set-up launch, and the
// apply as the kernels of cheby.hip around spmv_run (rsp_api.cpp). The Krylov
// solvers reach it through rsp_api::cheby_apply (api_krylov.cpp krylov_apply).

#include "rsp_internal.h"

using namespace rsp_api;

static bool good_bounds(double lmin, double lmax) {
    return std::isfinite(lmin) && std::isfinite(lmax) && lmin > 0.0 && lmin < lmax;
}

// c0, a[0 .. degree-2], b[0 .. degree-2] in fp64, in the order include/rsp.h
// states (the unit is built with -ffp-contract=off: no fused multiply-add).
static void coefficients(int degree, double lmin, double lmax, double *c0, double *a, double *b) {
    const double theta = (lmax + lmin) / 2.0, delta = (lmax - lmin) / 2.0, sigma = theta / delta;
    double rho = 1.0 / sigma;
    *c0 = 1.0 / theta;
    for (int j = 1; j < degree; j++) {
        const double rho_j = 1.0 / (2.0 * sigma - rho);
        a[j - 1] = rho_j * rho;
        b[j - 1] = 2.0 * rho_j / delta;
        rho = rho_j;
    }
}

static double round_to(rsp_datatype_t P, double v) { return P == RSP_R_32F ? (double)(float)v : v; }

static void set_bounds(rsp_cheby *c, double lmin, double lmax) {
    c->lmin = lmin;
    c->lmax = lmax;
    coefficients(c->degree, lmin, lmax, &c->c0, c->a, c->b);
    c->c0 = round_to(c->P, c->c0);
    for (int j = 0; j + 1 < c->degree; j++) {
        c->a[j] = round_to(c->P, c->a[j]);
        c->b[j] = round_to(c->P, c->b[j]);
    }
}

static rsp_status_t cheby_create(rsp_handle_t h, rsp_spmat_t A, int degree, rsp_cheby_scaling_t scaling,
                                 double ratio, int *position, rsp_cheby_t *out) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!out) return RSP_STATUS_INVALID_VALUE;
    *out = nullptr;
    if (position) *position = -1;
    if (!A || A->rows != A->cols || A->rows < 1 || A->rows > INT_MAX) return RSP_STATUS_INVALID_VALUE;
    if (degree < 1 || degree > RSP_CHEBY_MAX_DEGREE) return RSP_STATUS_INVALID_VALUE;
    if (scaling != RSP_CHEBY_SCALE_NONE && scaling != RSP_CHEBY_SCALE_JACOBI) return RSP_STATUS_INVALID_VALUE;
    if (!std::isfinite(ratio) || !(ratio > 1.0)) return RSP_STATUS_INVALID_VALUE;
    if (!A->planned || A->plan_type != A->type) RSP_TRY(spmv_plan(h, A, A->type));
    std::unique_ptr<rsp_cheby> c(new rsp_cheby);  // (a half-built one is freed on every way out)
    c->device = h->device;
    c->A = A;
    c->P = A->type;
    c->n = A->rows;
    c->degree = degree;
    // [set-up state | dinv (JACOBI) | d | w]
    const bool jacobi = scaling == RSP_CHEBY_SCALE_JACOBI;
    const size_t vb = align256((size_t)c->n * elem_size(c->P)), head = 256;
    RSP_CHECK_HIP(hipMalloc(&c->d_mem, head + (jacobi ? 3 : 2) * vb));
    char *at = (char *)c->d_mem + head;
    if (jacobi) {
        c->dinv = at;
        at += vb;
    }
    c->d = at;
    c->w = at + vb;
    unsigned long long state[2] = {0ull, ~0ull};
    RSP_CHECK_HIP(hipMemcpyAsync(c->d_mem, state, sizeof(state), hipMemcpyHostToDevice, h->stream));
    rsp::ChebySetupArgs a{};
    a.n = (int)c->n;
    a.rowptr = A->rowptr;
    a.colidx = A->colidx;
    a.vals = A->vals;
    a.dinv = c->dinv;
    a.state = (unsigned long long *)c->d_mem;
    const int f32 = c->P == RSP_R_32F;
    const hipError_t e = (h->ftz && f32) ? rsp_k_ftz::cheby_setup(f32, a, h->stream)
                                         : rsp_k::cheby_setup(f32, a, h->stream);
    if (e != hipSuccess) return RSP_STATUS_EXECUTION_FAILED;
    RSP_CHECK_HIP(hipMemcpyAsync(state, c->d_mem, sizeof(state), hipMemcpyDeviceToHost, h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    if (state[1] != ~0ull) {
        if (position) *position = (int)state[1];
        return RSP_STATUS_ZERO_PIVOT;
    }
    double lmax = 0.0;
    memcpy(&lmax, &state[0], sizeof(lmax));
    if (!good_bounds(lmax / ratio, lmax)) return RSP_STATUS_INVALID_VALUE;  // a bound not finite or <= 0
    set_bounds(c.get(), lmax / ratio, lmax);
    *out = c.release();
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_api::cheby_apply(rsp_handle_t h, rsp_cheby *c, const void *d_r, void *d_z) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!c || !d_r || !d_z || d_r == d_z) return RSP_STATUS_INVALID_VALUE;
    const int f32 = c->P == RSP_R_32F;
    const bool ftz = h->ftz && f32;
    auto kern = [&](rsp::ChebyOp op, const rsp::ChebyArgs &a) {
        const hipError_t e = ftz ? rsp_k_ftz::cheby(op, f32, a, h->stream) : rsp_k::cheby(op, f32, a, h->stream);
        return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
    };
    rsp::ChebyArgs a{};
    a.n = c->n;
    a.dinv = c->dinv;
    a.r = d_r;
    a.z = d_z;
    a.d = c->d;
    a.w = c->w;
    a.c0 = c->c0;
    a.only_z = c->degree == 1;
    RSP_TRY(kern(rsp::kChebyFirst, a));
    const double m1 = -1.0, p1 = 1.0;
    const float m1f = -1.0f, p1f = 1.0f;
    for (int j = 1; j < c->degree; j++) {
        // w = w - A d: the SpMV's own alpha / beta epilogue
        RSP_TRY(spmv_run(h, RSP_OPERATION_NON_TRANSPOSE, f32 ? (const void *)&m1f : (const void *)&m1, c->A, c->d,
                         f32 ? (const void *)&p1f : (const void *)&p1, c->w, c->P, nullptr, 0));
        a.a = c->a[j - 1];
        a.b = c->b[j - 1];
        a.only_z = j == c->degree - 1;
        RSP_TRY(kern(rsp::kChebyStep, a));
    }
    return RSP_STATUS_SUCCESS;
}

extern "C" {

rsp_status_t rsp_cheby_create(rsp_handle_t h, rsp_spmat_t A, int degree, rsp_cheby_scaling_t scaling, double ratio,
                              int *position, rsp_cheby_t *c) {
    return guarded([&] { return cheby_create(h, A, degree, scaling, ratio, position, c); });
}

rsp_status_t rsp_cheby_get_bounds(rsp_cheby_t c, double *lmin, double *lmax) {
    if (!c || !lmin || !lmax) return RSP_STATUS_INVALID_VALUE;
    *lmin = c->lmin;
    *lmax = c->lmax;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_cheby_set_bounds(rsp_cheby_t c, double lmin, double lmax) {
    if (!c || !good_bounds(lmin, lmax)) return RSP_STATUS_INVALID_VALUE;
    set_bounds(c, lmin, lmax);
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_cheby_apply(rsp_handle_t h, rsp_cheby_t c, const void *d_r, void *d_z) {
    return guarded([&] { return cheby_apply(h, c, d_r, d_z); });
}

rsp_status_t rsp_cheby_destroy(rsp_cheby_t c) {
    if (!c) return RSP_STATUS_INVALID_VALUE;
    delete c;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_cheby_coefficients_host(int degree, double lmin, double lmax, double *c0, double *a, double *b) {
    if (degree < 1 || degree > RSP_CHEBY_MAX_DEGREE || !good_bounds(lmin, lmax) || !c0) return RSP_STATUS_INVALID_VALUE;
    if (degree > 1 && (!a || !b)) return RSP_STATUS_INVALID_VALUE;
    coefficients(degree, lmin, lmax, c0, a, b);
    return RSP_STATUS_SUCCESS;
}

}  // the C ABI
