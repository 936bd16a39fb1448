/*
 * test_solve.c — ILU(0)- or Chebyshev-preconditioned BiCGStab / GMRES(m) / CG driver, with
 * --refine the same inside mixed-precision iterative refinement (built as
 * `test_solve`).
 * No GPU counterpart in the reference; shaped like its direct-solver drivers
 * (Pardiso/test_pardiso.c): b = 1 (:107), solve, relative residual ||b - A x||
 * / ||b|| recomputed on the host (:258-274).
 *
 *   test_solve <A.mtx | surrogate:NAME[@scale]> [--prec=fp64|fp32]
 *              [--precond=fp64|fp32|none] [--ftz] [--rtol=R] [--maxit=N]
 *              [--full-symmetric] [--dump=FILE] [--method=bicgstab|gmres|cg]
 *              [--restart=M] [--refine[=inner_rtol]] [--cheby=K] [--cheby-ratio=R]
 *
 * Flow: load as test_ilu0 does (outputbase 0); iteration values in --prec;
 * b = 1, x0 = 0; [timed "Symbolic"] ILU analysis; [timed "Numeric"]
 * factorisation of a copy of the values in the --precond type (default: the
 * --prec type; must not be wider); [timed "Solve"] rsp_bicgstab_solve, or with --method=gmres
 * rsp_gmres_solve of restart length --restart (default 30), or with
 * --method=cg rsp_cg_solve (A must be symmetric positive definite; a file
 * whose banner says symmetric is then loaded with both triangles, as under
 * --full-symmetric, and a general file is taken as it is); the six-line
 * report. Symbolic is wall-clock, Numeric and Solve are event pairs
 * on the stream. The residual line is the TRUE residual, in fp64 on the host
 * (rsp_host_spmv_f64 on the file's fp64 values), not the recurrence's.
 * Exit 0 for any reason code (converged, max iterations, breakdown);
 * non-zero only on a status error. --dump writes x (binary, --prec type).
 * --refine (needs --prec=fp64 and --precond=fp32 or none, else exit 2): the
 * values are narrowed to fp32 on the device (rsp_convert_scaled), the factor is
 * fp32 and the solve is rsp_refine_solve — fp64 residuals and updates around
 * all-fp32 solves by --method to inner_rtol (default 1e-4), each of at most
 * --maxit iterations, at most 50 steps; "Iterations" is then the inner
 * iterations of all steps, and two more lines follow the report.
 * --cheby=K (1..64; with --precond=none: exit 2): the preconditioner is the
 * degree-K Chebyshev polynomial (rsp_cheby_create, Jacobi scaling, lmin = lmax
 * / R, --cheby-ratio=R, default 30) in the --precond type instead of ILU(0) —
 * on A itself, or on an fp32 descriptor of the same pattern when --precond is
 * narrower than --prec; with --refine it is fp32. "Symbolic" is then the
 * polynomial's set-up (wall-clock) and "Numeric" is 0.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "drv_common.h"
#include "rsp.h"
#include "rsp_host.h"

#define HIP_OR_FAIL(stat)                                                                       \
    do {                                                                                        \
        hipError_t s_ = (stat);                                                                 \
        if (s_ != hipSuccess) {                                                                 \
            fprintf(stderr, "HIP Error: %s %s %d\n", hipGetErrorString(s_), __FILE__, __LINE__); \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)
#define RSP_OR_FAIL(stat)                                                                       \
    do {                                                                                        \
        rsp_status_t s_ = (stat);                                                               \
        if (s_ != RSP_STATUS_SUCCESS) {                                                         \
            fprintf(stderr, "RSP Error: %d (%s) %s %d\n", (int)s_, rsp_get_error_string(s_),    \
                    __FILE__, __LINE__);                                                        \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

static void demote(void *dst, const double *src, size_t n, int fp32) {
    for (size_t k = 0; k < n; k++) {
        if (fp32)
            ((float *)dst)[k] = (float)src[k];
        else
            ((double *)dst)[k] = src[k];
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr,
                "-- Usage --\n"
                "  %s <A.mtx | surrogate:NAME[@scale]> [--prec=fp64|fp32] [--precond=fp64|fp32|none]\n"
                "     [--ftz] [--rtol=R] [--maxit=N] [--full-symmetric] [--dump=FILE]\n"
                "     [--method=bicgstab|gmres|cg] [--restart=M]\n"
                "     [--refine[=inner_rtol]] [--cheby=K] [--cheby-ratio=R]\n"
                "  solves A x = 1 from x0 = 0 by ILU(0)-preconditioned BiCGStab.\n"
                "  --method=gmres: by restarted flexible GMRES(M) instead (--restart, default 30).\n"
                "  --method=cg: by preconditioned conjugate gradients (A symmetric positive definite).\n"
                "  A symmetric file loads as its lower triangle unless --full-symmetric is given\n"
                "  or --method=cg, which needs both triangles, is.\n"
                "  --refine: mixed-precision iterative refinement, fp64 residuals around all-fp32\n"
                "  solves by --method to inner_rtol (default 1e-4); needs --prec=fp64 and\n"
                "  --precond=fp32 or none.\n"
                "  --cheby=K: the degree-K Chebyshev polynomial preconditioner in the --precond type\n"
                "  instead of ILU(0), on [lmax / R, lmax] (--cheby-ratio=R, default 30).\n",
                argv[0]);
        return 2;
    }
    const char *prec = drv_flag(argc, argv, 2, "prec");
    const char *precond = drv_flag(argc, argv, 2, "precond");
    const char *dump = drv_flag(argc, argv, 2, "dump");
    const char *rtol_s = drv_flag(argc, argv, 2, "rtol");
    const char *maxit_s = drv_flag(argc, argv, 2, "maxit");
    const char *method = drv_flag(argc, argv, 2, "method");
    const char *restart_s = drv_flag(argc, argv, 2, "restart");
    const int gmres = method && strcmp(method, "gmres") == 0;
    const int cg = method && strcmp(method, "cg") == 0;
    const int restart = restart_s && *restart_s ? atoi(restart_s) : 30;
    const char *refine_s = drv_flag(argc, argv, 2, "refine");
    const int refine = refine_s != NULL;
    const double inner_rtol = refine_s && *refine_s ? atof(refine_s) : 1e-4;
    const char *cheby_s = drv_flag(argc, argv, 2, "cheby");
    const char *ratio_s = drv_flag(argc, argv, 2, "cheby-ratio");
    const int cheby = cheby_s != NULL;
    const int cheby_degree = cheby_s && *cheby_s ? atoi(cheby_s) : 4;
    const double cheby_ratio = ratio_s && *ratio_s ? atof(ratio_s) : 30.0;
    if (method && *method && !gmres && !cg && strcmp(method, "bicgstab") != 0) {
        fprintf(stderr, "Error: --method is bicgstab, gmres or cg\n");
        return 2;
    }
    const int fp32 = prec && strcmp(prec, "fp32") == 0;
    const int ftz = drv_flag(argc, argv, 2, "ftz") != NULL;
    const int fullsym = cg || drv_flag(argc, argv, 2, "full-symmetric") != NULL;
    const int use_m = !(precond && strcmp(precond, "none") == 0);
    const int m32 = precond && *precond && use_m ? strcmp(precond, "fp32") == 0 : fp32;
    const double rtol = rtol_s && *rtol_s ? atof(rtol_s) : (fp32 ? 1e-4 : 1e-10);
    const int maxit = maxit_s && *maxit_s ? atoi(maxit_s) : 1000;
    if (use_m && fp32 && !m32) {
        fprintf(stderr, "Error: --precond=fp64 is wider than --prec=fp32\n");
        return 2;
    }

    if (cheby && !use_m) {
        fprintf(stderr, "Error: --cheby needs a preconditioner type: --precond=fp64 or fp32\n");
        return 2;
    }

    if (refine && (fp32 || (use_m && !m32))) {
        fprintf(stderr, "Error: --refine needs --prec=fp64 and --precond=fp32 or none\n");
        return 2;
    }

    CSR A;
    if (!drv_load(argv[1], &A, 0, fullsym)) {
        fprintf(stderr, "Error: failed to load %s\n", argv[1]);
        return 1;
    }
    if (A.m != A.n || A.n < 1) {
        fprintf(stderr, "Error: the matrix is not square\n");
        return 1;
    }
    const int n = A.n, nnz_s = A.rowptr[A.m];
    const size_t vsz = fp32 ? sizeof(float) : sizeof(double), msz = m32 ? sizeof(float) : sizeof(double);
    const rsp_datatype_t dt = fp32 ? RSP_R_32F : RSP_R_64F, mt = m32 ? RSP_R_32F : RSP_R_64F;
    void *hv = malloc((size_t)(nnz_s ? nnz_s : 1) * vsz);
    void *hm = malloc((size_t)(nnz_s ? nnz_s : 1) * msz);
    void *hb = malloc((size_t)n * vsz);
    double *ones = (double *)malloc((size_t)n * sizeof(double));
    double *hx = (double *)malloc((size_t)n * sizeof(double));
    double *hax = (double *)malloc((size_t)n * sizeof(double));
    for (int i = 0; i < n; i++) ones[i] = 1.0;
    demote(hv, A.values, (size_t)nnz_s, fp32);
    demote(hm, A.values, (size_t)nnz_s, m32);
    demote(hb, ones, (size_t)n, fp32);

    rsp_handle_t handle = NULL;
    RSP_OR_FAIL(rsp_create(&handle));
    RSP_OR_FAIL(rsp_set_ftz(handle, ftz));

    int *d_rp = NULL, *d_ci = NULL;
    void *d_v = NULL, *d_m = NULL, *d_b = NULL, *d_x = NULL;
    HIP_OR_FAIL(hipMalloc((void **)&d_rp, ((size_t)n + 1) * sizeof(int)));
    HIP_OR_FAIL(hipMalloc((void **)&d_ci, (size_t)(nnz_s ? nnz_s : 1) * sizeof(int)));
    HIP_OR_FAIL(hipMalloc(&d_v, (size_t)(nnz_s ? nnz_s : 1) * vsz));
    HIP_OR_FAIL(hipMalloc(&d_m, (size_t)(nnz_s ? nnz_s : 1) * msz));
    HIP_OR_FAIL(hipMalloc(&d_b, (size_t)n * vsz));
    HIP_OR_FAIL(hipMalloc(&d_x, (size_t)n * vsz));
    HIP_OR_FAIL(hipMemcpy(d_rp, A.rowptr, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIP_OR_FAIL(hipMemcpy(d_ci, A.colidx, (size_t)nnz_s * sizeof(int), hipMemcpyHostToDevice));
    HIP_OR_FAIL(hipMemcpy(d_v, hv, (size_t)nnz_s * vsz, hipMemcpyHostToDevice));
    HIP_OR_FAIL(hipMemcpy(d_m, hm, (size_t)nnz_s * msz, hipMemcpyHostToDevice));
    HIP_OR_FAIL(hipMemcpy(d_b, hb, (size_t)n * vsz, hipMemcpyHostToDevice));
    HIP_OR_FAIL(hipMemset(d_x, 0, (size_t)n * vsz));

    rsp_spmat_t mat = NULL;
    RSP_OR_FAIL(rsp_create_csr(&mat, n, n, A.nnz, d_rp, d_ci, d_v, dt));

    hipEvent_t start, stop;
    HIP_OR_FAIL(hipEventCreate(&start));
    HIP_OR_FAIL(hipEventCreate(&stop));
    float time_symbolic = 0.0f, time_numeric = 0.0f, time_solve = 0.0f;

    rsp_ilu0_info_t info = NULL;
    if (use_m && !cheby) {
        RSP_OR_FAIL(rsp_create_ilu0_info(&info));
        double t0 = drv_wtime();
        RSP_OR_FAIL(rsp_ilu0_analysis(handle, n, A.nnz, d_rp, d_ci, info));
        time_symbolic = (float)((drv_wtime() - t0) * 1e3);
        int pos = -1;
        if (rsp_ilu0_zero_pivot(handle, info, &pos) == RSP_STATUS_ZERO_PIVOT) {
            fprintf(stderr, "Error: A(%d,%d) is missing\n", pos, pos);
            return 1;
        }
        HIP_OR_FAIL(hipEventRecord(start, NULL));
        RSP_OR_FAIL(rsp_ilu0_factor(handle, info, mt, d_m));
        HIP_OR_FAIL(hipEventRecord(stop, NULL));
        HIP_OR_FAIL(hipEventSynchronize(stop));
        HIP_OR_FAIL(hipEventElapsedTime(&time_numeric, start, stop));
    }

    rsp_bicgstab_t solver = NULL;
    rsp_gmres_t gsolver = NULL;
    rsp_cg_t csolver = NULL;
    rsp_refine_t rsolver = NULL;
    rsp_spmat_t mat_low = NULL;
    void *d_vlow = NULL;
    int steps = 0;
    rsp_cheby_t poly = NULL;
    rsp_spmat_t mat_poly = NULL; /* the polynomial's matrix when --precond is narrower than --prec */
    if (refine) {
        HIP_OR_FAIL(hipMalloc(&d_vlow, (size_t)(nnz_s ? nnz_s : 1) * sizeof(float)));
        RSP_OR_FAIL(rsp_convert_scaled(handle, nnz_s, RSP_R_64F, d_v, 0, RSP_R_32F, d_vlow));
        RSP_OR_FAIL(rsp_create_csr(&mat_low, n, n, A.nnz, d_rp, d_ci, d_vlow, RSP_R_32F));
    }
    if (cheby) {
        rsp_spmat_t on = refine ? mat_low : mat;
        if (!refine && m32 != fp32) {
            RSP_OR_FAIL(rsp_create_csr(&mat_poly, n, n, A.nnz, d_rp, d_ci, d_m, mt));
            on = mat_poly;
        }
        int pos = -1;
        double t0 = drv_wtime();
        rsp_status_t st = rsp_cheby_create(handle, on, cheby_degree, RSP_CHEBY_SCALE_JACOBI, cheby_ratio, &pos, &poly);
        time_symbolic = (float)((drv_wtime() - t0) * 1e3);
        if (st == RSP_STATUS_ZERO_PIVOT) {
            fprintf(stderr, "Error: A(%d,%d) is missing or zero\n", pos, pos);
            return 1;
        }
        RSP_OR_FAIL(st);
    }
    if (refine) {
        const rsp_refine_method_t rm = gmres ? RSP_REFINE_GMRES : (cg ? RSP_REFINE_CG : RSP_REFINE_BICGSTAB);
        if (cheby)
            RSP_OR_FAIL(rsp_refine_create_cheby(handle, mat, mat_low, poly, rm, restart, &rsolver));
        else
            RSP_OR_FAIL(rsp_refine_create(handle, mat, mat_low, info, d_m, rm, restart, &rsolver));
    } else if (cheby) {
        if (gmres)
            RSP_OR_FAIL(rsp_gmres_create_cheby(handle, mat, poly, restart, &gsolver));
        else if (cg)
            RSP_OR_FAIL(rsp_cg_create_cheby(handle, mat, poly, &csolver));
        else
            RSP_OR_FAIL(rsp_bicgstab_create_cheby(handle, mat, poly, &solver));
    } else if (gmres)
        RSP_OR_FAIL(rsp_gmres_create(handle, mat, info, mt, d_m, restart, &gsolver));
    else if (cg)
        RSP_OR_FAIL(rsp_cg_create(handle, mat, info, mt, d_m, &csolver));
    else
        RSP_OR_FAIL(rsp_bicgstab_create(handle, mat, info, mt, d_m, &solver));
    int iters = 0;
    double relres = 0.0;
    rsp_solve_reason_t reason = RSP_SOLVE_MAX_ITERS;
    HIP_OR_FAIL(hipEventRecord(start, NULL));
    if (refine)
        RSP_OR_FAIL(rsp_refine_solve(handle, rsolver, d_b, d_x, rtol, 50, inner_rtol, maxit, 1, &steps, &iters, &relres,
                                     &reason));
    else if (gmres)
        RSP_OR_FAIL(rsp_gmres_solve(handle, gsolver, d_b, d_x, rtol, maxit, 1, &iters, &relres, &reason));
    else if (cg)
        RSP_OR_FAIL(rsp_cg_solve(handle, csolver, d_b, d_x, rtol, maxit, 1, &iters, &relres, &reason));
    else
        RSP_OR_FAIL(rsp_bicgstab_solve(handle, solver, d_b, d_x, rtol, maxit, 1, &iters, &relres, &reason));
    HIP_OR_FAIL(hipEventRecord(stop, NULL));
    HIP_OR_FAIL(hipEventSynchronize(stop));
    HIP_OR_FAIL(hipEventElapsedTime(&time_solve, start, stop));

    /* the true residual, fp64 on the host */
    void *hxt = malloc((size_t)n * vsz);
    HIP_OR_FAIL(hipMemcpy(hxt, d_x, (size_t)n * vsz, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) hx[i] = fp32 ? (double)((float *)hxt)[i] : ((double *)hxt)[i];
    rsp_host_spmv_f64(n, A.rowptr, A.colidx, A.values, hx, hax);
    double rn = 0.0, bn = 0.0;
    for (int i = 0; i < n; i++) {
        const double d = ones[i] - hax[i];
        rn += d * d;
        bn += ones[i] * ones[i];
    }

    printf(fp32 ? "SINGLE PRECISION ITERATION IN  MILLISECONDS\n " : "DOUBLE PRECISION ITERATION IN  MILLISECONDS\n ");
    printf("Symbolic = %f\n Numeric = %f \n Solve = %f\n Iterations = %d\n Reason = %d\n Relative residual = %e\n",
           time_symbolic, time_numeric, time_solve, iters, (int)reason, sqrt(rn) / sqrt(bn));
    if (refine) printf(" Refinement steps = %d\n Inner iterations = %d\n", steps, iters);

    if (dump && *dump) {
        FILE *fp = fopen(dump, "wb");
        if (fp) {
            fwrite(hxt, vsz, (size_t)n, fp);
            fclose(fp);
        }
    }

    hipEventDestroy(start);
    hipEventDestroy(stop);
    if (refine) {
        rsp_refine_destroy(rsolver);
        rsp_destroy_spmat(mat_low);
        hipFree(d_vlow);
    } else if (gmres)
        rsp_gmres_destroy(gsolver);
    else if (cg)
        rsp_cg_destroy(csolver);
    else
        rsp_bicgstab_destroy(solver);
    if (info) rsp_destroy_ilu0_info(info);
    if (poly) rsp_cheby_destroy(poly);
    if (mat_poly) rsp_destroy_spmat(mat_poly);
    rsp_destroy_spmat(mat);
    rsp_destroy(handle);
    hipFree(d_rp);
    hipFree(d_ci);
    hipFree(d_v);
    hipFree(d_m);
    hipFree(d_b);
    hipFree(d_x);
    free(hv);
    free(hm);
    free(hb);
    free(ones);
    free(hx);
    free(hax);
    free(hxt);
    rsp_csr_free(&A);
    return 0;
}
