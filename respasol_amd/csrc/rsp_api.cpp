// rsp_api.cpp — the handle, the matrix descriptor and SpMV of include/rsp.h
// (the C-ABI operator library librsp.so): the upload of the host-side
// row-block schedule (spmv_plan.h), the launches of the kernels in spmv.hip,
// the batch, gather / scatter. Mirrors the cuSPARSE lifecycle the reference
// driver uses (GPU/spmv.cu:122-186); see include/rsp.h for the per-call
// mapping. ILU(0) and the Krylov solvers: api_ilu_analysis.cpp,
// api_ilu_solve.cpp, api_krylov.cpp (rsp_internal.h).

#include "rsp_internal.h"

#include <atomic>

using namespace rsp_api;

using rsp::SpmvBlock;
using rsp::SpmvLongRow;
using rsp_plan::PlanOptions;
using rsp_plan::TilePlan;

namespace {
std::atomic<unsigned long long> g_plan_next{1};
unsigned long long plan_new_gen() { return g_plan_next.fetch_add(1); }
}  // namespace

/* ----------------------------------------------------------------- SpMV */

static int64_t spmv_resident_tiles(rsp_handle_t h, rsp_datatype_t t) {
    return (int64_t)rsp_k::spmv_tiles_per_cu((int)elem_size(t)) * h->num_cus;
}

// The planner's options for a matrix of `local_cols` under the handle's
// RSP_SPMV_VARIANT (plan-time bits): bit 5 keeps every tile on the int32
// indices, bit 6 aligns the tile row cuts to 128-B y lines, bit 7 to 64 B
// (tuning knob; default unaligned), kSpmvVariantNoStage: no staged tiles.
// `spread`: PlanOptions::spread.
static PlanOptions handle_plan_options(rsp_handle_t h, rsp_datatype_t t, int64_t local_cols, int64_t spread) {
    const int e = (int)elem_size(t), v = h->spmv_variant;
    PlanOptions o = rsp_plan::plan_options(t);
    o.spread = spread;
    o.local_cols = local_cols;
    o.row_align = (v & 64) ? 128 / e : (v & 128) ? 64 / e : 1;
    o.use_c16 = !(v & 32);
    o.use_stage = !(v & rsp::kSpmvVariantNoStage);
    return o;
}

// Row offsets and column indices of `mat` on the host, validated (base 0,
// non-decreasing offsets, columns inside [0, cols)).
static rsp_status_t download_pattern(rsp_handle_t h, rsp_spmat_t mat, rsp_an::hvec<int> &rp,
                                     rsp_an::hvec<int> &ci) {
    const int m = (int)mat->rows;
    rp.assign((size_t)m + 1, 0);
    ci.clear();
    if (m > 0) {
        RSP_CHECK_HIP(hipMemcpyAsync(rp.data(), mat->rowptr, ((size_t)m + 1) * sizeof(int),
                                     hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    }
    if (m > 0 && rp[0] != 0) return RSP_STATUS_INVALID_VALUE;  // base 0 only
    for (int i = 0; i < m; i++)
        if (rp[i + 1] < rp[i]) return RSP_STATUS_INVALID_VALUE;
    // the stored entries must lie inside the colidx / vals arrays (nnz long)
    if (m > 0 && (int64_t)rp[(size_t)m] > mat->nnz) return RSP_STATUS_INVALID_VALUE;
    // Column indices are gathered unchecked by the kernel: validate them once
    // here (outside the timed loop) so a malformed matrix is an INVALID_VALUE
    // status, never an out-of-bounds read of x on the GPU.
    if (m > 0 && rp[(size_t)m] > 0) {
        if (!mat->colidx) return RSP_STATUS_INVALID_VALUE;
        ci.resize((size_t)rp[(size_t)m]);
        RSP_CHECK_HIP(hipMemcpyAsync(ci.data(), mat->colidx, ci.size() * sizeof(int),
                                     hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
        const int ncols = (int)mat->cols;
        for (int c : ci)
            if ((unsigned)c >= (unsigned)ncols) return RSP_STATUS_INVALID_VALUE;
    }
    return RSP_STATUS_SUCCESS;
}

// Build the schedule of `mat` for `compute_type` into the matrix's own device
// memory (host-blocking; see struct rsp_spmat).
rsp_status_t rsp_api::spmv_plan(rsp_handle_t h, rsp_spmat_t mat, rsp_datatype_t compute_type) {
    const int m = (int)mat->rows;
    rsp_an::hvec<int> rp, ci;
    rsp_status_t st = download_pattern(h, mat, rp, ci);
    if (st != RSP_STATUS_SUCCESS) return st;
    // Full tiles for every matrix. Rounds 3-4 spread a scattered (circuit)
    // matrix with fewer tiles than resident slots over up to that many small
    // tiles; once the row reduce stopped stalling on 33-256-entry rows (round
    // 5: branch-free steps, heavy rows eight lanes each) the full tiles are
    // faster per call: dc1 8.75 -> 7.02 us, G2_circuit 8.13 -> 6.10, ASIC_320ks
    // 11.77 -> 9.22, ss1 8.49 -> 6.61, matrix-new_3 9.10 -> 6.71
    // (profiles/r05_heavy_rows_ab.txt). RSP_SPMV_VARIANT bit 9 still spreads
    // every small matrix (A/B). A batch re-plans its members itself
    // (rsp_spmv_batch_create). Tiling never changes the result (canonical
    // summation order).
    const bool spread = (h->spmv_variant & 512) != 0;
    TilePlan p;
    rsp_plan::make_tile_plan(rp.data(), ci.data(), m, mat->nnz,
                             handle_plan_options(h, compute_type, mat->local_cols,
                                                 spread ? spmv_resident_tiles(h, compute_type) : 0),
                             p);
    // exact layout of this schedule in the matrix's device memory (grown,
    // never shrunk, on a re-plan)
    const size_t elem = elem_size(compute_type);
    const rsp_plan::SpmvLayout lay = rsp_plan::spmv_layout({p.blocks.size(), p.longrows.size(), (size_t)p.nslots},
                                                           elem, (int64_t)p.c16.size(), p.runs.size());
    mat->planned = 0;
    if (lay.bytes > mat->plan_cap || !mat->d_plan) {
        if (mat->d_plan) {
            int cur = 0;
            (void)hipGetDevice(&cur);
            (void)hipSetDevice(mat->plan_device);
            (void)hipFree(mat->d_plan);
            (void)hipSetDevice(cur);
            mat->d_plan = nullptr;
            mat->plan_cap = 0;
        }
        RSP_CHECK_HIP(hipMalloc(&mat->d_plan, std::max<size_t>(lay.bytes, 256)));
        mat->plan_cap = std::max<size_t>(lay.bytes, 256);
        RSP_CHECK_HIP(hipGetDevice(&mat->plan_device));
    }
    char *buf = (char *)mat->d_plan;
    auto upload = [&](size_t off, const void *src, size_t bytes) {
        return bytes == 0 ? hipSuccess : hipMemcpyAsync(buf + off, src, bytes, hipMemcpyHostToDevice, h->stream);
    };
    RSP_CHECK_HIP(upload(0, p.blocks.data(), p.blocks.size() * sizeof(SpmvBlock)));
    RSP_CHECK_HIP(upload(lay.off_cbase, p.cbase.data(), p.cbase.size() * sizeof(int)));
    RSP_CHECK_HIP(upload(lay.off_poff, p.poff.data(), p.poff.size() * sizeof(int)));
    RSP_CHECK_HIP(upload(lay.off_cidx, p.c16.data(), p.c16.size() * sizeof(uint16_t)));
    RSP_CHECK_HIP(upload(lay.off_runs, p.runs.data(), p.runs.size() * sizeof(int)));
    RSP_CHECK_HIP(upload(lay.off_long, p.longrows.data(), p.longrows.size() * sizeof(SpmvLongRow)));
    // partial slots: the long rows' arrival tickets start (and stay) at 0
    if (p.nslots > 0)
        RSP_CHECK_HIP(hipMemsetAsync(buf + lay.off_part, 0, (size_t)p.nslots * 2 * elem, h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    mat->planned = 1;
    mat->plan_type = compute_type;
    mat->nblocks = (int)p.blocks.size();
    mat->nint = p.nint;
    mat->plan_gen = plan_new_gen();
    mat->nlong = (int)p.longrows.size();
    mat->nslots = p.nslots;
    mat->nnz_s = m > 0 ? rp[(size_t)m] : 0;
    mat->lay = lay;
    mat->nnz_c16 = p.nnz_c16;
    mat->nnz_staged = p.nnz_staged;
    return RSP_STATUS_SUCCESS;
}

/* ------------------------------------------------- the transposed side */

// The pattern of `mat` downloaded, validated and transposed on the host
// (csr_transpose.h): what rsp_spmv(op = TRANSPOSE) and rsp_csr2csc share.
struct HostTranspose {
    rsp_an::hvec<int> rowptr, colidx, perm;
    int64_t nnz = 0;  // rowptr[rows] of mat
};

static rsp_status_t transpose_pattern(rsp_handle_t h, rsp_spmat_t mat, HostTranspose &t) {
    rsp_an::hvec<int> rp, ci;
    RSP_TRY(download_pattern(h, mat, rp, ci));
    t.nnz = mat->rows > 0 ? rp[(size_t)mat->rows] : 0;
    if (mat->cols > INT_MAX - 1) return RSP_STATUS_INVALID_VALUE;  // A^T's rows
    t.rowptr.assign((size_t)mat->cols + 1, 0);
    t.colidx.assign((size_t)t.nnz, 0);
    t.perm.assign((size_t)t.nnz, 0);
    return rsp_tr::csr_transpose(mat->rows, mat->cols, rp.data(), ci.data(), t.rowptr.data(), t.colidx.data(),
                                 t.perm.data());
}

static hipError_t upload_ints(rsp_handle_t h, void *dst, const rsp_an::hvec<int> &src) {
    return src.empty() ? hipSuccess
                       : hipMemcpyAsync(dst, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, h->stream);
}

// (Re)build the transposed side of `mat` from its pattern as it is now
// (host-blocking): pattern, permutation, room for the values and the child's
// schedule. The old side, if any, is dropped only once the new one stands.
static rsp_status_t tside_build(rsp_handle_t h, rsp_spmat_t mat) {
    HostTranspose ht;
    RSP_TRY(transpose_pattern(h, mat, ht));
    std::unique_ptr<rsp_spmat_tside> t(new rsp_spmat_tside());
    RSP_CHECK_HIP(hipGetDevice(&t->device));
    const size_t off_ci = align256(ht.rowptr.size() * sizeof(int));
    const size_t off_perm = off_ci + align256(ht.colidx.size() * sizeof(int));
    const size_t bytes = off_perm + std::max<size_t>(align256(ht.perm.size() * sizeof(int)), 256);
    RSP_CHECK_HIP(hipMalloc(&t->pattern.p, bytes));
    RSP_CHECK_HIP(hipMalloc(&t->vt.p, std::max<size_t>((size_t)ht.nnz * elem_size(mat->type), 256)));
    char *buf = (char *)t->pattern.p;
    RSP_CHECK_HIP(upload_ints(h, buf, ht.rowptr));
    RSP_CHECK_HIP(upload_ints(h, buf + off_ci, ht.colidx));
    RSP_CHECK_HIP(upload_ints(h, buf + off_perm, ht.perm));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    t->perm = (int *)(buf + off_perm);
    rsp_spmat &c = t->child;  // (value-initialised: no schedule yet)
    c.rows = mat->cols;
    c.cols = mat->rows;
    c.nnz = ht.nnz;
    c.rowptr = (int *)buf;
    c.colidx = (int *)(buf + off_ci);
    c.vals = t->vt.p;
    c.type = mat->type;
    c.local_cols = -1;
    RSP_TRY(rsp_api::spmv_plan(h, &c, c.type));
    rsp_k::warm_transpose();  // (the permutation's code object, outside the timed calls)
    delete mat->tside;
    mat->tside = t.release();
    return RSP_STATUS_SUCCESS;
}

// The transposed side of `mat`, built if absent, its values' room and the
// child's type brought up to the matrix's (rsp_csr_set_values to the other
// type: the pattern arrays and the permutation stay, the child re-plans).
static rsp_status_t tside_ready(rsp_handle_t h, rsp_spmat_t mat) {
    if (!mat->tside) return tside_build(h, mat);
    rsp_spmat_tside *t = mat->tside;
    if (t->child.type != mat->type) {
        DevMem v;
        RSP_CHECK_HIP(hipMalloc(&v.p, std::max<size_t>((size_t)t->child.nnz * elem_size(mat->type), 256)));
        t->vt = std::move(v);  // (the old values go with v)
        t->child.vals = t->vt.p;
        t->child.type = mat->type;
        t->child.planned = 0;
    }
    return RSP_STATUS_SUCCESS;
}

// y = alpha * A^T * x + beta * y: the permutation of the values as they are
// now, then the ordinary product of the child, both on the handle's stream.
static rsp_status_t spmv_run_transposed(rsp_handle_t h, const void *alpha, rsp_spmat_t mat, const void *d_x,
                                        const void *beta, void *d_y, rsp_datatype_t compute_type, void *d_buffer) {
    if (compute_type != mat->type) return RSP_STATUS_INVALID_VALUE;
    if ((mat->rows > 0 && !d_x) || (mat->cols > 0 && !d_y)) return RSP_STATUS_INVALID_VALUE;
    RSP_TRY(tside_ready(h, mat));
    rsp_spmat_tside *t = mat->tside;
    if (t->child.nnz > 0 && !mat->vals) return RSP_STATUS_INVALID_VALUE;
    if (rsp_k::permute_values((int)elem_size(compute_type), t->child.nnz, t->perm, mat->vals, t->vt.p, h->num_cus,
                              h->stream) != hipSuccess)
        return RSP_STATUS_EXECUTION_FAILED;
    return rsp_api::spmv_run(h, RSP_OPERATION_NON_TRANSPOSE, alpha, &t->child, d_x, beta, d_y, compute_type,
                             d_buffer, 0);
}

rsp_status_t rsp_api::spmv_run(rsp_handle_t h, rsp_operation_t op, const void *alpha, rsp_spmat_t mat,
                               const void *d_x, const void *beta, void *d_y,
                               rsp_datatype_t compute_type, void *d_buffer, int part) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!mat || !alpha || !beta) return RSP_STATUS_INVALID_VALUE;
    if (op == RSP_OPERATION_TRANSPOSE && part == 0)
        return spmv_run_transposed(h, alpha, mat, d_x, beta, d_y, compute_type, d_buffer);
    if (op != RSP_OPERATION_NON_TRANSPOSE) return RSP_STATUS_NOT_SUPPORTED;
    if (compute_type != mat->type) return RSP_STATUS_INVALID_VALUE;
    if (mat->rows > 0 && (!d_y || (mat->cols > 0 && !d_x))) return RSP_STATUS_INVALID_VALUE;
    (void)d_buffer;  // the schedule lives in the matrix (struct rsp_spmat)
    if (!mat->planned || mat->plan_type != compute_type) {  // lazily, if bufferSize was skipped
        rsp_status_t st = spmv_plan(h, mat, compute_type);
        if (st != RSP_STATUS_SUCCESS) return st;
    }
    char *plan = (char *)mat->d_plan;
    rsp::SpmvArgs a;
    a.m = (int)mat->rows;
    a.rowptr = mat->rowptr;
    a.colidx = mat->colidx;
    a.vals = mat->vals;
    a.x = d_x;
    a.y = d_y;
    a.blocks = (const SpmvBlock *)plan;
    a.nblocks = mat->nblocks;
    a.cbases = (const int *)(plan + mat->lay.off_cbase);
    a.poffs = (const int *)(plan + mat->lay.off_poff);
    a.cidx = (const unsigned short *)(plan + mat->lay.off_cidx);
    a.runs = (const int *)(plan + mat->lay.off_runs);
    a.cmax = mat->cols > 0 ? (int)(mat->cols - 1) : 0;
    a.longrows = (const SpmvLongRow *)(plan + mat->lay.off_long);
    a.nlong = mat->nlong;
    a.partials = plan + mat->lay.off_part;
    if (compute_type == RSP_R_64F) {
        a.alpha = *(const double *)alpha;
        a.beta = *(const double *)beta;
    } else {
        a.alpha = *(const float *)alpha;
        a.beta = *(const float *)beta;
    }
    if (part != 0) {  // split schedule: part 1 = interior tiles, part 2 = the rest + fixup
        if (a.beta != 0.0) return RSP_STATUS_INVALID_VALUE;
        if (part == 1) {
            a.nblocks = mat->nint;
            a.nlong = 0;
        } else {
            a.blocks += mat->nint;
            a.cbases += mat->nint;
            a.poffs += mat->nint;
            a.nblocks = mat->nblocks - mat->nint;
        }
    }
    a.vector_ok = ((((uintptr_t)mat->colidx) | ((uintptr_t)mat->vals)) & 15) == 0;
    a.nnz = mat->nnz_s;
    a.variant = h->spmv_variant;
    hipError_t e;
    if (compute_type == RSP_R_64F)
        e = rsp_k::spmv_f64(a, h->stream);
    else
        e = h->ftz ? rsp_k_ftz::spmv_f32(a, h->stream) : rsp_k::spmv_f32(a, h->stream);
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

/* ------------------------------------------------------- batched SpMV */

struct rsp_spmv_batch {
    rsp_datatype_t type;
    int part;
    rsp_an::hvec<rsp_spmat_t> mats;
    rsp_an::hvec<unsigned long long> plan_gen;  // schedules as copied (stale check)
    rsp_an::hvec<rsp::SpmvBatchArgs> launches;  // one per kSpmvBatchMax matrices
    void *d_mem = nullptr;                      // entries, tiles, long rows of every launch
    int64_t tiles = 0, entries_16bit = 0;       // rsp_spmv_batch_info
    ~rsp_spmv_batch() {
        if (d_mem) (void)hipFree(d_mem);
    }
};

static rsp_status_t spmv_batch_create(rsp_handle_t h, int count, const rsp_spmat_t *mats,
                                      const void *const *d_x, void *const *d_y,
                                      void *const *d_buffers, rsp_datatype_t compute_type,
                                      int part, rsp_spmv_batch_t *batch) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    (void)d_buffers;  // workspaces are not needed: schedules live in the matrices
    if (!batch || count < 0 || (count > 0 && (!mats || !d_x || !d_y)))
        return RSP_STATUS_INVALID_VALUE;
    if (part < 0 || part > 2) return RSP_STATUS_INVALID_VALUE;
    if (compute_type != RSP_R_64F && compute_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    *batch = nullptr;
    for (int j = 0; j < count; j++) {
        rsp_spmat_t A = mats[j];
        if (!A) return RSP_STATUS_INVALID_VALUE;
        if (A->type != compute_type) return RSP_STATUS_INVALID_VALUE;
        if (A->rows > 0 && (!d_y[j] || (A->cols > 0 && !d_x[j]))) return RSP_STATUS_INVALID_VALUE;
        if (!A->planned || A->plan_type != compute_type) {
            rsp_status_t st = spmv_plan(h, A, compute_type);
            if (st != RSP_STATUS_SUCCESS) return st;
        }
    }
    std::unique_ptr<rsp_spmv_batch> b(new rsp_spmv_batch());
    b->type = compute_type;
    b->part = part;
    // The batch carries its own schedules. Each matrix's own plan is spread
    // over the whole chip for a lone launch (rsp_spmv_preprocess); in a
    // batch that only shrinks the tiles, which cost the moderate set 35 %
    // (0.145 vs 0.108 ms per step). So members are planned with
    // full tiles, and spread only when the launch's tiles together do not
    // fill the resident slots (each matrix over its nnz share of them).
    // Long rows and their partial slots are the same in every spread of a
    // matrix; the batch keeps its own partials and tickets per member, so a
    // matrix may appear in several batches and several times in one (the
    // same A with several right-hand sides), and a batch never shares
    // tickets with single calls of its matrices.
    const int64_t R = spmv_resident_tiles(h, compute_type);
    const bool spread_ok = !(h->spmv_variant & 16);
    rsp_an::hvec<TilePlan> plans((size_t)count);
    // layout: per launch [entries | tiles | tile column bases | tile record
    // offsets | long rows | 16-bit column offsets of each matrix | runs and
    // records of each matrix | long-row partials and tickets of each matrix
    // (zero)], each 16-B aligned
    struct Region { size_t off, len; };
    struct Span {
        int first, count, nt, nl;  // members [first, first + count); their tiles and long rows in this launch
        rsp_an::hvec<Region> reg;  // in layout order: the five shared regions, then three per member
        enum { kEntries, kTiles, kCbases, kPoffs, kLongRows, kC16, kRuns, kPartials };
        const Region &at(int kind, int q) const { return reg[kind < kC16 ? kind : kC16 + (kind - kC16) * count + q]; }
    };
    rsp_an::hvec<Span> spans;
    size_t bytes = 0;
    auto tile_range = [part](const TilePlan &p, int *t0, int *t1) {
        *t0 = part == 2 ? p.nint : 0;
        *t1 = part == 1 ? p.nint : (int)p.blocks.size();
    };
    for (int first = 0; first < count; first += rsp::kSpmvBatchMax) {
        Span sp{first, std::min(rsp::kSpmvBatchMax, count - first), 0, 0, {}};
        rsp_an::hvec<rsp_an::hvec<int>> rps((size_t)sp.count), cis((size_t)sp.count);
        auto plan_members = [&](int64_t spread_all, int64_t nnz_all) {  // spread_all: of the launch, 0 = full tiles
            sp.nt = 0;
            for (int q = 0; q < sp.count; q++) {
                rsp_spmat_t A = mats[first + q];
                const int64_t nnz_q = A->rows > 0 ? rps[q][(size_t)A->rows] : 0;
                const int64_t share =
                    spread_all > 0 ? std::max<int64_t>(1, spread_all * nnz_q / std::max<int64_t>(1, nnz_all)) : 0;
                TilePlan &p = plans[first + q];
                rsp_plan::make_tile_plan(rps[q].data(), cis[q].data(), (int)A->rows, A->nnz,
                                         handle_plan_options(h, compute_type, A->local_cols, share), p);
                int t0, t1;
                tile_range(p, &t0, &t1);
                sp.nt += t1 - t0;
            }
        };
        int64_t nnz_all = 0;
        for (int q = 0; q < sp.count; q++) {
            rsp_spmat_t A = mats[first + q];
            rsp_status_t st = download_pattern(h, A, rps[q], cis[q]);
            if (st != RSP_STATUS_SUCCESS) return st;
            nnz_all += A->rows > 0 ? rps[q][(size_t)A->rows] : 0;
        }
        plan_members(0, nnz_all);
        if (spread_ok && sp.nt < R) plan_members(R, nnz_all);
        for (int q = 0; q < sp.count; q++) {
            const TilePlan &p = plans[first + q];
            rsp_spmat_t A = mats[first + q];
            // the long rows index partial slots of the matrix's own workspace
            if ((int)p.longrows.size() != A->nlong || p.nslots != A->nslots)
                return RSP_STATUS_INTERNAL_ERROR;
            sp.nl += part == 1 ? 0 : (int)p.longrows.size();
        }
        sp.reg = {{0, (size_t)sp.count * sizeof(rsp::SpmvBatchEntry)},
                  {0, (size_t)sp.nt * sizeof(SpmvBlock)},
                  {0, (size_t)sp.nt * sizeof(int)},
                  {0, (size_t)sp.nt * sizeof(int)},
                  {0, (size_t)sp.nl * sizeof(SpmvLongRow)}};
        for (int q = 0; q < sp.count; q++) sp.reg.push_back({0, plans[first + q].c16.size() * sizeof(uint16_t)});
        for (int q = 0; q < sp.count; q++) sp.reg.push_back({0, plans[first + q].runs.size() * sizeof(int)});
        for (int q = 0; q < sp.count; q++)
            sp.reg.push_back({0, (size_t)plans[first + q].nslots * 2 * elem_size(compute_type)});
        for (Region &r : sp.reg) {
            r.off = bytes;
            bytes += (r.len + 15) & ~(size_t)15;
        }
        spans.push_back(sp);
    }
    // Layout invariant (the round-4 fault was a zero-fill that reached the
    // entries and tiles of a later launch): every region of every launch lies
    // inside the allocation, after the previous one, and overlaps no other;
    // in particular each member's partials and tickets (zeros of the image,
    // written by nothing else here) are its own.
    {
        size_t end = 0;
        for (const Span &sp : spans)
            for (const Region &r : sp.reg) {
                if (r.off < end || r.off + r.len > bytes) return RSP_STATUS_INTERNAL_ERROR;
                end = r.off + r.len;
            }
    }
    if (bytes > 0) RSP_CHECK_HIP(hipMalloc(&b->d_mem, bytes));
    rsp_an::hvec<unsigned char> host(bytes);
    bool fits = true;  // every copy of the fill lies inside the region the layout gave it
    for (const Span &sp : spans) {
        auto dev = [&](int kind, int q = 0) { return (char *)b->d_mem + sp.at(kind, q).off; };
        auto put = [&](int kind, int q, size_t at, const void *src, size_t n) {
            const Region &r = sp.at(kind, q);
            if (at + n > r.len)
                fits = false;
            else if (n > 0)
                memcpy(host.data() + r.off + at, src, n);
        };
        rsp::SpmvBatchArgs a{};
        a.entries = (const rsp::SpmvBatchEntry *)dev(Span::kEntries);
        a.tiles = (const SpmvBlock *)dev(Span::kTiles);
        a.cbases = (const int *)dev(Span::kCbases);
        a.poffs = (const int *)dev(Span::kPoffs);
        a.longrows = (const SpmvLongRow *)dev(Span::kLongRows);
        a.count = sp.count;
        for (int q = 0; q <= rsp::kSpmvBatchMax; q++)
            a.tiles_at.begin[q] = a.longs_at.begin[q] = INT_MAX;
        size_t nt = 0, nl = 0;
        for (int q = 0; q < sp.count; q++) {
            rsp_spmat_t A = mats[sp.first + q];
            const TilePlan &p = plans[sp.first + q];
            int t0, t1;
            tile_range(p, &t0, &t1);
            const size_t ntq = (size_t)(t1 - t0), nlq = part == 1 ? 0 : p.longrows.size();
            rsp::SpmvBatchEntry e{};
            e.rowptr = A->rowptr;
            e.colidx = A->colidx;
            e.vals = A->vals;
            e.x = d_x[sp.first + q];
            e.y = d_y[sp.first + q];
            e.partials = (void *)dev(Span::kPartials, q);  // this member's own
            e.cidx = (const unsigned short *)dev(Span::kC16, q);
            e.runs = (const int *)dev(Span::kRuns, q);
            e.cmax = A->cols > 0 ? (int)(A->cols - 1) : 0;
            e.nnz = A->nnz_s;
            e.vector_ok = ((((uintptr_t)A->colidx) | ((uintptr_t)A->vals)) & 15) == 0;
            put(Span::kEntries, 0, (size_t)q * sizeof(e), &e, sizeof(e));
            a.tiles_at.begin[q] = (int)nt;
            a.longs_at.begin[q] = (int)nl;
            for (int t = t0; t < t1; t++)
                if (p.cbase[(size_t)t] != rsp_plan::kCbaseInt32)
                    b->entries_16bit += p.blocks[(size_t)t].k1 - p.blocks[(size_t)t].k0;
            b->tiles += (int64_t)ntq;
            put(Span::kTiles, 0, nt * sizeof(SpmvBlock), p.blocks.data() + t0, ntq * sizeof(SpmvBlock));
            put(Span::kCbases, 0, nt * sizeof(int), p.cbase.data() + t0, ntq * sizeof(int));
            put(Span::kPoffs, 0, nt * sizeof(int), p.poff.data() + t0, ntq * sizeof(int));
            put(Span::kLongRows, 0, nl * sizeof(SpmvLongRow), p.longrows.data(), nlq * sizeof(SpmvLongRow));
            put(Span::kC16, q, 0, p.c16.data(), p.c16.size() * sizeof(uint16_t));
            put(Span::kRuns, q, 0, p.runs.data(), p.runs.size() * sizeof(int));
            nt += ntq;
            nl += nlq;
        }
        a.tiles_at.begin[sp.count] = (int)nt;
        a.longs_at.begin[sp.count] = (int)nl;
        b->launches.push_back(a);
    }
    if (!fits) return RSP_STATUS_INTERNAL_ERROR;
    // the image is value-initialised, so every member's long-row partials and
    // tickets go up as 0 (tickets start, and stay, at 0 between launches)
    // (on the handle's stream; create is host-blocking and `host` is freed on return)
    if (bytes > 0) {
        RSP_CHECK_HIP(hipMemcpyAsync(b->d_mem, host.data(), bytes, hipMemcpyHostToDevice, h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    }
    for (int j = 0; j < count; j++) {
        b->mats.push_back(mats[j]);
        b->plan_gen.push_back(mats[j]->plan_gen);
    }
    *batch = b.release();
    return RSP_STATUS_SUCCESS;
}

extern "C" {

int rsp_get_version(void) { return RSP_VERSION_MAJOR * 1000 + RSP_VERSION_MINOR; }

const char *rsp_get_error_string(rsp_status_t s) {
    switch (s) {
        case RSP_STATUS_SUCCESS: return "RSP_STATUS_SUCCESS";
        case RSP_STATUS_NOT_INITIALIZED: return "RSP_STATUS_NOT_INITIALIZED";
        case RSP_STATUS_ALLOC_FAILED: return "RSP_STATUS_ALLOC_FAILED";
        case RSP_STATUS_INVALID_VALUE: return "RSP_STATUS_INVALID_VALUE";
        case RSP_STATUS_ARCH_MISMATCH: return "RSP_STATUS_ARCH_MISMATCH";
        case RSP_STATUS_EXECUTION_FAILED: return "RSP_STATUS_EXECUTION_FAILED";
        case RSP_STATUS_INTERNAL_ERROR: return "RSP_STATUS_INTERNAL_ERROR";
        case RSP_STATUS_MATRIX_TYPE_NOT_SUPPORTED: return "RSP_STATUS_MATRIX_TYPE_NOT_SUPPORTED";
        case RSP_STATUS_ZERO_PIVOT: return "RSP_STATUS_ZERO_PIVOT";
        case RSP_STATUS_NOT_SUPPORTED: return "RSP_STATUS_NOT_SUPPORTED";
    }
    return "RSP_STATUS_UNKNOWN";
}

rsp_status_t rsp_create(rsp_handle_t *handle) {
    if (!handle) return RSP_STATUS_INVALID_VALUE;
    *handle = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return RSP_STATUS_NOT_INITIALIZED;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return RSP_STATUS_NOT_INITIALIZED;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RSP_STATUS_ARCH_MISMATCH;
    rsp_context *c = new (std::nothrow) rsp_context;
    if (!c) return RSP_STATUS_ALLOC_FAILED;
    c->device = dev;
    c->stream = nullptr;
    c->ftz = 0;
    const char *v = getenv("RSP_SPMV_VARIANT");
    c->spmv_variant = v ? atoi(v) : 0;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // every kernel code object loaded now, as cusparseCreate sets itself up
    // outside the reference's timed calls (a lazily loaded one cost the
    // first timed SpMV of a --ref-sequence run 1.2-1.5 ms, measured)
    rsp_k::warm_spmv();
    rsp_k_ftz::warm_spmv();
    rsp_k::warm_ilu();
    rsp_k_ftz::warm_ilu();
    rsp_k::warm_analysis();
    rsp_k::warm_krylov();
    rsp_k_ftz::warm_krylov();
    c->d_ftrace = nullptr;
    c->d_strace = nullptr;
    c->d_dot = nullptr;
    c->h_dot = nullptr;
    c->d_gm = nullptr;
    c->h_gm = nullptr;
    *handle = c;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_destroy(rsp_handle_t h) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (h->d_ftrace || h->d_strace || h->d_dot || h->h_dot || h->d_gm || h->h_gm) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(h->device);
        if (h->d_ftrace) (void)hipFree(h->d_ftrace);
        if (h->d_strace) (void)hipFree(h->d_strace);
        if (h->d_dot) (void)hipFree(h->d_dot);
        if (h->h_dot) (void)hipHostFree(h->h_dot);
        if (h->d_gm) (void)hipFree(h->d_gm);
        if (h->h_gm) (void)hipHostFree(h->h_gm);
        (void)hipSetDevice(cur);
    }
    delete h;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_set_stream(rsp_handle_t h, void *stream) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    h->stream = (hipStream_t)stream;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_get_stream(rsp_handle_t h, void **stream) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!stream) return RSP_STATUS_INVALID_VALUE;
    *stream = (void *)h->stream;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_set_ftz(rsp_handle_t h, int enable) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    h->ftz = enable ? 1 : 0;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_get_ftz(rsp_handle_t h, int *enable) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!enable) return RSP_STATUS_INVALID_VALUE;
    *enable = h->ftz;
    return RSP_STATUS_SUCCESS;
}

/* ------------------------------------------------------------------ CSR */

rsp_status_t rsp_create_csr(rsp_spmat_t *mat, int64_t rows, int64_t cols, int64_t nnz,
                            void *d_row_offsets, void *d_col_ind, void *d_values,
                            rsp_datatype_t value_type) {
    if (!mat) return RSP_STATUS_INVALID_VALUE;
    *mat = nullptr;
    if (rows < 0 || cols < 0 || nnz < 0 || rows > INT_MAX - 1 || cols > INT_MAX || nnz > INT_MAX)
        return RSP_STATUS_INVALID_VALUE;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (!d_row_offsets && rows > 0) return RSP_STATUS_INVALID_VALUE;
    if ((!d_col_ind || !d_values) && nnz > 0) return RSP_STATUS_INVALID_VALUE;
    rsp_spmat *a = new (std::nothrow) rsp_spmat;
    if (!a) return RSP_STATUS_ALLOC_FAILED;
    memset(a, 0, sizeof(*a));
    a->rows = rows;
    a->cols = cols;
    a->nnz = nnz;
    a->rowptr = (int *)d_row_offsets;
    a->colidx = (int *)d_col_ind;
    a->vals = d_values;
    a->type = value_type;
    a->planned = 0;
    a->d_plan = nullptr;
    a->local_cols = -1;
    *mat = a;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_spmat_set_local_cols(rsp_spmat_t mat, int64_t ncols_local) {
    if (!mat || ncols_local < 0 || ncols_local > mat->cols) return RSP_STATUS_INVALID_VALUE;
    mat->local_cols = ncols_local;
    mat->planned = 0;  // re-plan on the next call
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_csr_set_values(rsp_spmat_t mat, void *d_values, rsp_datatype_t value_type) {
    if (!mat) return RSP_STATUS_INVALID_VALUE;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (d_values != mat->vals) mat->plan_gen = plan_new_gen();  // batches hold the old pointer
    mat->vals = d_values;
    if (value_type != mat->type) mat->planned = 0;  // tile size depends on type
    mat->type = value_type;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_destroy_spmat(rsp_spmat_t mat) {
    if (!mat) return RSP_STATUS_INVALID_VALUE;
    if (mat->d_plan) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(mat->plan_device);
        (void)hipFree(mat->d_plan);
        (void)hipSetDevice(cur);
    }
    delete mat->tside;  // (on the device it was built on)
    delete mat;
    return RSP_STATUS_SUCCESS;
}

/* ----------------------------------------------------------------- SpMV */

rsp_status_t rsp_spmv_buffer_size(rsp_handle_t h, rsp_operation_t op, const void *alpha,
                                  rsp_spmat_t mat, const void *beta, rsp_datatype_t compute_type,
                                  size_t *buffer_size) {
    (void)alpha;
    (void)beta;
    return guarded([&] {
        if (!h) return RSP_STATUS_NOT_INITIALIZED;
        if (!mat || !buffer_size) return RSP_STATUS_INVALID_VALUE;
        if (op == RSP_OPERATION_TRANSPOSE) {  // the transposed side, built if absent; no workspace either
            if (compute_type != mat->type) return RSP_STATUS_INVALID_VALUE;
            RSP_TRY(tside_ready(h, mat));
            rsp_spmat *c = &mat->tside->child;
            if (!c->planned || c->plan_type != compute_type) RSP_TRY(spmv_plan(h, c, compute_type));
            *buffer_size = 0;
            return RSP_STATUS_SUCCESS;
        }
        if (op != RSP_OPERATION_NON_TRANSPOSE) return RSP_STATUS_NOT_SUPPORTED;
        if (compute_type != mat->type) return RSP_STATUS_INVALID_VALUE;
        // the schedule is built here, into the matrix's own device memory (the
        // reference calls bufferSize once, before its timed loop); the caller's
        // workspace is not needed
        if (!mat->planned || mat->plan_type != compute_type) RSP_TRY(spmv_plan(h, mat, compute_type));
        *buffer_size = 0;
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_spmv_preprocess(rsp_handle_t h, rsp_operation_t op, const void *alpha,
                                 rsp_spmat_t mat, const void *d_x, const void *beta, void *d_y,
                                 rsp_datatype_t compute_type, void *d_buffer) {
    (void)alpha;
    (void)beta;
    (void)d_x;
    (void)d_y;
    (void)d_buffer;
    return guarded([&] {
        if (!h) return RSP_STATUS_NOT_INITIALIZED;
        if (!mat) return RSP_STATUS_INVALID_VALUE;
        if (op != RSP_OPERATION_NON_TRANSPOSE && op != RSP_OPERATION_TRANSPOSE) return RSP_STATUS_NOT_SUPPORTED;
        if (compute_type != mat->type) return RSP_STATUS_INVALID_VALUE;
        // explicit request: always re-plan (op = TRANSPOSE: the transposed side alone, from the pattern as it is now)
        return op == RSP_OPERATION_TRANSPOSE ? tside_build(h, mat) : spmv_plan(h, mat, compute_type);
    });
}

rsp_status_t rsp_spmv_plan_info(rsp_spmat_t mat, int64_t *tiles, int64_t *entries_16bit) {
    if (!mat || !tiles || !entries_16bit) return RSP_STATUS_INVALID_VALUE;
    if (!mat->planned) return RSP_STATUS_NOT_INITIALIZED;
    *tiles = mat->nblocks;
    *entries_16bit = mat->nnz_c16;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_spmv(rsp_handle_t h, rsp_operation_t op, const void *alpha, rsp_spmat_t mat,
                      const void *d_x, const void *beta, void *d_y, rsp_datatype_t compute_type,
                      void *d_buffer) {
    return guarded([&] { return spmv_run(h, op, alpha, mat, d_x, beta, d_y, compute_type, d_buffer, 0); });
}

rsp_status_t rsp_spmv_part(rsp_handle_t h, const void *alpha, rsp_spmat_t mat, const void *d_x,
                           const void *beta, void *d_y, rsp_datatype_t compute_type,
                           void *d_buffer, int part) {
    return guarded([&] {
        if (part < 0 || part > 2) return RSP_STATUS_INVALID_VALUE;
        return spmv_run(h, RSP_OPERATION_NON_TRANSPOSE, alpha, mat, d_x, beta, d_y, compute_type,
                        d_buffer, part);
    });
}

/* ------------------------------------------------------- batched SpMV */

rsp_status_t rsp_spmv_batch_create(rsp_handle_t h, int count, const rsp_spmat_t *mats,
                                   const void *const *d_x, void *const *d_y,
                                   void *const *d_buffers, rsp_datatype_t compute_type,
                                   int part, rsp_spmv_batch_t *batch) {
    return guarded([&] { return spmv_batch_create(h, count, mats, d_x, d_y, d_buffers, compute_type, part, batch); });
}

rsp_status_t rsp_spmv_batch_run(rsp_handle_t h, rsp_spmv_batch_t b, const void *alpha,
                                const void *beta) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!b || !alpha || !beta) return RSP_STATUS_INVALID_VALUE;
    for (size_t j = 0; j < b->mats.size(); j++) {  // re-planned since create: stale copy
        const rsp_spmat_t A = b->mats[j];
        if (!A->planned || A->plan_gen != b->plan_gen[j]) return RSP_STATUS_INVALID_VALUE;
    }
    const double av = b->type == RSP_R_64F ? *(const double *)alpha : *(const float *)alpha;
    const double bv = b->type == RSP_R_64F ? *(const double *)beta : *(const float *)beta;
    if (b->part != 0 && bv != 0.0) return RSP_STATUS_INVALID_VALUE;
    for (rsp::SpmvBatchArgs a : b->launches) {
        a.alpha = av;
        a.beta = bv;
        a.variant = h->spmv_variant;
        hipError_t e;
        if (b->type == RSP_R_64F)
            e = rsp_k::spmv_batch_f64(a, h->stream);
        else
            e = h->ftz ? rsp_k_ftz::spmv_batch_f32(a, h->stream) : rsp_k::spmv_batch_f32(a, h->stream);
        if (e != hipSuccess) return RSP_STATUS_EXECUTION_FAILED;
    }
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_spmv_batch_info(rsp_spmv_batch_t b, int64_t *tiles, int64_t *entries_16bit) {
    if (!b || !tiles || !entries_16bit) return RSP_STATUS_INVALID_VALUE;
    *tiles = b->tiles;
    *entries_16bit = b->entries_16bit;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_spmv_batch_destroy(rsp_spmv_batch_t b) {
    if (!b) return RSP_STATUS_INVALID_VALUE;
    delete b;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_gather(rsp_handle_t h, rsp_datatype_t value_type, int64_t n, const int64_t *d_idx,
                        const void *d_src, void *d_dst) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (n < 0 || (n > 0 && (!d_idx || !d_src || !d_dst))) return RSP_STATUS_INVALID_VALUE;
    hipError_t e = rsp_k::gather(value_type == RSP_R_64F ? 8 : 4, n, d_idx, d_src, d_dst, h->stream);
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

rsp_status_t rsp_scatter(rsp_handle_t h, rsp_datatype_t value_type, int64_t n, const int64_t *d_idx,
                         const void *d_src, void *d_dst) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    if (n < 0 || (n > 0 && (!d_idx || !d_src || !d_dst))) return RSP_STATUS_INVALID_VALUE;
    hipError_t e = rsp_k::scatter(value_type == RSP_R_64F ? 8 : 4, n, d_idx, d_src, d_dst, h->stream);
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

rsp_status_t rsp_spmv_transpose_permute(rsp_handle_t h, rsp_spmat_t mat) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!mat) return RSP_STATUS_INVALID_VALUE;
    const rsp_spmat_tside *t = mat->tside;
    if (!t || t->child.type != mat->type) return RSP_STATUS_NOT_INITIALIZED;
    if (t->child.nnz > 0 && !mat->vals) return RSP_STATUS_INVALID_VALUE;
    const hipError_t e = rsp_k::permute_values((int)elem_size(mat->type), t->child.nnz, t->perm, mat->vals, t->vt.p,
                                               h->num_cus, h->stream);
    return e == hipSuccess ? RSP_STATUS_SUCCESS : RSP_STATUS_EXECUTION_FAILED;
}

rsp_status_t rsp_csr2csc(rsp_handle_t h, int64_t rows, int64_t cols, int64_t nnz, const int *d_row_offsets,
                         const int *d_col_ind, const void *d_values, rsp_datatype_t value_type,
                         int *d_csc_col_offsets, int *d_csc_row_ind, void *d_csc_values) {
    return guarded([&] {
        if (!h) return RSP_STATUS_NOT_INITIALIZED;
        if (rows < 0 || cols < 0 || nnz < 0 || rows > INT_MAX - 1 || cols > INT_MAX - 1 || nnz > INT_MAX)
            return RSP_STATUS_INVALID_VALUE;
        if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
        if ((!d_row_offsets && rows > 0) || !d_csc_col_offsets) return RSP_STATUS_INVALID_VALUE;
        const bool symbolic = !d_values && !d_csc_values;
        rsp_spmat a;  // (a view for transpose_pattern: the pattern alone)
        memset(&a, 0, sizeof(a));
        a.rows = rows;
        a.cols = cols;
        a.nnz = nnz;
        a.rowptr = const_cast<int *>(d_row_offsets);
        a.colidx = const_cast<int *>(d_col_ind);
        HostTranspose ht;
        RSP_TRY(transpose_pattern(h, &a, ht));
        if (ht.nnz > 0 && (!d_csc_row_ind || (!symbolic && (!d_values || !d_csc_values))))
            return RSP_STATUS_INVALID_VALUE;
        DevMem perm;
        RSP_CHECK_HIP(upload_ints(h, d_csc_col_offsets, ht.rowptr));
        RSP_CHECK_HIP(upload_ints(h, d_csc_row_ind, ht.colidx));
        if (!symbolic && ht.nnz > 0) {
            RSP_CHECK_HIP(hipMalloc(&perm.p, (size_t)ht.nnz * sizeof(int)));
            RSP_CHECK_HIP(upload_ints(h, perm.p, ht.perm));
            if (rsp_k::permute_values((int)elem_size(value_type), ht.nnz, (const int *)perm.p, d_values,
                                      d_csc_values, h->num_cus, h->stream) != hipSuccess)
                return RSP_STATUS_EXECUTION_FAILED;
        }
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));  // (ht and perm go on return)
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_spmv_plan_host(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                rsp_datatype_t compute_type, int64_t *tiles, int64_t *entries_16bit,
                                int64_t *entries_staged) {
    return guarded([&] {
        if (m < 0 || (m > 0 && (!row_offsets || !col_ind)) || !tiles || !entries_16bit || !entries_staged)
            return RSP_STATUS_INVALID_VALUE;
        if (compute_type != RSP_R_64F && compute_type != RSP_R_32F) return RSP_STATUS_NOT_SUPPORTED;
        const PlanOptions o = rsp_plan::plan_options(compute_type);
        TilePlan p;
        rsp_plan::make_tile_plan(row_offsets, col_ind, m, nnz, o, p);
        if (!rsp_plan::plan_verify(row_offsets, col_ind, m, o, p)) return RSP_STATUS_INTERNAL_ERROR;
        *tiles = (int64_t)p.blocks.size();
        *entries_16bit = p.nnz_c16;
        *entries_staged = p.nnz_staged;
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_spmv_plan_tiles_host(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                      rsp_datatype_t compute_type, int64_t spread, int64_t local_cols, int row_align,
                                      int use_c16, int use_stage, int64_t *facts, int64_t max_tiles,
                                      int64_t counts[4]) {
    return guarded([&] {
        if (m < 0 || (m > 0 && (!row_offsets || !col_ind)) || !counts || max_tiles < 0 || (max_tiles > 0 && !facts) ||
            row_align < 1)
            return RSP_STATUS_INVALID_VALUE;
        if (compute_type != RSP_R_64F && compute_type != RSP_R_32F) return RSP_STATUS_NOT_SUPPORTED;
        PlanOptions o = rsp_plan::plan_options(compute_type);
        o.spread = spread;
        o.local_cols = local_cols;
        o.row_align = row_align;
        o.use_c16 = use_c16 != 0;
        o.use_stage = use_stage != 0;
        TilePlan p;
        rsp_plan::make_tile_plan(row_offsets, col_ind, m, nnz, o, p);
        if (!rsp_plan::plan_verify(row_offsets, col_ind, m, o, p)) return RSP_STATUS_INTERNAL_ERROR;
        const int64_t nt = (int64_t)p.blocks.size();
        for (int64_t t = 0; t < std::min(nt, max_tiles); t++)
            rsp_plan::tile_facts(p, (size_t)t, facts + t * RSP_SPMV_TILE_FACTS);
        counts[0] = nt;
        counts[1] = p.nint;
        counts[2] = (int64_t)p.longrows.size();
        counts[3] = p.nslots;
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_spmv_plan_stats(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                 rsp_datatype_t compute_type, int64_t stats[8]) {
    return guarded([&] {
        if (m < 0 || (m > 0 && (!row_offsets || !col_ind)) || !stats) return RSP_STATUS_INVALID_VALUE;
        if (compute_type != RSP_R_64F && compute_type != RSP_R_32F) return RSP_STATUS_NOT_SUPPORTED;
        TilePlan p;
        rsp_plan::make_tile_plan(row_offsets, col_ind, m, nnz, rsp_plan::plan_options(compute_type), p);
        rsp_plan::plan_stats(p, compute_type, stats);
        return RSP_STATUS_SUCCESS;
    });
}

}  // the C ABI
