// api_ilu_analysis.cpp — the ILU(0) analysis of include/rsp.h: the info
// object's lifecycle, the device half of the symbolic factor
// (ilu_analysis.hip) overlapped with the host plans (ilu_analysis.cpp, ilu_plan_*.cpp), their
// upload, the L / L^T solve plans built on a worker thread and the U plan,
// and the plan queries. Mirrors the analysis calls of the reference driver
// (GPU/ilu0.cu:82-252); the factor and the solves: api_ilu_solve.cpp.

#include "rsp_internal.h"

#include <atomic>
#include <chrono>
#include <functional>

using namespace rsp_api;

using Dag = rsp_ilu0_info::Dag;

// Sub-phase wall times on stderr, for RSP_ILU_TIMING >= 3 (diagnostics).
struct Stopwatch {
    const char *fmt;  // (n, what, ms)
    int n;
    bool on = env_int("RSP_ILU_TIMING", 0) >= 3;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, fmt, n, what, std::chrono::duration<double, std::milli>(t - last).count());
        last = t;
    }
};

// Device helper of the ILU analysis upload. Many arrays in ONE device
// allocation: add() records each array (host data to copy, or space only),
// commit() makes one hipMalloc and one copy per array. (One allocation per
// array — ~40 per analysis — had cost more than the copies themselves.)
// The arena keeps the ADDRESS of every destination pointer until commit()
// writes it: a destination (a member of the info's rsp_ilu0_info, built in place,
// or a local) must not move or die between its add and the commit.
struct Arena {
    struct Item {
        void **dst;
        const void *src;
        size_t bytes, copy, off;
    };
    rsp_an::hvec<Item> items;
    size_t total = 0;
    void add(void **dst, const void *src, size_t bytes, size_t copy) {
        items.push_back({dst, src, bytes, copy, total});
        total += (bytes + 255) & ~(size_t)255;
    }
    template <typename V>
    void up(const V **dst, const rsp_an::hvec<V> &v) {  // (a kernel-argument struct's read-only array)
        add((void **)dst, v.empty() ? nullptr : v.data(), std::max<size_t>(v.size(), 1) * sizeof(V),
            v.size() * sizeof(V));
    }
    template <typename V>
    void up(V **dst, const rsp_an::hvec<V> &v) {
        up((const V **)dst, v);
    }
    template <typename T>  // (T: any element type, const or not, or void)
    void space(T **dst, size_t bytes) {
        add((void **)dst, nullptr, bytes, 0);
    }
    hipError_t commit(DevMem &base, hipStream_t s) {
        base = DevMem();
        if (total == 0) return hipSuccess;
        hipError_t e = hipMalloc(&base.p, total);
        if (e != hipSuccess) return e;
        for (const Item &it : items) {
            *it.dst = (char *)base.p + it.off;
            if (it.copy && e == hipSuccess)
                e = hipMemcpyAsync(*it.dst, it.src, it.copy, hipMemcpyHostToDevice, s);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e;
    }
};

// What dag_upload and dag_upload_rows share: the DAG's host parts and the
// first arrays of its plan.
static void dag_upload_head(Arena &ar, Dag &d, const rsp_an::DagHost &h, int nterms) {
    d.ptr = h.ptr;
    d.batch = h.batch;
    d.group = h.group;
    d.segs = h.sp.segs;
    d.nshort = h.sp.nshort;
    d.nwave = h.sp.nwave;
    d.sbase = h.sp.sbase;
    d.nterms = nterms;
    if (!d.plan.rows) {  // (L's levels may be in the factor's arena already)
        ar.up(&d.plan.rows, h.rows);
        ar.up(&d.plan.ptr_dev, h.ptr);
    }
    ar.up(&d.plan.tasks, h.sp.tasks);
    ar.up(&d.plan.nshort, h.sp.nshort);
}

// Upload one DAG's solve plan (into the arena `ar`) and keep its host parts.
static void dag_upload(Arena &ar, Dag &d, const rsp_an::DagHost &h) {
    dag_upload_head(ar, d, h, (int)h.sp.tpos.size());
    ar.up(&d.plan.tpos, h.sp.tpos);
    ar.up(&d.plan.src, h.sp.src);
    ar.up(&d.plan.chunks, h.sp.chunks);
    ar.up(&d.plan.trow, h.sp.trow);
    ar.up(&d.plan.sid, h.sp.sid);
    ar.up(&d.plan.stg, h.sp.stg);
    ar.up(&d.plan.fitems, h.sp.fitems);
}

// Upload a block-inverse solve plan (into the arena) with its scratch.
static void blk_upload(Arena &ar, rsp_ilu0_info::BlkDag &d, const rsp_an::BlkPlanHost &h) {
    rsp::BlkArgs &b = d.args;
    d.on = true;
    d.segs = h.segs;
    b.n = h.n;
    b.nb = h.nb;
    b.lds_elems = h.lds_elems;
    b.lds_words = h.lds_words;
    ar.up(&b.order, h.order);
    ar.up(&b.desc, h.desc);
    ar.up(&b.rows, h.rows);
    ar.up(&b.ref, h.ref);
    ar.up(&b.vpos, h.vpos);
    ar.up(&b.eord, h.eord);
    ar.up(&b.lptr, h.lptr);
    ar.up(&b.rptr, h.rptr);
    ar.up(&b.rit, h.rit);
    ar.space(&b.ev, ((size_t)h.entries + 1) * sizeof(double));
    ar.space(&b.yp, ((size_t)h.n + 1) * sizeof(double));  // (+ a spare cell, trsv_blk_seg)
    ar.space(&b.rc, (size_t)h.nb * 64 * 144);
}

// Upload one DAG's per-row solve plan (L or L^T) into the arena and reserve
// the per-term arrays, which rsp_k::ilu_an_solve_terms then builds on the
// device (t: its arguments; pointers set at commit, the rest by the caller).
static void dag_upload_rows(Arena &ar, Dag &d, const rsp_an::DagHost &h, int n, rsp_k::SolveTermsArgs &t) {
    dag_upload_head(ar, d, h, std::max(h.sp.nterm, 1));
    const size_t nx = h.rows.size(), nch = h.sp.chunks.size();
    long long thin_terms = 0;
    for (const rsp::LevelChunk &ch : h.sp.chunks) thin_terms += ch.k1 - ch.k0;
    ar.space(&d.plan.tpos, (size_t)d.nterms * 4);
    ar.space(&d.plan.src, (size_t)d.nterms * 4);
    ar.space(&d.plan.sid, (size_t)d.nterms * 4);
    ar.up(&d.plan.chunks, h.sp.chunks);  // staged ranges written on the device
    ar.space(&d.plan.trow, std::max<size_t>(nx, 1) * sizeof(rsp::ThinRowPlan));
    ar.space(&d.plan.stg, (size_t)std::max(thin_terms, 1LL) * sizeof(rsp::StagedTerm));
    ar.up(&d.plan.fitems, h.sp.fitems);
    ar.up(&t.cbase, h.sp.cbase);
    ar.space(&t.slot_of, (size_t)std::max(n, 1) * 4);
    ar.space(&t.nst, (nch + 1) * 4);
    ar.space(&t.nst_ptr, (nch + 1) * 4);
    size_t tb = 0;
    (void)rsp_k::ilu_an_scan(nullptr, nullptr, (int)nch + 1, nullptr, &tb, nullptr);
    ar.space(&t.scan, std::max<size_t>(tb, 16));
    t.n = n;
    t.nx = (int)nx;
    t.total = h.sp.nterm;
    t.nch = (int)nch;
    t.group = h.group;
}

// After the commit: the per-term arrays of a DAG uploaded by dag_upload_rows
// (the one place that writes through the plan's read-only pointers).
static hipError_t dag_build_terms(const Dag &d, rsp_k::SolveTermsArgs &t, hipStream_t s) {
    const rsp::LevelPlan &p = d.plan;
    t.tasks = p.tasks;
    t.ptr = p.ptr_dev;
    t.chunks = const_cast<rsp::LevelChunk *>(p.chunks);
    t.tpos = const_cast<int *>(p.tpos);
    t.src = const_cast<int *>(p.src);
    t.sid = const_cast<int *>(p.sid);
    t.trow = const_cast<rsp::ThinRowPlan *>(p.trow);
    t.stg = const_cast<rsp::StagedTerm *>(p.stg);
    return rsp_k::ilu_an_solve_terms(t, s);
}

// Tests only (RSP_ILU_DIGEST): the device-built per-term arrays back into the
// host plan, so the digest covers them.
static hipError_t dag_download_terms(const Dag &d, const rsp_k::SolveTermsArgs &t, rsp_an::DagHost &h,
                                     hipStream_t s) {
    rsp_an::SolvePlan &sp = h.sp;
    int nstg = 0;
    hipError_t e = hipMemcpyAsync(&nstg, t.nst_ptr + t.nch, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    sp.tpos.resize((size_t)d.nterms);
    sp.src.resize((size_t)d.nterms);
    sp.sid.resize((size_t)d.nterms);
    sp.trow.resize(std::max<size_t>((size_t)t.nx, 1));
    sp.stg.resize((size_t)std::max(nstg, 1));
    e = hipMemcpyAsync(sp.tpos.data(), t.tpos, sp.tpos.size() * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sp.src.data(), t.src, sp.src.size() * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sp.sid.data(), t.sid, sp.sid.size() * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(sp.trow.data(), t.trow, sp.trow.size() * sizeof(rsp::ThinRowPlan), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(sp.stg.data(), t.stg, sp.stg.size() * sizeof(rsp::StagedTerm), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(sp.chunks.data(), t.chunks, sp.chunks.size() * sizeof(rsp::LevelChunk),
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// Budget of the fat factor slot layout (ints): RSP_ILU_SLOT_CAP_MB if set,
// else the smaller of 2 GB and 1/8 of the device memory free now.
static long long slot_cap_ints() {
    long long cap_mb = env_int("RSP_ILU_SLOT_CAP_MB", -1);
    if (cap_mb < 0) {
        size_t fr = 0, tot = 0;
        cap_mb = 2048;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) cap_mb = std::min<long long>(cap_mb, (long long)(fr >> 23));
    }
    return cap_mb * (1LL << 20) / 4;
}
// ... of the host entries (no device to ask): the knob if set, else 2 GB
static long long host_slot_cap_ints() {
    const long long cap_mb = env_int("RSP_ILU_SLOT_CAP_MB", -1);
    return (cap_mb >= 0 ? cap_mb : 2048) * (1LL << 20) / 4;
}

// The data-parallel analysis on the device (ilu_analysis.hip), overlapped
// with the host level sets: validation, diagonal positions and structural
// zero, then the symbolic factor (update lists, stages, stage order, divisor
// positions), which stays on the device for the factor kernels; the host gets
// back the pattern, dpos / hasdiag, the update lists and stages its plans
// read. Rows longer than kAnDevRow entries (circuit hubs: a long serial chain
// of lower positions, slow at one GPU lane's memory latency) are done on the
// host (rsp_an::symbolic_rows) and their ranges uploaded. Fills hp (levels
// included).
static constexpr int kAnDevRow = 1024;
// device rows longer than this get one wave each for their stages (the
// thread-per-row kernel takes the rest; RSP_AN_WAVE_ROW overrides, A/B)
static constexpr int kAnWaveRow = 128;
static rsp_status_t ilu_symbolic_device(rsp_handle_t h, rsp_ilu0_info *f, const int *d_rp, const int *d_ci,
                                        const rsp_an::hvec<int> &rp, rsp_an::hvec<int> &ci, rsp_an::IluHostPlan &hp,
                                        rsp_an::Phases &ph, const std::function<void()> &after_levels) {
    const int n = hp.n, nnz_s = hp.nnz_s;
    hipStream_t s = h->stream;
    Stopwatch sub{"rsp_ilu0_analysis n=%d     %-22s %8.2f ms\n", n};
    rsp_an::hvec<int> dev_rows, long_rows, wave_rows;
    const int wave_row = (int)env_int("RSP_AN_WAVE_ROW", kAnWaveRow);
    int cap0 = 1;  // the longest device row: the pair kernel's LDS per row
    for (int i = 0; i < n; i++) {
        const int len = rp[(size_t)i + 1] - rp[(size_t)i];
        if (len > kAnDevRow) {
            long_rows.push_back(i);
        } else {
            cap0 = std::max(cap0, len);
            if (len > wave_row) wave_rows.push_back(i);
        }
    }
    rsp_an::resize_uninit(dev_rows, (size_t)(n - (int)long_rows.size()));
    if (long_rows.empty()) {  // every row (FEM / stencil patterns): 0 .. n-1 in parallel
        rsp_an::parallel_for(n, 1 << 16, [&](long long a, long long b) {
            for (long long i = a; i < b; i++) dev_rows[(size_t)i] = (int)i;
        });
    } else {
        size_t w = 0;
        for (int i = 0; i < n; i++)
            if (rp[(size_t)i + 1] - rp[(size_t)i] <= kAnDevRow) dev_rows[w++] = i;
    }
    // The host level pass needs only the pattern: download it first, check it
    // (columns in range, rows strictly increasing: the device check below
    // returns the same verdict), take the diagonal positions from it and run
    // the level pass on a thread of its own while the device validates,
    // counts, scans and fills (round 4: the level pass used to wait for all
    // of that).
    if (nnz_s > 0) {
        RSP_CHECK_HIP(hipMemcpyAsync(ci.data(), d_ci, (size_t)nnz_s * 4, hipMemcpyDeviceToHost, s));
        RSP_CHECK_HIP(hipStreamSynchronize(s));
    }
    sub("D2H pattern");
    {
        // (and the diagonal flags and the structural zero: the device rows
        // kernel below computes the same arrays for the device, so nothing of
        // it is read back — round 5: two synchronisations fewer per analysis)
        std::atomic<int> bad{0}, szero{INT_MAX};
        rsp_an::resize_uninit(hp.dpos, (size_t)n);
        rsp_an::resize_uninit(hp.hasdiag, (size_t)n);
        rsp_an::parallel_for(n, 1 << 14, [&](long long r0, long long r1) {
            int sz = INT_MAX;
            for (long long i = r0; i < r1; i++) {
                const int a = rp[(size_t)i], b = rp[(size_t)i + 1];
                int d = b, prev = -1;
                for (int p = a; p < b; p++) {
                    const int c = ci[(size_t)p];
                    if (c < 0 || c >= n || c <= prev) bad.store(1, std::memory_order_relaxed);
                    if (d == b && c >= (int)i) d = p;
                    prev = c;
                }
                hp.dpos[(size_t)i] = d;
                const int hd = d < b && ci[(size_t)d] == (int)i ? 1 : 0;
                hp.hasdiag[(size_t)i] = hd;
                if (!hd && sz == INT_MAX) sz = (int)i;
            }
            for (int cur = szero.load(); sz < cur && !szero.compare_exchange_weak(cur, sz);) {
            }
        });
        if (bad.load()) return RSP_STATUS_INVALID_VALUE;  // a column out of range or a row not increasing
        hp.structural_zero = szero.load() == INT_MAX ? -1 : szero.load();
    }
    sub("host check + dpos");
    // (the L levels: the factor's; L^T's are the solve plans' thread's first step)
    rsp_an::Task levels([&] { rsp_an::plan_levels_lower(rp.data(), ci.data(), hp); });
    size_t scan_bytes = 0;
    RSP_CHECK_HIP(rsp_k::ilu_an_scan(nullptr, nullptr, nnz_s + 1, nullptr, &scan_bytes, s));
    Arena ar;
    int *d_flags = nullptr, *d_cnt = nullptr, *d_stage = nullptr, *d_scratch = nullptr, *d_rows = nullptr;
    // the symbolic arrays the kernels below write and the factor reads (f->fac)
    int *d_dpos = nullptr, *d_hasdiag = nullptr, *d_upd_ptr = nullptr, *d_upd_l = nullptr, *d_upd_u = nullptr;
    int *d_lord = nullptr, *d_lend = nullptr, *d_udiv = nullptr;
    void *d_scan = nullptr;
    ar.space(&d_dpos, (size_t)std::max(n, 1) * 4);
    ar.space(&d_hasdiag, (size_t)std::max(n, 1) * 4);
    ar.space(&d_flags, 2 * 4);
    ar.space(&d_cnt, ((size_t)nnz_s + 1) * 4);
    ar.space(&d_upd_ptr, ((size_t)nnz_s + 1) * 4);
    ar.space(&d_stage, (size_t)std::max(nnz_s, 1) * 4);
    ar.space(&d_lord, (size_t)std::max(nnz_s, 1) * 4);
    ar.space(&d_lend, (size_t)std::max(nnz_s, 1) * 4);
    ar.space(&d_udiv, (size_t)std::max(nnz_s, 1) * 4);
    ar.space(&d_scratch, (size_t)std::max(nnz_s, 1) * 4);
    ar.space(&d_scan, std::max<size_t>(scan_bytes, 16));
    ar.up(&d_rows, dev_rows);
    int *d_wrows = nullptr;
    ar.up(&d_wrows, wave_rows);
    sub("arena");
    RSP_CHECK_HIP(ar.commit(f->arena_sym, s));
    rsp::IluArgs &fa = f->fac;
    fa.dpos = d_dpos, fa.hasdiag = d_hasdiag, fa.upd_ptr = d_upd_ptr;
    fa.lord = d_lord, fa.lend = d_lend, fa.udiv = d_udiv;
    // the device's diagonal positions and flags (its validation flags are not
    // read: the host check above gave the same verdict)
    RSP_CHECK_HIP(rsp_k::ilu_an_rows(n, d_rp, d_ci, d_dpos, d_hasdiag, d_flags, s));
    const int n_c[3] = {(int)dev_rows.size(), 0, 0};
    const int *rows_c[3] = {d_rows, nullptr, nullptr};
    RSP_CHECK_HIP(rsp_k::ilu_an_count(rows_c, n_c, cap0, d_rp, d_ci, d_dpos, d_hasdiag, d_cnt, d_scratch, s));
    sub("rows + count kernels");
    // the long rows' counts on the host
    rsp_an::hvec<int> hcnt(long_rows.empty() ? 0 : (size_t)nnz_s);
    rsp_an::symbolic_rows(long_rows, n, rp.data(), ci.data(), hp.dpos.data(), hp.hasdiag.data(), hcnt.data(),
                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    for (int i : long_rows)
        RSP_CHECK_HIP(hipMemcpyAsync(d_cnt + rp[(size_t)i], hcnt.data() + rp[(size_t)i],
                                     (size_t)(rp[(size_t)i + 1] - rp[(size_t)i]) * 4, hipMemcpyHostToDevice, s));
    sub("long-row counts");
    RSP_CHECK_HIP(hipMemsetAsync(d_cnt + nnz_s, 0, 4, s));
    RSP_CHECK_HIP(rsp_k::ilu_an_scan(d_cnt, d_upd_ptr, nnz_s + 1, d_scan, &scan_bytes, s));
    rsp_an::resize_uninit(hp.sym.upd_ptr, (size_t)nnz_s + 1);
    RSP_CHECK_HIP(hipMemcpyAsync(hp.sym.upd_ptr.data(), d_upd_ptr, ((size_t)nnz_s + 1) * 4,
                                 hipMemcpyDeviceToHost, s));
    RSP_CHECK_HIP(hipStreamSynchronize(s));
    sub("scan + D2H upd_ptr");
    ph.mark("device rows");
    // a pair count past int would overflow the plans' indices
    const int total = hp.sym.upd_ptr[(size_t)nnz_s];
    if (total < 0) return RSP_STATUS_ALLOC_FAILED;
    Arena ap;
    ap.space(&d_upd_l, (size_t)std::max(total, 1) * 4);
    ap.space(&d_upd_u, (size_t)std::max(total, 1) * 4);
    RSP_CHECK_HIP(ap.commit(f->arena_pairs, s));
    fa.upd_l = d_upd_l, fa.upd_u = d_upd_u;
    sub("pairs arena");
    RSP_CHECK_HIP(rsp_k::ilu_an_fill(rows_c, n_c, cap0, d_rp, d_ci, d_dpos, d_hasdiag, d_upd_ptr, d_scratch,
                                     d_upd_l, d_upd_u, s));
    RSP_CHECK_HIP(rsp_k::ilu_an_stages(n, std::min(wave_row, kAnDevRow), d_rp, d_ci, d_dpos, d_hasdiag, d_upd_ptr, d_upd_l,
                                       d_stage, d_lord, d_lend, d_udiv, d_scratch, d_wrows,
                                       (int)wave_rows.size(), s));
    // the level sets (host thread, started above) while the device fills the update lists
    levels.join();
    ph.mark("levels");
    after_levels();  // the solve plans need nothing more: started here
    // the host factor plan reads the update pairs of its thin rows only: those
    // are packed on the device and downloaded (FEM matrices have tens of
    // millions of pairs, nearly all in fat levels). Not with host-built hub
    // rows (their lists are uploaded from full host arrays) or for the tests'
    // plan digest (which covers the full arrays).
    const bool pack = long_rows.empty() && !env_int("RSP_ILU_DIGEST", 0) && env_int("RSP_ILU_PACK_PAIRS", 1);
    bool want_stage = true;  // the factor plan reads the stages of its thin rows only
    if (pack) {
        const rsp_an::hvec<int> trows = rsp_an::factor_thin_rows(rp.data(), hp);
        want_stage = !trows.empty();
        rsp_an::hvec<int> cbase(trows.size() + 1, 0);
        for (size_t r = 0; r < trows.size(); r++) {
            const int i = trows[r];
            cbase[r + 1] = cbase[r] + hp.sym.upd_ptr[(size_t)rp[(size_t)i + 1]] - hp.sym.upd_ptr[(size_t)rp[(size_t)i]];
        }
        const int packed = cbase.back();
        hp.sym.pair_base.assign((size_t)std::max(n, 1), 0);
        for (size_t r = 0; r < trows.size(); r++) hp.sym.pair_base[(size_t)trows[r]] = cbase[r];
        rsp_an::resize_uninit(hp.sym.upd_l, (size_t)packed);
        rsp_an::resize_uninit(hp.sym.upd_u, (size_t)packed);
        if (packed > 0) {
            Arena ag;
            int *d_trows = nullptr, *d_cbase = nullptr, *d_pl = nullptr, *d_pu = nullptr;
            DevMem gather;
            ag.up(&d_trows, trows);
            ag.up(&d_cbase, cbase);
            ag.space(&d_pl, (size_t)packed * 4);
            ag.space(&d_pu, (size_t)packed * 4);
            RSP_CHECK_HIP(ag.commit(gather, s));
            hipError_t e = rsp_k::ilu_an_gather_pairs(d_trows, (int)trows.size(), d_rp, d_upd_ptr, d_cbase,
                                                      d_upd_l, d_upd_u, d_pl, d_pu, s);
            if (e == hipSuccess) e = hipMemcpyAsync(hp.sym.upd_l.data(), d_pl, (size_t)packed * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(hp.sym.upd_u.data(), d_pu, (size_t)packed * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            RSP_CHECK_HIP(e);
        }
    } else {
        rsp_an::resize_uninit(hp.sym.upd_l, (size_t)total);
        rsp_an::resize_uninit(hp.sym.upd_u, (size_t)total);
        if (total > 0) {
            RSP_CHECK_HIP(hipMemcpyAsync(hp.sym.upd_l.data(), d_upd_l, (size_t)total * 4, hipMemcpyDeviceToHost, s));
            RSP_CHECK_HIP(hipMemcpyAsync(hp.sym.upd_u.data(), d_upd_u, (size_t)total * 4, hipMemcpyDeviceToHost, s));
        }
    }
    rsp_an::resize_uninit(hp.sym.stage, want_stage ? (size_t)nnz_s : 0);
    if (nnz_s > 0 && want_stage)
        RSP_CHECK_HIP(hipMemcpyAsync(hp.sym.stage.data(), d_stage, (size_t)nnz_s * 4, hipMemcpyDeviceToHost, s));
    RSP_CHECK_HIP(hipStreamSynchronize(s));
    sub("D2H pairs + stages");
    if (!long_rows.empty()) {  // the long rows' lists, stages, stage order, divisors on the host
        rsp_an::hvec<int> lord((size_t)nnz_s), lend((size_t)nnz_s), udiv((size_t)nnz_s);
        rsp_an::symbolic_rows(long_rows, n, rp.data(), ci.data(), hp.dpos.data(), hp.hasdiag.data(), nullptr,
                              hp.sym.upd_ptr.data(), hp.sym.upd_l.data(), hp.sym.upd_u.data(), hp.sym.stage.data(),
                              lord.data(), lend.data(), udiv.data());
        for (int i : long_rows) {
            const size_t rs = (size_t)rp[(size_t)i], len = (size_t)(rp[(size_t)i + 1] - rp[(size_t)i]);
            const size_t q0 = (size_t)hp.sym.upd_ptr[rs], nq = (size_t)hp.sym.upd_ptr[rs + len] - q0;
            if (nq > 0) {
                RSP_CHECK_HIP(hipMemcpyAsync(d_upd_l + q0, hp.sym.upd_l.data() + q0, nq * 4, hipMemcpyHostToDevice, s));
                RSP_CHECK_HIP(hipMemcpyAsync(d_upd_u + q0, hp.sym.upd_u.data() + q0, nq * 4, hipMemcpyHostToDevice, s));
            }
            RSP_CHECK_HIP(hipMemcpyAsync(d_lord + rs, lord.data() + rs, len * 4, hipMemcpyHostToDevice, s));
            RSP_CHECK_HIP(hipMemcpyAsync(d_lend + rs, lend.data() + rs, len * 4, hipMemcpyHostToDevice, s));
            RSP_CHECK_HIP(hipMemcpyAsync(d_udiv + rs, udiv.data() + rs, len * 4, hipMemcpyHostToDevice, s));
        }
        RSP_CHECK_HIP(hipStreamSynchronize(s));
    }
    sub("long rows");
    ph.mark("device symbolic");
    return RSP_STATUS_SUCCESS;
}

static rsp_status_t ilu0_analysis(rsp_handle_t h, int n, int nnz, const int *d_row_offsets,
                                  const int *d_col_ind, rsp_ilu0_info *f) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    // diagnostics: RSP_ILU_TIMING=1 prints the wall time of each analysis phase
    rsp_an::Phases ph;
    ph.print = env_int("RSP_ILU_TIMING", 0) != 0;
    ph.n = n;
    ph.start();
    if (!f || n < 0 || nnz < 0 || (n > 0 && !d_row_offsets)) return RSP_STATUS_INVALID_VALUE;
    Stopwatch pre{"rsp_ilu0_analysis n=%d     %-22s %8.2f ms\n", n};  // diagnostics: preamble sub-phases
    f->reset();  // the previous analysis goes: its planning thread, device arrays, counters, call records
    pre("free");
    // the pattern to the host (row offsets first: the stored entries must lie
    // inside the declared arrays before colidx is read)
    rsp_an::hvec<int> rp((size_t)n + 1, 0);
    if (n > 0) {
        RSP_CHECK_HIP(hipMemcpyAsync(rp.data(), d_row_offsets, ((size_t)n + 1) * sizeof(int),
                                     hipMemcpyDeviceToHost, h->stream));
        RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    }
    if (rp[0] != 0) return RSP_STATUS_INVALID_VALUE;
    for (int i = 0; i < n; i++)
        if (rp[(size_t)i + 1] < rp[(size_t)i]) return RSP_STATUS_INVALID_VALUE;
    const int nnz_s = rp[(size_t)n];
    if (nnz_s > 0 && !d_col_ind) return RSP_STATUS_INVALID_VALUE;
    if (nnz_s > nnz) return RSP_STATUS_INVALID_VALUE;  // entries past the declared arrays
    pre("D2H rowptr + checks");
    rsp_an::hvec<int> ci;
    rsp_an::resize_uninit(ci, (size_t)nnz_s);  // (downloaded whole below)
    std::unique_ptr<rsp_an::IluHostPlan> hp(new (std::nothrow) rsp_an::IluHostPlan());
    if (!hp) return RSP_STATUS_ALLOC_FAILED;
    hp->n = n;
    hp->nnz_s = nnz_s;
    // the solve plans are built on a second thread from the moment the levels
    // exist, under the symbolic factor's transfers and the factor plan
    // their per-term half is built on the device after the upload
    // (RSP_ILU_HOST_TERMS=1: on the host, as rsp_ilu0_analysis_host does; A/B)
    const bool dev_terms = n > 0 && !env_int("RSP_ILU_HOST_TERMS", 0);
    // (declared after rp, ci, hp: destroyed - joined - before them if the
    // factor plan throws)
    // the solve plans' thread outlives this call (rsp_ilu0_info::solves_task):
    // it holds the buffers, which move into the info below, not the locals
    std::unique_ptr<rsp_an::Task> solves;
    const int *rpd = rp.data(), *cid = ci.data();
    rsp_an::IluHostPlan *H = hp.get();
    rsp_status_t st = ilu_symbolic_device(h, f, d_row_offsets, d_col_ind, rp, ci, *hp, ph, [&] {
        solves.reset(new rsp_an::Task([rpd, cid, H, n, dev_terms] {
            rsp_an::plan_levels_upper(rpd, cid, *H);  // L^T levels, the transposed lower part
            // block-inverse plans of the deep DAGs, beside the row plans
            auto blk = [&](int kind) {
                const rsp_an::DagHost &dg = kind == 0 ? H->L : H->LT;
                if (!rsp_an::blocks_wanted(n, (int)dg.ptr.size() - 1)) return;
                bool &has = kind == 0 ? H->has_lb : H->has_ltb;
                has = rsp_an::plan_blocks(kind, rpd, cid, *H, kind == 0 ? H->Lb : H->LTb);
            };
            rsp_an::Task bl([&] { blk(0); }), bt([&] { blk(1); });
            if (dev_terms)
                rsp_an::plan_solves_rows(rpd, cid, *H);
            else
                rsp_an::plan_solves(rpd, cid, *H);
            bl.join();
            bt.join();
        }));
    });
    if (st == RSP_STATUS_SUCCESS) rsp_an::plan_factor(rp.data(), ci.data(), slot_cap_ints(), *hp);
    if (st != RSP_STATUS_SUCCESS) {
        solves.reset();  // (joined before the buffers it reads go)
        f->reset();
        return st;
    }
    // the U DAG (--true-lu extension) is planned on its first use
    ph.mark("plans");
    f->structural_zero = hp->structural_zero;
    f->n_updates = nnz_s > 0 ? (long long)hp->sym.upd_ptr[(size_t)nnz_s] : 0;
    f->fac_batch = hp->fac_batch;
    f->fac_segs = hp->fplan.segs;
    f->fslev = hp->fslev;
    if (env_int("RSP_ILU_DIGEST", 0)) {  // tests only: the device-only symbolic arrays too
        hp->sym.lord.resize((size_t)nnz_s);
        hp->sym.lend.resize((size_t)nnz_s);
        hp->udiv.resize((size_t)nnz_s);
        hipError_t e = hipSuccess;
        if (nnz_s > 0) {
            e = hipMemcpyAsync(hp->sym.lord.data(), f->fac.lord, (size_t)nnz_s * 4, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(hp->sym.lend.data(), f->fac.lend, (size_t)nnz_s * 4, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(hp->udiv.data(), f->fac.udiv, (size_t)nnz_s * 4, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
        f->digest = e == hipSuccess ? 1 : 0;  // computed once the solve terms exist (below)
    }
    Stopwatch up_step{"rsp_ilu0_analysis n=%d     upload: %-16s %8.2f ms\n", n};  // diagnostics: the upload's steps
    // everything in one device allocation; the factor's arguments (f->fac) get
    // the pattern and the factor plan here, beside ilu_symbolic_device's arrays
    rsp::IluArgs &fa = f->fac;
    fa.n = n;
    fa.rowptr = d_row_offsets;
    fa.colidx = d_col_ind;
    Arena ar;
    ar.up(&fa.rchunks, hp->fplan.chunks);
    ar.up(&fa.ritems, hp->fplan.items);
    ar.up(&fa.rpairs, hp->fplan.pairs);
    ar.up(&fa.rstaged, hp->fplan.staged);
    ar.up(&fa.rrounds, hp->fplan.rounds);
    ar.up(&fa.frow, hp->frow);
    ar.up(&fa.fitems, hp->ffitems);
    f->fruns = hp->fruns;
    f->fac_one = hp->fac_one;    // the factor walks its own one level (rsp_an::IluHostPlan::F), else L's
    fa.fac_one = hp->fac_scale;  // (IluArgs' name for another thing:) the whole factor is ilu0_scale_lower
    // (the solve plans add the rest of L at ilu_solves_ready)
    Dag &fd = hp->fac_one ? f->F : f->L;
    const rsp_an::DagHost &fh = hp->fac_one ? hp->F : hp->L;
    fd.ptr = fh.ptr;
    ar.up(&fd.plan.rows, fh.rows);
    ar.up(&fd.plan.ptr_dev, fh.ptr);
    // flow runs: the saved upper input values of their rows (ilu0_flow_prep)
    if (!hp->fruns.empty()) ar.space(&fa.forig, (size_t)std::max(hp->nnz_s, 1) * sizeof(double));
    ar.space(&f->d_zero, 8 * sizeof(int));  // zero pivot, flow give-ups, claim counter
    // flow items (factor rows; solve items hold >= 1 row each, U's included) <= n
    ar.space(&f->d_fdone, (size_t)std::max(n, 1) * sizeof(int));
    ar.space(&f->d_tk, 2 * rsp::kFlowTicketCtrs * sizeof(unsigned));
    int4 *d_desc = nullptr;
    long long *d_offs = nullptr;
    if (!hp->slot_desc.empty()) {
        ar.up(&d_desc, hp->slot_desc);
        ar.up(&d_offs, hp->slot_offs);
    }
    up_step("arena build");
    hipError_t e = ar.commit(f->arena, h->stream);
    up_step("commit (H2D)");
    fa.zero_pivot = f->d_zero;
    // on the handle's stream like everything else (the call is host-blocking:
    // the counters are in place when it returns, whatever stream comes next)
    if (e == hipSuccess) e = hipMemsetD32Async(f->d_zero, INT_MAX, 1, h->stream);
    if (e == hipSuccess) e = hipMemsetD32Async(f->d_zero + 1, 0, 7, h->stream);
    if (e == hipSuccess) e = hipMemsetD32Async(f->d_fdone, 0, (size_t)std::max(n, 1), h->stream);
    if (e == hipSuccess) e = hipMemsetD32Async(f->d_tk, 0, 2 * rsp::kFlowTicketCtrs, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    // fat factor slots, written on the device from the uploaded symbolic
    // arrays; the layout is an optimisation: without its memory, or if the
    // build fails, the FacRow path factors every fat level (same bits)
    if (e == hipSuccess && hp->slot_total > 0) {
        hipError_t es = hipMalloc(&f->fslots.p, (size_t)hp->slot_total * sizeof(int));
        if (es == hipSuccess) {
            rsp::IluArgs a = fa;  // (its plan is all zero: fac is value-initialised, the plan set per call)
            a.plan.rows = fd.plan.rows;
            es = rsp_k::ilu0_build_slots(a, d_desc, d_offs, (int)hp->slot_desc.size(), (int *)f->fslots.p,
                                         h->stream);
            if (es == hipSuccess) es = hipStreamSynchronize(h->stream);
        }
        up_step("factor slots");
        if (es == hipSuccess) {
            fa.fslots = (const int *)f->fslots.p;
        } else {
            (void)hipGetLastError();
            f->fslots = DevMem();
            f->fslev.assign(f->fslev.size(), rsp::FacSlotLevel{0, 0, 0, 0, 0});
            f->fruns.clear();  // the flow runs read the slots too
        }
    }
    ph.mark("upload");
    if (e != hipSuccess) {
        f->reset();
        return e == hipErrorOutOfMemory ? RSP_STATUS_ALLOC_FAILED : RSP_STATUS_EXECUTION_FAILED;
    }
    // (the buffers keep their addresses: the solve plans' thread reads them on)
    f->host_rp.swap(rp);
    f->host_ci.swap(ci);
    f->host = std::move(hp);
    f->solves_task = std::move(solves);
    f->dev_terms = dev_terms;
    f->han = h;
    f->n = n;
    f->nnz_s = nnz_s;
    f->analysed = 1;
    return RSP_STATUS_SUCCESS;
}

// The L and L^T solve plans (rsp_trsv_analysis, or the first solve): wait
// for their thread (started by rsp_ilu0_analysis) and upload them — the row
// plans, the block-inverse plans of deep DAGs, the solve streams — and build
// their per-term half on the device. Once per analysis.
rsp_status_t rsp_api::ilu_solves_ready(rsp_handle_t h, rsp_ilu0_info *f) {
    if (f->solves_ready) return RSP_STATUS_SUCCESS;
    if (!f->analysed || !f->host || !h) return RSP_STATUS_INVALID_VALUE;
    if (f->solves_task) {
        std::unique_ptr<rsp_an::Task> t = std::move(f->solves_task);
        try {
            t->join();
        } catch (...) {  // the plans are incomplete: the info needs a new analysis
            f->analysed = 0;
            throw;  // (guarded: an error status)
        }
    }
    rsp_an::IluHostPlan *hp = f->host.get();
    const int n = f->n;
    const bool dev_terms = f->dev_terms;
    Stopwatch up_step{"rsp_trsv_analysis n=%d     upload: %-16s %8.2f ms\n", n};  // diagnostics
    Arena ar;
    rsp_k::SolveTermsArgs tl{}, tt{};
    if (dev_terms) {
        dag_upload_rows(ar, f->L, hp->L, n, tl);
        dag_upload_rows(ar, f->LT, hp->LT, n, tt);
        tl.kind = 0;
        tl.rp = f->fac.rowptr;
        tl.ci = f->fac.colidx;
        // the split term order (rsp_an::split_terms); none (nullptr) for the
        // reference's order
        if (!hp->lpos.empty()) {
            ar.up(&tl.lpos, hp->lpos);
            ar.up(&tl.ne, hp->ne_l);
            ar.up(&tt.ne, hp->ne_lt);
        }
        tt.kind = 1;
        ar.up(&tt.ltp, hp->ltp);
        ar.up(&tt.lts, hp->lts);
        ar.up(&tt.ltc, hp->ltc);
    } else {
        dag_upload(ar, f->L, hp->L);
        dag_upload(ar, f->LT, hp->LT);
    }
    if (hp->has_lb) blk_upload(ar, f->Lb, hp->Lb);
    if (hp->has_ltb) blk_upload(ar, f->LTb, hp->LTb);
    // solve streams: values per flat term, alpha x and u_ii per level-order slot (fp64 size)
    const size_t nt = (size_t)std::max({f->L.nterms, f->LT.nterms, 1});
    ar.space(&f->d_sval, nt * sizeof(double));
    ar.space(&f->d_sx, (size_t)std::max(n, 1) * sizeof(double));
    ar.space(&f->d_sdg, (size_t)std::max(n, 1) * sizeof(double));
    up_step("arena build");
    hipError_t e = ar.commit(f->arena_s, h->stream);
    up_step("commit (H2D)");
    if (e == hipSuccess && dev_terms) {
        tl.dpos = f->fac.dpos;
        e = dag_build_terms(f->L, tl, h->stream);
        if (e == hipSuccess) e = dag_build_terms(f->LT, tt, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    up_step("solve terms");
    if (e == hipSuccess && env_int("RSP_ILU_DIGEST", 0)) {  // tests only
        if (dev_terms) {
            e = dag_download_terms(f->L, tl, hp->L, h->stream);
            if (e == hipSuccess) e = dag_download_terms(f->LT, tt, hp->LT, h->stream);
        }
        f->digest = e == hipSuccess && f->digest ? rsp_an::digest(*hp) : 0;
    }
    if (e != hipSuccess) {
        f->reset();  // (half-uploaded plans: analyse again)
        return e == hipErrorOutOfMemory ? RSP_STATUS_ALLOC_FAILED : RSP_STATUS_EXECUTION_FAILED;
    }
    // host copies kept for the U plan, built on first use (rsp_trsv_upper)
    hp->sym = rsp_an::IluSymbolic();
    hp->fplan = rsp_an::FacPlan();
    hp->L = rsp_an::DagHost();
    hp->LT = rsp_an::DagHost();
    hp->F = rsp_an::DagHost();
    hp->Lb = rsp_an::BlkPlanHost();
    hp->LTb = rsp_an::BlkPlanHost();
    hp->ltp.clear();
    hp->lts.clear();
    hp->ltc.clear();
    hp->udiv.clear();
    hp->frow.clear();
    hp->slot_desc.clear();
    hp->slot_offs.clear();
    f->solves_ready = true;
    return RSP_STATUS_SUCCESS;
}

// The U DAG's plan (rsp_trsv_upper, the --true-lu extension), on first use.
rsp_status_t rsp_api::ilu_plan_u(rsp_handle_t h, rsp_ilu0_info *f) {
    if (f->U.plan.ptr_dev) return RSP_STATUS_SUCCESS;
    if (!f->host) return RSP_STATUS_INTERNAL_ERROR;
    rsp_an::plan_u(f->host_rp.data(), f->host_ci.data(), *f->host);
    Arena ar;
    dag_upload(ar, f->U, f->host->U);
    // its streams (the L / L^T ones are sized for those DAGs' terms)
    ar.space(&f->d_usval, (size_t)std::max(f->U.nterms, 1) * sizeof(double));
    hipError_t e = ar.commit(f->arena_u, h->stream);
    f->host->U = rsp_an::DagHost();
    if (e != hipSuccess) {  // (L and L^T stay usable)
        f->arena_u = DevMem();
        f->U = Dag();
        return e == hipErrorOutOfMemory ? RSP_STATUS_ALLOC_FAILED : RSP_STATUS_EXECUTION_FAILED;
    }
    return RSP_STATUS_SUCCESS;
}

extern "C" {

rsp_status_t rsp_create_ilu0_info(rsp_ilu0_info_t *info) {
    if (!info) return RSP_STATUS_INVALID_VALUE;
    *info = new (std::nothrow) rsp_ilu0_info();
    return *info ? RSP_STATUS_SUCCESS : RSP_STATUS_ALLOC_FAILED;
}

rsp_status_t rsp_destroy_ilu0_info(rsp_ilu0_info_t info) {
    if (!info) return RSP_STATUS_INVALID_VALUE;
    delete info;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_ilu0_buffer_size(rsp_handle_t h, int n, int nnz, rsp_datatype_t value_type,
                                  rsp_ilu0_info_t info, size_t *buffer_size) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!info || !buffer_size || n < 0 || nnz < 0) return RSP_STATUS_INVALID_VALUE;
    if (value_type != RSP_R_64F && value_type != RSP_R_32F) return RSP_STATUS_INVALID_VALUE;
    *buffer_size = 0;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_ilu0_analysis(rsp_handle_t h, int n, int nnz, const int *d_row_offsets,
                               const int *d_col_ind, rsp_ilu0_info_t f) {
    return guarded([&] { return ilu0_analysis(h, n, nnz, d_row_offsets, d_col_ind, f); },
                   [&] {
                       if (f) f->reset();
                   });
}

rsp_status_t rsp_ilu0_analysis_host(int n, const int *row_offsets, const int *col_ind,
                                    int *levels_lower, int *levels_upper, uint64_t *digest,
                                    double *phase_ms) {
    return guarded([&] {
        rsp_an::Phases ph;
        ph.n = n;
        ph.ms = phase_ms;
        if (phase_ms)
            for (int i = 0; i < rsp_an::kPhases; i++) phase_ms[i] = 0.0;
        ph.start();
        rsp_an::IluHostPlan hp;
        RSP_TRY(rsp_an::plan_host(n, row_offsets, col_ind, host_slot_cap_ints(), false, hp, ph));
        if (levels_lower) *levels_lower = (int)hp.L.ptr.size() - 1;
        if (levels_upper) *levels_upper = (int)hp.LT.ptr.size() - 1;
        if (digest) *digest = rsp_an::digest(hp);
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_ilu0_plan_facts_host(int n, const int *row_offsets, const int *col_ind, int64_t *facts, int nfacts) {
    return guarded([&] {
        if (nfacts < 0 || (nfacts > 0 && !facts)) return RSP_STATUS_INVALID_VALUE;
        rsp_an::Phases ph;
        ph.n = n;
        ph.start();
        const long long cap = host_slot_cap_ints();
        rsp_an::IluHostPlan hp;
        RSP_TRY(rsp_an::plan_host(n, row_offsets, col_ind, cap, true, hp, ph));
        const std::string why = rsp_an::check_plans(row_offsets, col_ind, hp, cap);
        if (!why.empty()) {
            fprintf(stderr, "rsp_ilu0_plan_facts_host n=%d: %s\n", n, why.c_str());
            return RSP_STATUS_INTERNAL_ERROR;
        }
        long long f[rsp_an::kPlanFacts];
        rsp_an::plan_facts(row_offsets, hp, cap, f);
        for (int k = 0; k < nfacts; k++) facts[k] = k < rsp_an::kPlanFacts ? (int64_t)f[k] : 0;
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_trsv_analysis(rsp_handle_t h, rsp_operation_t op, rsp_ilu0_info_t f) {
    return guarded([&] {
        if (!h) return RSP_STATUS_NOT_INITIALIZED;
        if (!f || !f->analysed) return RSP_STATUS_INVALID_VALUE;
        if (op != RSP_OPERATION_NON_TRANSPOSE && op != RSP_OPERATION_TRANSPOSE) return RSP_STATUS_INVALID_VALUE;
        return ilu_solves_ready(h, f);
    });
}

rsp_status_t rsp_ilu0_plan_digest(rsp_ilu0_info_t f, uint64_t *digest) {
    return guarded([&] {
        if (!f || !digest || !f->analysed) return RSP_STATUS_INVALID_VALUE;
        RSP_TRY(ilu_solves_ready(f->han, f));  // (the digest covers the solve plans)
        if (!f->digest) return RSP_STATUS_INVALID_VALUE;
        *digest = f->digest;
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_ilu0_solve_blocks(rsp_ilu0_info_t f, int *blocks_lower, int *blocks_upper) {
    return guarded([&] {
        if (!f || !blocks_lower || !blocks_upper || !f->analysed) return RSP_STATUS_INVALID_VALUE;
        RSP_TRY(ilu_solves_ready(f->han, f));
        *blocks_lower = f->Lb.on ? f->Lb.args.nb : 0;
        *blocks_upper = f->LTb.on ? f->LTb.args.nb : 0;
        return RSP_STATUS_SUCCESS;
    });
}

rsp_status_t rsp_ilu0_levels(rsp_ilu0_info_t f, int *levels_lower, int *levels_upper) {
    return guarded([&] {
        if (!f || !f->analysed) return RSP_STATUS_INVALID_VALUE;
        if (levels_upper) RSP_TRY(ilu_solves_ready(f->han, f));  // (the L^T levels come with the solve plans)
        if (levels_lower) *levels_lower = (int)f->L.ptr.size() - 1;
        if (levels_upper) *levels_upper = (int)f->LT.ptr.size() - 1;
        return RSP_STATUS_SUCCESS;
    });
}

}  // the C ABI
