// rsp_api.cpp — the handle, the matrix descriptor and SpMV of include/rsp.h
// (the C-ABI operator library librsp.so): the host-side row-block schedule
// (make_tile_plan), the launches of the kernels in spmv.hip, the batch,
// gather / scatter. Mirrors the cuSPARSE lifecycle the reference driver uses
// (GPU/spmv.cu:122-186); see include/rsp.h for the per-call mapping. ILU(0)
// and the Krylov solvers: api_ilu_analysis.cpp, api_ilu_solve.cpp,
// api_krylov.cpp (rsp_internal.h).

#include "rsp_internal.h"
#include "spmv_pack.h"

#include <atomic>

using namespace rsp_api;

using rsp::SpmvBlock;
using rsp::SpmvLongRow;
using rsp::SpmvTile;

namespace {
std::atomic<unsigned long long> g_plan_next{1};
unsigned long long plan_new_gen() { return g_plan_next.fetch_add(1); }
}  // namespace

/* ----------------------------------------------------------------- SpMV */

struct SpmvBounds {
    size_t nblocks, nlong, nslots;
};

static SpmvBounds spmv_bounds(int64_t rows, int64_t nnz, int cap) {
    // greedy packing: two consecutive size-closed tiles exceed `cap`, long
    // rows contribute <= nnz/cap + 1 chunks each side.
    // + every row longer than kSpmvLongRow may sit in a tile of its own and
    // close the tile before it: <= 2 * nnz / kSpmvLongRow extra tiles.
    SpmvBounds b;
    size_t q = (size_t)(nnz / cap) + 1;
    size_t l = (size_t)(nnz / rsp::kSpmvLongRow) + 1;
    b.nlong = q;
    b.nslots = 2 * q + 1;
    b.nblocks = 6 * q + 2 * l + (size_t)(rows / rsp::kSpmvMaxRows) + 8;
    b.nblocks += std::min<size_t>(b.nblocks, 8192);  // headroom for spread-out small plans
    return b;
}

// Workspace: [tiles | long rows | chunk partials | per-tile column base |
// per-tile packed-record offset | 16-bit column offsets (2 B per stored
// entry) | staged tiles' runs, then their packed records].
struct SpmvLayout {
    size_t off_long, off_part, off_cbase, off_poff, off_cidx, off_runs, bytes;
};
static SpmvLayout spmv_layout(const SpmvBounds &b, size_t elem, int64_t nnz, size_t run_ints = 0) {
    SpmvLayout l;
    l.off_long = align256(b.nblocks * sizeof(SpmvBlock));
    l.off_part = l.off_long + align256(b.nlong * sizeof(SpmvLongRow));
    l.off_cbase = l.off_part + align256(b.nslots * 2 * elem);  // value + ticket per slot
    l.off_poff = l.off_cbase + align256(b.nblocks * sizeof(int));
    l.off_cidx = l.off_poff + align256(b.nblocks * sizeof(int));
    l.off_runs = l.off_cidx + align256((size_t)std::max<int64_t>(nnz, 0) * sizeof(uint16_t));
    l.bytes = l.off_runs + align256(run_ints * sizeof(int));
    return l;
}

static int tile_cap(rsp_datatype_t t) {
    return t == RSP_R_64F ? SpmvTile<double>::kMaxNnz : SpmvTile<float>::kMaxNnz;
}
static int chunk_cap(rsp_datatype_t t) {
    return t == RSP_R_64F ? SpmvTile<double>::kChunk : SpmvTile<float>::kChunk;
}
// Tile row cuts: RSP_SPMV_VARIANT bit 6 aligns them to 128-B y lines, bit 7
// to 64 B (tuning knob; default unaligned).
static int spmv_row_align(rsp_handle_t h, rsp_datatype_t t) {
    const int e = (int)elem_size(t);
    return (h->spmv_variant & 64) ? 128 / e : (h->spmv_variant & 128) ? 64 / e : 1;
}

// Greedy row-block schedule over host row offsets (see spmv.hip header).
// Rows longer than kSpmvLongRow get tiles of their own (one per `chunk`
// entries); the others are packed into tiles of <= cap entries / maxrows rows.
static int build_spmv_plan(const int *rp, int m, int cap, int chunk, rsp_an::hvec<SpmvBlock> &blocks,
                           rsp_an::hvec<SpmvLongRow> &longrows, int *nslots,
                           int maxrows = rsp::kSpmvMaxRows, int row_align = 1) {
    blocks.clear();
    longrows.clear();
    int slots = 0;
    int r = 0;
    while (r < m) {
        int len = rp[r + 1] - rp[r];
        if (len > rsp::kSpmvLongRow) {
            if (len <= chunk) {  // one chunk: reduced and written in place
                SpmvBlock b;
                b.r0 = r;
                b.r1 = rsp::kSpmvWholeRow;
                b.k0 = rp[r];
                b.k1 = rp[r + 1];
                blocks.push_back(b);
                r++;
                continue;
            }
            SpmvLongRow lr;
            lr.row = r;
            lr.first = slots;
            lr.nchunks = 0;
            lr.pad = 0;
            for (int k = rp[r]; k < rp[r + 1]; k += chunk) {
                SpmvBlock b;
                b.r0 = r;
                b.r1 = -(slots + 1);
                b.k0 = k;
                b.k1 = std::min(k + chunk, rp[r + 1]);
                blocks.push_back(b);
                slots++;
                lr.nchunks++;
            }
            longrows.push_back(lr);
            r++;
            continue;
        }
        int start = r, nnz = 0;
        while (r < m && r - start < maxrows) {
            int l = rp[r + 1] - rp[r];
            // a tile always takes its first row (<= kSpmvLongRow <= kMaxNnz)
            if (l > rsp::kSpmvLongRow || (r > start && nnz + l > cap)) break;
            nnz += l;
            r++;
        }
        // row_align > 1: end a packed tile on a multiple of row_align rows,
        // so its y stores cover whole lines, where the tile keeps >= 3/4 of
        // its entries
        if (row_align > 1 && r < m && r % row_align != 0) {
            const int ra = r - r % row_align;
            if (ra > start && (int64_t)(rp[ra] - rp[start]) * 4 >= (int64_t)(rp[r] - rp[start]) * 3) r = ra;
        }
        SpmvBlock b;
        b.r0 = start;
        b.r1 = r;
        b.k0 = rp[start];
        b.k1 = rp[r];
        blocks.push_back(b);
    }
    *nslots = slots;
    return 0;
}

// A complete SpMV schedule over host row offsets `rp` and column indices `ci`:
// tiles (interior tiles first when local_cols >= 0), long rows, per-tile
// column base and the 16-bit column offsets.
struct TilePlan {
    rsp_an::hvec<SpmvBlock> blocks;
    rsp_an::hvec<SpmvLongRow> longrows;
    int nslots = 0, nint = 0;
    rsp_an::hvec<int> cbase;
    rsp_an::hvec<uint16_t> c16;
    rsp_an::hvec<int> runs;  // staged tiles' run descriptors (int pairs), then the packed records; SpmvArgs::runs
    rsp_an::hvec<int> poff;  // per tile: packed record (SpmvArgs::poffs), -1 = none
    int64_t nnz_c16 = 0;     // entries not read through the int32 colidx (16-bit offsets, slot indices, packed slots)
    int64_t nnz_staged = 0;  // ... of which in staged tiles
    int64_t tiles_packed = 0, nnz_packed = 0;  // ... of which in packed tiles
};

// RSP_SPMV_PACK (plan time): 0 no packed records (the unpacked plan), 1 the
// slot fields only, 2 (default) slot fields and row offsets. On the big set's
// batched fp64 launch: 534.8 / 530.7 / 518.8 us (profiles/r07_pack_ab.txt).
static int spmv_pack_mode() { return std::min(std::max(env_int("RSP_SPMV_PACK", 2), 0), 2); }

// Packed records (spmv_pack.h) of the staged tiles whose slot fields are
// strictly fewer bytes than their 16-bit words, appended to p.runs after every
// run descriptor (whose offsets have the smaller range), each 16-B aligned.
// An offset past the encoding's range leaves the tile unpacked.
template <typename T>
static void pack_staged_tiles(const int *rp, TilePlan &p, int mode) {
    constexpr int VW = SpmvTile<T>::kVec, IT = rsp::kSpmvIter, NTH = rsp::kSpmvThreads;
    constexpr int IW = rsp_pack::index_words(NTH, IT * VW);
    p.poff.assign(p.blocks.size(), -1);
    p.tiles_packed = p.nnz_packed = 0;
    if (mode <= 0) return;
    int64_t end = ((int64_t)p.runs.size() + 3) & ~(int64_t)3;
    for (size_t t = 0; t < p.blocks.size(); t++) {
        const SpmvBlock &b = p.blocks[t];
        if (p.cbase[t] > -2 || b.r1 < 0 || !rsp_pack::eligible(NTH, IT * VW, b.k1 - b.k0)) continue;
        const int64_t words = IW + (mode >= 2 ? rsp_pack::row_words(b.r1 - b.r0) : 0);
        if (end + words >= (1LL << 30)) break;  // (poff = word << 1 | rows; never reached on real matrices)
        p.poff[t] = (int)(end << 1) | (mode >= 2 ? 1 : 0);
        end = (end + words + 3) & ~(int64_t)3;
        p.tiles_packed++;
        p.nnz_packed += b.k1 - b.k0;
    }
    if (p.tiles_packed == 0) return;
    p.runs.resize((size_t)end + 4, 0);  // (+ 16 B: a vector load of a record's last words stays inside)
    rsp_an::parallel_for((long long)p.blocks.size(), 64, [&](long long t0, long long t1) {
        for (long long t = t0; t < t1; t++) {
            if (p.poff[(size_t)t] < 0) continue;
            const SpmvBlock &b = p.blocks[(size_t)t];
            uint32_t *rec = reinterpret_cast<uint32_t *>(p.runs.data()) + (p.poff[(size_t)t] >> 1);
            rsp_pack::pack_slots(p.c16.data(), b.k0, b.k1, VW, IT, NTH, rec);
            if (p.poff[(size_t)t] & 1) rsp_pack::pack_rows(rp, b.r0, b.r1 - b.r0, b.k0 & ~(VW - 1), rec + IW);
        }
    });
}

// spread > 0: a plan of fewer tiles than `spread` (the resident workgroup
// slots it may use) is re-packed into up to `spread` smaller tiles, so a lone
// launch does not leave slots idle. Long rows do not depend on the packing
// cap (they are cut at the fixed chunk), so every spread of one matrix has
// the same long rows and partial slots.
static void make_tile_plan(const int *rp, const int *ci, int m, int64_t nnz_bound,
                           rsp_datatype_t type, int64_t spread, int64_t local_cols, bool use_c16,
                           TilePlan &p, int row_align = 1, bool use_stage = true) {
    const int chunk = chunk_cap(type);
    const int cap = tile_cap(type);
    const int align = row_align;
    const int maxrows = type == RSP_R_64F ? SpmvTile<double>::kMaxRows : SpmvTile<float>::kMaxRows;
    build_spmv_plan(rp, m, cap, chunk, p.blocks, p.longrows, &p.nslots, maxrows, align);
    const int64_t nb = (int64_t)p.blocks.size();
    if (spread > 0 && nb > 0 && nb < spread) {
        const SpmvBounds bb = spmv_bounds(m, std::max<int64_t>(nnz_bound, 0), chunk);
        const int64_t nnz_s = rp[(size_t)m];
        int c = (int)std::max<int64_t>(64, std::min<int64_t>(cap, (nnz_s + spread - 1) / spread));
        for (int tries = 0; tries < 32 && c < cap; tries++) {
            rsp_an::hvec<SpmvBlock> b2;
            rsp_an::hvec<SpmvLongRow> l2;
            int s2 = 0;
            build_spmv_plan(rp, m, c, chunk, b2, l2, &s2, maxrows, align);
            if ((int64_t)b2.size() <= spread && b2.size() <= bb.nblocks) {
                p.blocks.swap(b2);
                p.longrows.swap(l2);
                p.nslots = s2;
                break;
            }
            c += std::max(8, c / 16);
        }
    }
    // Random-band matrices (round 4): tiles whose columns lie in a band
    // narrower than 65536 but scattered over it (more runs than a staged
    // tile's run table holds) are staged by an explicit column LIST instead
    // (below); that needs at most kStageSlots distinct columns per tile, so
    // such a matrix is re-packed with tiles of at most kStageSlots entries
    // (the canonical summation order does not depend on the packing). Judged
    // on a sample of 64 tiles; not for spread plans (already small tiles).
    const int ucap = type == RSP_R_64F ? SpmvTile<double>::kStageSlots : SpmvTile<float>::kStageSlots;
    const bool list_ok = use_stage && use_c16 && type == RSP_R_64F && SpmvTile<double>::kStageList &&
                         env_int("RSP_SPMV_STAGE_LIST", 1) != 0;
    if (list_ok && (int64_t)p.blocks.size() == nb && nb > 0) {
        int64_t band = 0, all = 0;
        std::vector<int> cols;
        const size_t step = std::max<size_t>(1, p.blocks.size() / 64);
        for (size_t t = 0; t < p.blocks.size(); t += step) {
            const SpmvBlock &bk = p.blocks[t];
            if (bk.r1 < 0 || bk.k1 <= bk.k0) continue;
            cols.assign(ci + bk.k0, ci + bk.k1);
            std::sort(cols.begin(), cols.end());
            cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
            int R = 1;
            for (size_t u = 1; u < cols.size(); u++) R += cols[u] != cols[u - 1] + 1;
            all += bk.k1 - bk.k0;
            if (cols.back() - cols.front() <= 65535 && R > rsp::kStageRuns && (int)cols.size() > ucap)
                band += bk.k1 - bk.k0;
        }
        if (2 * band > all) {
            rsp_an::hvec<SpmvBlock> b2;
            rsp_an::hvec<SpmvLongRow> l2;
            int s2 = 0;
            // RSP_SPMV_LIST_CAP (A/B knob): a smaller tile for the re-packed plan
            const int lcap = std::min(std::max(env_int("RSP_SPMV_LIST_CAP", ucap), 64), ucap);
            build_spmv_plan(rp, m, std::min(cap, lcap), chunk, b2, l2, &s2, maxrows, align);
            p.blocks.swap(b2);
            p.longrows.swap(l2);
            p.nslots = s2;
        }
    }
    // split schedule (rsp_spmat_set_local_cols): tiles reading own columns
    // only first; long-row tiles always in the second part (with the fixup)
    p.nint = 0;
    if (local_cols >= 0) {
        auto interior = [&](const SpmvBlock &b) {
            if (b.r1 < 0) return false;
            for (int k = b.k0; k < b.k1; k++)
                if (ci[(size_t)k] >= local_cols) return false;
            return true;
        };
        auto mid = std::stable_partition(p.blocks.begin(), p.blocks.end(), interior);
        p.nint = (int)(mid - p.blocks.begin());
    }
    // 16-bit column offsets: a tile whose columns span < 65536 reads
    // col = cbase + off (2 B per entry instead of 4; the int32 colidx is not
    // read for it). Staged tiles (round 4, spmv.hip stream_products_staged):
    // where the tile's distinct columns are few (at most kStageSlots, at most
    // RSP_SPMV_STAGE_PCT % of its entries, default 80) in at most kStageRuns
    // contiguous runs, its 16-bit values are instead the entries' slots in the
    // sorted list of those columns, and the runs ({first column, first slot},
    // then {0, slots}) go to `runs`. Tiles are planned in parallel.
    const int64_t nnz_s = m > 0 ? rp[(size_t)m] : 0;
    p.cbase.assign(p.blocks.size(), -1);
    p.c16.clear();
    p.runs.clear();
    p.poff.assign(p.blocks.size(), -1);
    p.tiles_packed = p.nnz_packed = 0;
    p.nnz_c16 = 0;
    p.nnz_staged = 0;
    if (use_c16 && nnz_s > 0 && nnz_s <= nnz_bound) {
        p.c16.assign((size_t)nnz_s, 0);
        const long long nt = (long long)p.blocks.size();
        const long long pct = std::min(std::max(env_int("RSP_SPMV_STAGE_PCT", 80), 0), 100);
        const int64_t xelem = type == RSP_R_64F ? 8 : 4;
        std::vector<std::vector<int>> truns(use_stage ? (size_t)nt : 0);
        std::vector<char> tmode(use_stage ? (size_t)nt : 0, 0);  // 1 runs, 2 list
        std::atomic<int64_t> n16{0}, nst{0};
        rsp_an::parallel_for(nt, 64, [&](long long t0, long long t1) {
            std::vector<int> cols;
            int64_t c16n = 0, stn = 0;
            for (long long t = t0; t < t1; t++) {
                const SpmvBlock &bk = p.blocks[(size_t)t];
                if (bk.k1 <= bk.k0) continue;
                int lo = ci[(size_t)bk.k0], hi = lo;
                for (int k = bk.k0 + 1; k < bk.k1; k++) {
                    lo = std::min(lo, ci[(size_t)k]);
                    hi = std::max(hi, ci[(size_t)k]);
                }
                if (hi - lo > 65535) continue;
                const int len = bk.k1 - bk.k0;
                c16n += len;
                // staged x loads use 32-bit byte offsets into a buffer resource of
                // 0x7ffffffc bytes (spmv.hip stream_products_staged): a tile whose
                // columns reach past that keeps the plain 16-bit offsets
                const bool x_in_rsrc = ((int64_t)hi + 1) * xelem <= (int64_t)0x7ffffffc;
                if (use_stage && bk.r1 >= 0 && x_in_rsrc) {  // (long-row chunks keep the offsets)
                    cols.assign(ci + bk.k0, ci + bk.k1);
                    std::sort(cols.begin(), cols.end());
                    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
                    const int U = (int)cols.size();
                    int R = 1;
                    for (int u = 1; u < U; u++) R += cols[(size_t)u] != cols[(size_t)u - 1] + 1;
                    const bool runs_mode = U <= ucap && R <= rsp::kStageRuns && 100LL * U <= pct * len;
                    const bool list_mode = !runs_mode && list_ok && U <= ucap && R > rsp::kStageRuns;
                    if (runs_mode || list_mode) {
                        std::vector<int> &r = truns[(size_t)t];
                        tmode[(size_t)t] = runs_mode ? 1 : 2;
                        if (runs_mode) {
                            r.reserve(2 * (size_t)(R + 1));
                            for (int u = 0; u < U; u++)
                                if (u == 0 || cols[(size_t)u] != cols[(size_t)u - 1] + 1) {
                                    r.push_back(cols[(size_t)u]);
                                    r.push_back(u);
                                }
                            r.push_back(0);
                            r.push_back(U);
                        } else {  // {base column, U}, then the U column offsets as uint16, padded to 8 B
                            r.assign(2 + 2 * (size_t)((U + 3) / 4), 0);
                            r[0] = cols[0];
                            r[1] = U;
                            uint16_t *o = reinterpret_cast<uint16_t *>(r.data() + 2);
                            for (int u = 0; u < U; u++) o[u] = (uint16_t)(cols[(size_t)u] - cols[0]);
                        }
                        for (int k = bk.k0; k < bk.k1; k++)
                            p.c16[(size_t)k] = (uint16_t)(std::lower_bound(cols.begin(), cols.end(), ci[(size_t)k]) -
                                                          cols.begin());
                        stn += len;
                        continue;
                    }
                }
                p.cbase[(size_t)t] = lo;
                for (int k = bk.k0; k < bk.k1; k++) p.c16[(size_t)k] = (uint16_t)(ci[(size_t)k] - lo);
            }
            n16 += c16n;
            nst += stn;
        });
        p.nnz_c16 = n16;
        p.nnz_staged = nst;
        if (use_stage) {  // descriptors concatenated in tile order; cbase = -2 - (pair offset << 8 | runs)
            for (size_t t = 0; t < truns.size(); t++) {
                const std::vector<int> &r = truns[t];
                if (r.empty()) continue;
                const int64_t off = (int64_t)p.runs.size() / 2;
                // runs mode: descriptors + sentinel; list mode: 255 (header {base, U} + offsets)
                const int nr = tmode[t] == 2 ? 255 : (int)r.size() / 2 - 1;
                if (off >= (1LL << 22)) {  // (encoding range; never reached on real matrices)
                    p.nnz_c16 -= p.blocks[t].k1 - p.blocks[t].k0;
                    p.nnz_staged -= p.blocks[t].k1 - p.blocks[t].k0;
                    continue;  // cbase stays -1: the int32 path
                }
                p.cbase[t] = -2 - (int)((off << 8) | nr);
                p.runs.insert(p.runs.end(), r.begin(), r.end());
            }
            if (type == RSP_R_64F)
                pack_staged_tiles<double>(rp, p, spmv_pack_mode());
            else
                pack_staged_tiles<float>(rp, p, spmv_pack_mode());
        }
    }
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

static int64_t spmv_resident_tiles(rsp_handle_t h, rsp_datatype_t t) {
    return (int64_t)rsp_k::spmv_tiles_per_cu((int)elem_size(t)) * h->num_cus;
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
    // every small matrix (A/B), bit 5 keeps every tile on the int32 indices.
    // A batch re-plans its members itself (rsp_spmv_batch_create). Tiling
    // never changes the result (canonical summation order).
    const bool spread = (h->spmv_variant & 512) != 0;
    TilePlan p;
    make_tile_plan(rp.data(), ci.data(), m, mat->nnz, compute_type,
                   spread ? spmv_resident_tiles(h, compute_type) : 0,
                   mat->local_cols, !(h->spmv_variant & 32), p, spmv_row_align(h, compute_type),
                   !(h->spmv_variant & rsp::kSpmvVariantNoStage));
    const rsp_an::hvec<SpmvBlock> &blocks = p.blocks;
    const rsp_an::hvec<SpmvLongRow> &longrows = p.longrows;
    const int nslots = p.nslots, nint = p.nint;
    const rsp_an::hvec<int> &cbase = p.cbase;
    const rsp_an::hvec<uint16_t> &c16 = p.c16;
    const int64_t nnz_c16 = p.nnz_c16;
    // exact layout of this schedule in the matrix's device memory (grown,
    // never shrunk, on a re-plan)
    SpmvBounds b{blocks.size(), longrows.size(), (size_t)nslots};
    const SpmvLayout lay = spmv_layout(b, elem_size(compute_type), (int64_t)c16.size(), p.runs.size());
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
    if (!blocks.empty()) {
        RSP_CHECK_HIP(hipMemcpyAsync(buf, blocks.data(), blocks.size() * sizeof(SpmvBlock),
                                     hipMemcpyHostToDevice, h->stream));
        RSP_CHECK_HIP(hipMemcpyAsync(buf + lay.off_cbase, cbase.data(), cbase.size() * sizeof(int),
                                     hipMemcpyHostToDevice, h->stream));
        RSP_CHECK_HIP(hipMemcpyAsync(buf + lay.off_poff, p.poff.data(), p.poff.size() * sizeof(int),
                                     hipMemcpyHostToDevice, h->stream));
    }
    if (!c16.empty())
        RSP_CHECK_HIP(hipMemcpyAsync(buf + lay.off_cidx, c16.data(), c16.size() * sizeof(uint16_t),
                                     hipMemcpyHostToDevice, h->stream));
    if (!p.runs.empty())
        RSP_CHECK_HIP(hipMemcpyAsync(buf + lay.off_runs, p.runs.data(), p.runs.size() * sizeof(int),
                                     hipMemcpyHostToDevice, h->stream));
    const size_t off_long = lay.off_long, off_part = lay.off_part;
    if (!longrows.empty())
        RSP_CHECK_HIP(hipMemcpyAsync(buf + off_long, longrows.data(),
                                     longrows.size() * sizeof(SpmvLongRow), hipMemcpyHostToDevice,
                                     h->stream));
    // partial slots: the long rows' arrival tickets start (and stay) at 0
    if (nslots > 0)
        RSP_CHECK_HIP(hipMemsetAsync(buf + off_part, 0, (size_t)nslots * 2 * elem_size(compute_type),
                                     h->stream));
    RSP_CHECK_HIP(hipStreamSynchronize(h->stream));
    mat->planned = 1;
    mat->plan_type = compute_type;
    mat->nblocks = (int)blocks.size();
    mat->nint = nint;
    mat->plan_gen = plan_new_gen();
    mat->nlong = (int)longrows.size();
    mat->nslots = nslots;
    mat->nnz_s = m > 0 ? rp[(size_t)m] : 0;
    mat->off_long = off_long;
    mat->off_part = off_part;
    mat->off_cbase = lay.off_cbase;
    mat->off_poff = lay.off_poff;
    mat->off_cidx = lay.off_cidx;
    mat->off_runs = lay.off_runs;
    mat->nnz_c16 = nnz_c16;
    mat->nnz_staged = p.nnz_staged;
    return RSP_STATUS_SUCCESS;
}

rsp_status_t rsp_api::spmv_run(rsp_handle_t h, rsp_operation_t op, const void *alpha, rsp_spmat_t mat,
                               const void *d_x, const void *beta, void *d_y,
                               rsp_datatype_t compute_type, void *d_buffer, int part) {
    if (!h) return RSP_STATUS_NOT_INITIALIZED;
    if (!mat || !alpha || !beta) return RSP_STATUS_INVALID_VALUE;
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
    a.cbases = (const int *)(plan + mat->off_cbase);
    a.poffs = (const int *)(plan + mat->off_poff);
    a.cidx = (const unsigned short *)(plan + mat->off_cidx);
    a.runs = (const int *)(plan + mat->off_runs);
    a.cmax = mat->cols > 0 ? (int)(mat->cols - 1) : 0;
    a.longrows = (const SpmvLongRow *)(plan + mat->off_long);
    a.nlong = mat->nlong;
    a.partials = plan + mat->off_part;
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
    const bool spread_ok = !(h->spmv_variant & 16), c16_ok = !(h->spmv_variant & 32);
    const bool stage_ok = !(h->spmv_variant & rsp::kSpmvVariantNoStage);
    rsp_an::hvec<TilePlan> plans((size_t)count);
    // layout: per launch [entries | tiles | tile column bases | long rows |
    // 16-bit column offsets of each matrix | long-row partials and tickets of
    // each matrix (zero)], each 16-B aligned
    struct Span { int first, count; size_t off_e, off_t, off_c, off_k, off_l; rsp_an::hvec<size_t> off_16, off_p, off_r; };
    rsp_an::hvec<Span> spans;
    size_t bytes = 0;
    auto tile_range = [part](const TilePlan &p, int *t0, int *t1) {
        *t0 = part == 2 ? p.nint : 0;
        *t1 = part == 1 ? p.nint : (int)p.blocks.size();
    };
    for (int first = 0; first < count; first += rsp::kSpmvBatchMax) {
        Span sp{first, std::min(rsp::kSpmvBatchMax, count - first), 0, 0, 0, 0, 0, {}, {}, {}};
        rsp_an::hvec<rsp_an::hvec<int>> rps((size_t)sp.count), cis((size_t)sp.count);
        int64_t nt_full = 0, nnz_all = 0;
        for (int q = 0; q < sp.count; q++) {
            rsp_spmat_t A = mats[first + q];
            rsp_status_t st = download_pattern(h, A, rps[q], cis[q]);
            if (st != RSP_STATUS_SUCCESS) return st;
            make_tile_plan(rps[q].data(), cis[q].data(), (int)A->rows, A->nnz, compute_type, 0,
                           A->local_cols, c16_ok, plans[first + q], spmv_row_align(h, compute_type), stage_ok);
            int t0, t1;
            tile_range(plans[first + q], &t0, &t1);
            nt_full += t1 - t0;
            nnz_all += A->rows > 0 ? rps[q][(size_t)A->rows] : 0;
        }
        if (spread_ok && nt_full < R)
            for (int q = 0; q < sp.count; q++) {
                rsp_spmat_t A = mats[first + q];
                const int64_t nnz_q = A->rows > 0 ? rps[q][(size_t)A->rows] : 0;
                const int64_t share = std::max<int64_t>(1, R * nnz_q / std::max<int64_t>(1, nnz_all));
                make_tile_plan(rps[q].data(), cis[q].data(), (int)A->rows, A->nnz, compute_type,
                               share, A->local_cols, c16_ok, plans[first + q],
                               spmv_row_align(h, compute_type), stage_ok);
            }
        int nt = 0, nl = 0;
        for (int q = 0; q < sp.count; q++) {
            const TilePlan &p = plans[first + q];
            rsp_spmat_t A = mats[first + q];
            // the long rows index partial slots of the matrix's own workspace
            if ((int)p.longrows.size() != A->nlong || p.nslots != A->nslots)
                return RSP_STATUS_INTERNAL_ERROR;
            int t0, t1;
            tile_range(p, &t0, &t1);
            nt += t1 - t0;
            nl += part == 1 ? 0 : (int)p.longrows.size();
        }
        sp.off_e = bytes;
        bytes += (size_t)sp.count * sizeof(rsp::SpmvBatchEntry);
        sp.off_t = bytes;
        bytes += (size_t)nt * sizeof(SpmvBlock);
        sp.off_c = bytes;
        bytes += ((size_t)nt * sizeof(int) + 15) & ~(size_t)15;
        sp.off_k = bytes;
        bytes += ((size_t)nt * sizeof(int) + 15) & ~(size_t)15;
        sp.off_l = bytes;
        bytes += ((size_t)nl * sizeof(SpmvLongRow) + 15) & ~(size_t)15;
        for (int q = 0; q < sp.count; q++) {
            sp.off_16.push_back(bytes);
            bytes += (plans[first + q].c16.size() * sizeof(uint16_t) + 15) & ~(size_t)15;
        }
        for (int q = 0; q < sp.count; q++) {
            sp.off_r.push_back(bytes);
            bytes += (plans[first + q].runs.size() * sizeof(int) + 15) & ~(size_t)15;
        }
        for (int q = 0; q < sp.count; q++) {
            sp.off_p.push_back(bytes);
            const size_t pb = (size_t)plans[first + q].nslots * 2 * elem_size(compute_type);
            bytes += (pb + 15) & ~(size_t)15;
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
        auto region = [&](size_t off, size_t len) {
            const bool ok = off >= end && off + len <= bytes;
            end = off + len;
            return ok;
        };
        for (const Span &sp : spans) {
            int nt = 0, nl = 0;
            for (int q = 0; q < sp.count; q++) {
                int t0, t1;
                tile_range(plans[sp.first + q], &t0, &t1);
                nt += t1 - t0;
                nl += part == 1 ? 0 : (int)plans[sp.first + q].longrows.size();
            }
            bool ok = region(sp.off_e, (size_t)sp.count * sizeof(rsp::SpmvBatchEntry)) &&
                      region(sp.off_t, (size_t)nt * sizeof(SpmvBlock)) && region(sp.off_c, (size_t)nt * sizeof(int)) &&
                      region(sp.off_k, (size_t)nt * sizeof(int)) && region(sp.off_l, (size_t)nl * sizeof(SpmvLongRow));
            for (int q = 0; ok && q < sp.count; q++) ok = region(sp.off_16[q], plans[sp.first + q].c16.size() * 2);
            for (int q = 0; ok && q < sp.count; q++) ok = region(sp.off_r[q], plans[sp.first + q].runs.size() * 4);
            for (int q = 0; ok && q < sp.count; q++)
                ok = region(sp.off_p[q], (size_t)plans[sp.first + q].nslots * 2 * elem_size(compute_type));
            if (!ok) return RSP_STATUS_INTERNAL_ERROR;
        }
    }
    if (bytes > 0) RSP_CHECK_HIP(hipMalloc(&b->d_mem, bytes));
    rsp_an::hvec<unsigned char> host(bytes);
    for (const Span &sp : spans) {
        rsp::SpmvBatchArgs a{};
        a.entries = (const rsp::SpmvBatchEntry *)((char *)b->d_mem + sp.off_e);
        a.tiles = (const SpmvBlock *)((char *)b->d_mem + sp.off_t);
        a.cbases = (const int *)((char *)b->d_mem + sp.off_c);
        a.poffs = (const int *)((char *)b->d_mem + sp.off_k);
        a.longrows = (const SpmvLongRow *)((char *)b->d_mem + sp.off_l);
        a.count = sp.count;
        for (int q = 0; q <= rsp::kSpmvBatchMax; q++)
            a.tiles_at.begin[q] = a.longs_at.begin[q] = INT_MAX;
        int nt = 0, nl = 0;
        for (int q = 0; q < sp.count; q++) {
            rsp_spmat_t A = mats[sp.first + q];
            const TilePlan &p = plans[sp.first + q];
            int t0, t1;
            tile_range(p, &t0, &t1);
            const int nlq = part == 1 ? 0 : (int)p.longrows.size();
            rsp::SpmvBatchEntry e{};
            e.rowptr = A->rowptr;
            e.colidx = A->colidx;
            e.vals = A->vals;
            e.x = d_x[sp.first + q];
            e.y = d_y[sp.first + q];
            e.partials = (void *)((char *)b->d_mem + sp.off_p[q]);  // this member's own
            e.cidx = (const unsigned short *)((char *)b->d_mem + sp.off_16[q]);
            e.runs = (const int *)((char *)b->d_mem + sp.off_r[q]);
            e.cmax = A->cols > 0 ? (int)(A->cols - 1) : 0;
            e.nnz = A->nnz_s;
            e.vector_ok = ((((uintptr_t)A->colidx) | ((uintptr_t)A->vals)) & 15) == 0;
            memcpy(host.data() + sp.off_e + (size_t)q * sizeof(e), &e, sizeof(e));
            a.tiles_at.begin[q] = nt;
            a.longs_at.begin[q] = nl;
            for (int t = t0; t < t1; t++)
                if (p.cbase[(size_t)t] != -1) b->entries_16bit += p.blocks[(size_t)t].k1 - p.blocks[(size_t)t].k0;
            b->tiles += t1 - t0;
            if (t1 > t0) {
                memcpy(host.data() + sp.off_t + (size_t)nt * sizeof(SpmvBlock), p.blocks.data() + t0,
                       (size_t)(t1 - t0) * sizeof(SpmvBlock));
                memcpy(host.data() + sp.off_c + (size_t)nt * sizeof(int), p.cbase.data() + t0,
                       (size_t)(t1 - t0) * sizeof(int));
                memcpy(host.data() + sp.off_k + (size_t)nt * sizeof(int), p.poff.data() + t0,
                       (size_t)(t1 - t0) * sizeof(int));
            }
            if (nlq > 0)
                memcpy(host.data() + sp.off_l + (size_t)nl * sizeof(SpmvLongRow), p.longrows.data(),
                       (size_t)nlq * sizeof(SpmvLongRow));
            if (!p.c16.empty())
                memcpy(host.data() + sp.off_16[q], p.c16.data(), p.c16.size() * sizeof(uint16_t));
            if (!p.runs.empty())
                memcpy(host.data() + sp.off_r[q], p.runs.data(), p.runs.size() * sizeof(int));
            nt += t1 - t0;
            nl += nlq;
        }
        a.tiles_at.begin[sp.count] = nt;
        a.longs_at.begin[sp.count] = nl;
        b->launches.push_back(a);
    }
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

// A packed record's geometry for `type`: vector width, slot-field words.
static void pack_geometry(rsp_datatype_t type, int *vw, int *iw) {
    *vw = type == RSP_R_64F ? SpmvTile<double>::kVec : SpmvTile<float>::kVec;
    *iw = rsp_pack::index_words(rsp::kSpmvThreads, rsp::kSpmvIter * *vw);
}

// rsp_spmv_plan_stats: what one call over the schedule of a host pattern
// reads besides the values, x and y (see include/rsp.h for the rule).
static rsp_status_t spmv_plan_stats(int m, const int *rp, const int *ci, int64_t nnz, rsp_datatype_t type,
                                    int64_t *out) {
    if (m < 0 || (m > 0 && (!rp || !ci)) || !out) return RSP_STATUS_INVALID_VALUE;
    if (type != RSP_R_64F && type != RSP_R_32F) return RSP_STATUS_NOT_SUPPORTED;
    TilePlan p;
    make_tile_plan(rp, ci, m, nnz, type, 0, -1, true, p);
    int vw, iw;
    pack_geometry(type, &vw, &iw);
    int64_t staged = 0, idx = 0, desc = 0, rows16 = 0, rowptr = 0;
    for (size_t t = 0; t < p.blocks.size(); t++) {
        const SpmvBlock &b = p.blocks[t];
        const int cb = p.cbase[t], po = p.poff[t];
        const int64_t len = b.k1 - b.k0, nrows = b.r1 > b.r0 ? b.r1 - b.r0 : 0;
        idx += po >= 0 ? 4LL * iw : cb == -1 ? 4 * len : 2 * len;
        if (cb <= -2) {
            const int code = -2 - cb, nr = code & 255;
            staged++;
            desc += nr == 255 ? 8 + 2LL * p.runs[2 * (size_t)(code >> 8) + 1] : 8LL * (nr + 1);
        }
        if (po >= 0 && (po & 1))
            rows16 += 4LL * rsp_pack::row_words((int)nrows);
        else
            rowptr += 4 * (nrows + 1);
    }
    out[0] = (int64_t)p.blocks.size();
    out[1] = p.tiles_packed;
    out[2] = p.nnz_packed;
    out[3] = 24 * (int64_t)p.blocks.size() + idx + desc + rows16;
    out[4] = rowptr;
    out[5] = staged;
    out[6] = idx;
    out[7] = rows16;
    return RSP_STATUS_SUCCESS;
}

// rsp_spmv_plan_host: the schedule of a host pattern, every 16-bit / staged
// column decoded back and compared with the pattern; a packed tile's slots
// are read from its record's fields, whose padding must be 0, and its packed
// row offsets are compared with the row offsets.
static rsp_status_t spmv_plan_host(int m, const int *rp, const int *ci, int64_t nnz, rsp_datatype_t type,
                                   int64_t *tiles, int64_t *e16, int64_t *est) {
    if (m < 0 || (m > 0 && (!rp || !ci)) || !tiles || !e16 || !est) return RSP_STATUS_INVALID_VALUE;
    if (type != RSP_R_64F && type != RSP_R_32F) return RSP_STATUS_NOT_SUPPORTED;
    TilePlan p;
    make_tile_plan(rp, ci, m, nnz, type, 0, -1, true, p);
    const int ucap = type == RSP_R_64F ? SpmvTile<double>::kStageSlots : SpmvTile<float>::kStageSlots;
    int vw, iw;
    pack_geometry(type, &vw, &iw);
    const int pack_mode = spmv_pack_mode();
    if (p.poff.size() != p.blocks.size()) return RSP_STATUS_INTERNAL_ERROR;
    int64_t npk = 0, epk = 0;
    for (size_t t = 0; t < p.blocks.size(); t++) {
        const SpmvBlock &b = p.blocks[t];
        const int cb = p.cbase[t], po = p.poff[t];
        const uint32_t *rec = nullptr;
        if (po >= 0) {  // the record: a staged, eligible tile; inside `runs`, after the descriptors
            const int nrows = b.r1 - b.r0, kb = b.k0 & ~(vw - 1);
            const size_t w0 = (size_t)(po >> 1), words = (size_t)iw + ((po & 1) ? rsp_pack::row_words(nrows) : 0);
            if (cb > -2 || b.r1 < 0 || pack_mode == 0 || (po & 1) != (pack_mode >= 2) ||
                !rsp_pack::eligible(rsp::kSpmvThreads, rsp::kSpmvIter * vw, b.k1 - b.k0) || (w0 & 3) ||
                w0 + words > p.runs.size())
                return RSP_STATUS_INTERNAL_ERROR;
            rec = reinterpret_cast<const uint32_t *>(p.runs.data()) + w0;
            const int nwt = iw / rsp::kSpmvThreads;
            for (int tid = 0; tid < rsp::kSpmvThreads; tid++)  // fields outside [k0, k1) are 0
                for (int f = 0; f < rsp::kSpmvIter * vw; f++) {
                    const long long e = (long long)kb + (long long)((f / vw) * rsp::kSpmvThreads + tid) * vw + f % vw;
                    if ((e < b.k0 || e >= b.k1) && rsp_pack::get_field(rec + (size_t)tid * nwt, f) != 0)
                        return RSP_STATUS_INTERNAL_ERROR;
                }
            if (po & 1)
                for (int i = 0; i <= nrows; i++)
                    if (rsp_pack::unpack_row(rec + iw, i) + kb != rp[b.r0 + i]) return RSP_STATUS_INTERNAL_ERROR;
            npk++;
            epk += b.k1 - b.k0;
        }
        auto slot_of = [&](int k) {
            return rec ? (int)rsp_pack::unpack_slot(rec, b.k0, k, vw, rsp::kSpmvIter, rsp::kSpmvThreads)
                       : (int)p.c16[(size_t)k];
        };
        if (cb == -1) continue;
        for (int k = b.k0; k < b.k1; k++) {
            int col;
            if (cb >= 0) {
                col = cb + p.c16[(size_t)k];
            } else {
                const int code = -2 - cb, nr = code & 255, off = code >> 8;
                if (nr == 255) {  // list mode (fp64): {base, U}, then U uint16 offsets
                    if (type != RSP_R_64F) return RSP_STATUS_INTERNAL_ERROR;
                    if ((size_t)2 * off + 2 > p.runs.size()) return RSP_STATUS_INTERNAL_ERROR;
                    const int *r = p.runs.data() + 2 * (size_t)off;
                    const int U = r[1];
                    if (U < 1 || U > ucap || (size_t)2 * off + 2 + 2 * (size_t)((U + 3) / 4) > p.runs.size())
                        return RSP_STATUS_INTERNAL_ERROR;
                    const uint16_t *o = reinterpret_cast<const uint16_t *>(r + 2);
                    for (int u = 1; u < U; u++)
                        if (o[u] <= o[u - 1]) return RSP_STATUS_INTERNAL_ERROR;
                    const int u = slot_of(k);
                    if (u >= U) return RSP_STATUS_INTERNAL_ERROR;
                    if (r[0] + o[u] != ci[k]) return RSP_STATUS_INTERNAL_ERROR;
                    continue;
                }
                if (nr < 1 || nr > rsp::kStageRuns || (size_t)2 * (off + nr + 1) > p.runs.size())
                    return RSP_STATUS_INTERNAL_ERROR;
                const int *r = p.runs.data() + 2 * (size_t)off;
                const int U = r[2 * nr + 1];
                if (r[1] != 0 || U > ucap) return RSP_STATUS_INTERNAL_ERROR;
                for (int j = 1; j <= nr; j++)
                    if (r[2 * j + 1] <= r[2 * j - 1] || (j < nr && r[2 * j] <= r[2 * j - 2] + (r[2 * j + 1] - r[2 * j - 1]) - 1))
                        return RSP_STATUS_INTERNAL_ERROR;
                const int u = slot_of(k);
                if (u >= U) return RSP_STATUS_INTERNAL_ERROR;
                int j = 0;
                while (j + 1 < nr && r[2 * (j + 1) + 1] <= u) j++;
                col = r[2 * j] + (u - r[2 * j + 1]);
            }
            if (col != ci[k]) return RSP_STATUS_INTERNAL_ERROR;
        }
    }
    if (npk != p.tiles_packed || epk != p.nnz_packed) return RSP_STATUS_INTERNAL_ERROR;
    *tiles = (int64_t)p.blocks.size();
    *e16 = p.nnz_c16;
    *est = p.nnz_staged;
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
        if (op != RSP_OPERATION_NON_TRANSPOSE) return RSP_STATUS_NOT_SUPPORTED;
        if (compute_type != mat->type) return RSP_STATUS_INVALID_VALUE;
        return spmv_plan(h, mat, compute_type);  // explicit request: always re-plan
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

rsp_status_t rsp_spmv_plan_host(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                rsp_datatype_t compute_type, int64_t *tiles, int64_t *entries_16bit,
                                int64_t *entries_staged) {
    return guarded([&] {
        return spmv_plan_host(m, row_offsets, col_ind, nnz, compute_type, tiles, entries_16bit, entries_staged);
    });
}

rsp_status_t rsp_spmv_plan_stats(int m, const int *row_offsets, const int *col_ind, int64_t nnz,
                                 rsp_datatype_t compute_type, int64_t stats[8]) {
    return guarded([&] { return spmv_plan_stats(m, row_offsets, col_ind, nnz, compute_type, stats); });
}

}  // the C ABI
