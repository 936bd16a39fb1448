// spmv_plan.cpp — the SpMV planner (spmv_plan.h): row packing, the column
// encoding of every tile, the packed records, and the plan's statistics,
// verifier and digest. No HIP calls here.

#include "spmv_plan.h"
#include "spmv_pack.h"

#include <algorithm>
#include <atomic>
#include <vector>

namespace rsp_plan {

using rsp::SpmvTile;

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Tile geometry of a compute type (rsp_kernels.h SpmvTile<T>).
struct TileGeom {
    int cap, chunk, maxrows;  // entries per tile, per long-row chunk; rows per tile
    int ucap;                 // distinct columns of a staged tile, at most
    bool list;                // list-staged tiles exist for this type
    int vw, iw;               // a packed record's vector width and slot-field words
    int xelem;                // bytes per x element
};
template <typename T>
TileGeom geom_of() {
    using S = SpmvTile<T>;
    return {S::kMaxNnz, S::kChunk, S::kMaxRows, S::kStageSlots, S::kStageList, S::kVec,
            rsp_pack::index_words(rsp::kSpmvThreads, rsp::kSpmvIter * S::kVec), (int)sizeof(T)};
}
TileGeom geom(rsp_datatype_t t) { return t == RSP_R_64F ? geom_of<double>() : geom_of<float>(); }

SpmvBounds spmv_bounds(int64_t rows, int64_t nnz, int cap) {
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

}  // namespace

SpmvLayout spmv_layout(const SpmvBounds &b, size_t elem, int64_t nnz, size_t run_ints) {
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

PlanOptions plan_options(rsp_datatype_t type) {
    using rsp_an::env_int;
    PlanOptions o;
    o.type = type;
    o.stage_list = env_int("RSP_SPMV_STAGE_LIST", 1);
    o.list_cap = env_int("RSP_SPMV_LIST_CAP", o.list_cap);
    o.stage_pct = std::min(std::max(env_int("RSP_SPMV_STAGE_PCT", 80), 0), 100);
    o.pack_mode = std::min(std::max(env_int("RSP_SPMV_PACK", 2), 0), 2);
    return o;
}

// Greedy row-block schedule over host row offsets (see spmv.hip header).
// Rows longer than kSpmvLongRow get tiles of their own (one per `chunk`
// entries); the others are packed into tiles of <= cap entries / maxrows rows.
RowPlan build_spmv_plan(const int *rp, int m, int cap, int chunk, int maxrows, int row_align) {
    RowPlan out;
    hvec<SpmvBlock> &blocks = out.blocks;
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
            out.longrows.push_back(lr);
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
    out.nslots = slots;
    return out;
}

namespace {

RowPlan pack_rows(const int *rp, int m, int cap, const TileGeom &g, const PlanOptions &o) {
    return build_spmv_plan(rp, m, cap, g.chunk, g.maxrows, o.row_align);
}

// spread > 0: a plan of fewer tiles than `spread` (the resident workgroup
// slots it may use) is re-packed into up to `spread` smaller tiles, so a lone
// launch does not leave slots idle. Long rows do not depend on the packing
// cap (they are cut at the fixed chunk), so every spread of one matrix has
// the same long rows and partial slots.
void respread(const int *rp, int m, int64_t nnz_bound, const TileGeom &g, const PlanOptions &o, RowPlan &p) {
    const SpmvBounds bb = spmv_bounds(m, std::max<int64_t>(nnz_bound, 0), g.chunk);
    const int64_t nnz_s = rp[(size_t)m];
    int c = (int)std::max<int64_t>(64, std::min<int64_t>(g.cap, (nnz_s + o.spread - 1) / o.spread));
    for (int tries = 0; tries < 32 && c < g.cap; tries++) {
        RowPlan p2 = pack_rows(rp, m, c, g, o);
        if ((int64_t)p2.blocks.size() <= o.spread && p2.blocks.size() <= bb.nblocks) {
            p = std::move(p2);
            break;
        }
        c += std::max(8, c / 16);
    }
}

// The sorted distinct columns of entries [k0, k1) (k1 > k0) into `cols`;
// returns the number of contiguous column runs they form.
int distinct_cols(const int *ci, int k0, int k1, std::vector<int> &cols) {
    cols.assign(ci + k0, ci + k1);
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    int R = 1;
    for (size_t u = 1; u < cols.size(); u++) R += cols[u] != cols[u - 1] + 1;
    return R;
}

bool list_tiles_ok(const TileGeom &g, const PlanOptions &o) {
    return o.use_stage && o.use_c16 && g.list && o.stage_list != 0;
}

// Random-band matrices (round 4): tiles whose columns lie in a band
// narrower than 65536 but scattered over it (more runs than a staged
// tile's run table holds) are staged by an explicit column LIST instead
// (encode_columns); that needs at most kStageSlots distinct columns per tile,
// so such a matrix is re-packed with tiles of at most kStageSlots entries
// (the canonical summation order does not depend on the packing). Judged
// on a sample of 64 tiles; not for spread plans (already small tiles).
void list_repack(const int *rp, const int *ci, int m, const TileGeom &g, const PlanOptions &o, RowPlan &p) {
    int64_t band = 0, all = 0;
    std::vector<int> cols;
    const size_t step = std::max<size_t>(1, p.blocks.size() / 64);
    for (size_t t = 0; t < p.blocks.size(); t += step) {
        const SpmvBlock &bk = p.blocks[t];
        if (bk.r1 < 0 || bk.k1 <= bk.k0) continue;
        const int R = distinct_cols(ci, bk.k0, bk.k1, cols);
        all += bk.k1 - bk.k0;
        if (cols.back() - cols.front() <= 65535 && R > rsp::kStageRuns && (int)cols.size() > g.ucap)
            band += bk.k1 - bk.k0;
    }
    if (2 * band > all) p = pack_rows(rp, m, std::min(g.cap, std::min(std::max(o.list_cap, 64), g.ucap)), g, o);
}

// split schedule (rsp_spmat_set_local_cols): tiles reading own columns
// only first; long-row tiles always in the second part (with the fixup)
bool interior_tile(const SpmvBlock &b, const int *ci, int64_t local_cols) {
    if (b.r1 < 0) return false;
    for (int k = b.k0; k < b.k1; k++)
        if (ci[(size_t)k] >= local_cols) return false;
    return true;
}
int partition_interior(const int *ci, int64_t local_cols, hvec<SpmvBlock> &blocks) {
    auto mid = std::stable_partition(blocks.begin(), blocks.end(),
                                     [&](const SpmvBlock &b) { return interior_tile(b, ci, local_cols); });
    return (int)(mid - blocks.begin());
}

// How a tile of >= 1 entries reads its columns. `lo`: its smallest column;
// Runs / List: `cols` holds its sorted distinct columns, `R` their runs.
enum class TileKind { Int32, Gather16, Runs, List };
TileKind classify_tile(const SpmvBlock &bk, const int *ci, const TileGeom &g, const PlanOptions &o,
                       std::vector<int> &cols, int *lo_out, int *R_out) {
    int lo = ci[(size_t)bk.k0], hi = lo;
    for (int k = bk.k0 + 1; k < bk.k1; k++) {
        lo = std::min(lo, ci[(size_t)k]);
        hi = std::max(hi, ci[(size_t)k]);
    }
    *lo_out = lo;
    if (hi - lo > 65535) return TileKind::Int32;
    // staged x loads use 32-bit byte offsets into a buffer resource of
    // 0x7ffffffc bytes (spmv.hip stream_products_staged): a tile whose
    // columns reach past that keeps the plain 16-bit offsets
    const bool x_in_rsrc = ((int64_t)hi + 1) * g.xelem <= (int64_t)0x7ffffffc;
    if (!o.use_stage || bk.r1 < 0 || !x_in_rsrc) return TileKind::Gather16;  // (long-row chunks keep the offsets)
    const int len = bk.k1 - bk.k0;
    const int R = *R_out = distinct_cols(ci, bk.k0, bk.k1, cols);
    const int U = (int)cols.size();
    if (U <= g.ucap && R <= rsp::kStageRuns && 100LL * U <= (long long)o.stage_pct * len) return TileKind::Runs;
    if (list_tiles_ok(g, o) && U <= g.ucap && R > rsp::kStageRuns) return TileKind::List;
    return TileKind::Gather16;
}

// 16-bit column offsets: a tile whose columns span < 65536 reads
// col = cbase + off (2 B per entry instead of 4; the int32 colidx is not
// read for it). Staged tiles (round 4, spmv.hip stream_products_staged):
// where the tile's distinct columns are few (at most kStageSlots, at most
// RSP_SPMV_STAGE_PCT % of its entries, default 80) in at most kStageRuns
// contiguous runs, its 16-bit values are instead the entries' slots in the
// sorted list of those columns, and the runs ({first column, first slot},
// then {0, slots}) go to `runs`. Tiles are planned in parallel.
void encode_columns(const int *ci, int64_t nnz_s, const TileGeom &g, const PlanOptions &o, TilePlan &p) {
    p.c16.assign((size_t)nnz_s, 0);
    const long long nt = (long long)p.blocks.size();
    std::vector<std::vector<int>> truns(o.use_stage ? (size_t)nt : 0);
    std::vector<char> tlist(o.use_stage ? (size_t)nt : 0, 0);
    std::atomic<int64_t> n16{0}, nst{0};
    rsp_an::parallel_for(nt, 64, [&](long long t0, long long t1) {
        std::vector<int> cols;
        int64_t c16n = 0, stn = 0;
        for (long long t = t0; t < t1; t++) {
            const SpmvBlock &bk = p.blocks[(size_t)t];
            if (bk.k1 <= bk.k0) continue;
            int lo = 0, R = 0;
            const TileKind kind = classify_tile(bk, ci, g, o, cols, &lo, &R);
            if (kind == TileKind::Int32) continue;
            const int len = bk.k1 - bk.k0;
            c16n += len;
            if (kind == TileKind::Gather16) {
                p.cbase[(size_t)t] = lo;
                for (int k = bk.k0; k < bk.k1; k++) p.c16[(size_t)k] = (uint16_t)(ci[(size_t)k] - lo);
                continue;
            }
            const int U = (int)cols.size();
            std::vector<int> &r = truns[(size_t)t];
            tlist[(size_t)t] = kind == TileKind::List;
            if (kind == TileKind::Runs) {
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
                uint16_t *ofs = reinterpret_cast<uint16_t *>(r.data() + 2);
                for (int u = 0; u < U; u++) ofs[u] = (uint16_t)(cols[(size_t)u] - cols[0]);
            }
            for (int k = bk.k0; k < bk.k1; k++)
                p.c16[(size_t)k] =
                    (uint16_t)(std::lower_bound(cols.begin(), cols.end(), ci[(size_t)k]) - cols.begin());
            stn += len;
        }
        n16 += c16n;
        nst += stn;
    });
    p.nnz_c16 = n16;
    p.nnz_staged = nst;
    // descriptors concatenated in tile order
    for (size_t t = 0; t < truns.size(); t++) {
        const std::vector<int> &r = truns[t];
        if (r.empty()) continue;
        const int64_t off = (int64_t)p.runs.size() / 2;
        if (off >= kStageOffLimit) {  // (encoding range; never reached on real matrices)
            p.nnz_c16 -= p.blocks[t].k1 - p.blocks[t].k0;
            p.nnz_staged -= p.blocks[t].k1 - p.blocks[t].k0;
            continue;  // cbase stays kCbaseInt32
        }
        // runs mode: descriptors + sentinel; list mode: header {base, U} + offsets
        p.cbase[t] = stage_encode(off, tlist[t] ? kStageListCode : (int)r.size() / 2 - 1);
        p.runs.insert(p.runs.end(), r.begin(), r.end());
    }
}

// Packed records (spmv_pack.h) of the staged tiles whose slot fields are
// strictly fewer bytes than their 16-bit words, appended to p.runs after every
// run descriptor (whose offsets have the smaller range), each 16-B aligned.
// An offset past the encoding's range leaves the tile unpacked.
void pack_staged_tiles(const int *rp, const TileGeom &g, int mode, TilePlan &p) {
    constexpr int IT = rsp::kSpmvIter, NTH = rsp::kSpmvThreads;
    const int VW = g.vw, IW = g.iw;
    if (mode <= 0) return;
    int64_t end = ((int64_t)p.runs.size() + 3) & ~(int64_t)3;
    for (size_t t = 0; t < p.blocks.size(); t++) {
        const SpmvBlock &b = p.blocks[t];
        if (!staged(p.cbase[t]) || b.r1 < 0 || !rsp_pack::eligible(NTH, IT * VW, b.k1 - b.k0)) continue;
        const int64_t words = IW + (mode >= 2 ? rsp_pack::row_words(b.r1 - b.r0) : 0);
        if (end + words >= kPackWordLimit) break;  // (never reached on real matrices)
        p.poff[t] = pack_encode(end, mode >= 2);
        end = (end + words + 3) & ~(int64_t)3;
        p.tiles_packed++;
        p.nnz_packed += b.k1 - b.k0;
    }
    if (p.tiles_packed == 0) return;
    p.runs.resize((size_t)end + 4, 0);  // (+ 16 B: a vector load of a record's last words stays inside)
    rsp_an::parallel_for((long long)p.blocks.size(), 64, [&](long long t0, long long t1) {
        for (long long t = t0; t < t1; t++) {
            if (p.poff[(size_t)t] == kNoPack) continue;
            const SpmvBlock &b = p.blocks[(size_t)t];
            const PackCode pc = pack_decode(p.poff[(size_t)t]);
            uint32_t *rec = reinterpret_cast<uint32_t *>(p.runs.data()) + pc.word;
            rsp_pack::pack_slots(p.c16.data(), b.k0, b.k1, VW, IT, NTH, rec);
            if (pc.rows) rsp_pack::pack_rows(rp, b.r0, b.r1 - b.r0, b.k0 & ~(VW - 1), rec + IW);
        }
    });
}

}  // namespace

void make_tile_plan(const int *rp, const int *ci, int m, int64_t nnz_bound, const PlanOptions &o, TilePlan &p) {
    const TileGeom g = geom(o.type);
    RowPlan &rows = p;
    rows = pack_rows(rp, m, g.cap, g, o);
    const size_t nb = p.blocks.size();
    if (o.spread > 0 && nb > 0 && (int64_t)nb < o.spread) respread(rp, m, nnz_bound, g, o, rows);
    if (list_tiles_ok(g, o) && p.blocks.size() == nb && nb > 0) list_repack(rp, ci, m, g, o, rows);
    p.nint = o.local_cols >= 0 ? partition_interior(ci, o.local_cols, p.blocks) : 0;
    const int64_t nnz_s = m > 0 ? rp[(size_t)m] : 0;
    p.cbase.assign(p.blocks.size(), kCbaseInt32);
    p.c16.clear();
    p.runs.clear();
    p.poff.assign(p.blocks.size(), kNoPack);
    p.tiles_packed = p.nnz_packed = 0;
    p.nnz_c16 = 0;
    p.nnz_staged = 0;
    if (o.use_c16 && nnz_s > 0 && nnz_s <= nnz_bound) {
        encode_columns(ci, nnz_s, g, o, p);
        if (o.use_stage) pack_staged_tiles(rp, g, o.pack_mode, p);
    }
}

void plan_stats(const TilePlan &p, rsp_datatype_t type, int64_t out[8]) {
    const TileGeom g = geom(type);
    int64_t nstaged = 0, idx = 0, desc = 0, rows16 = 0, rowptr = 0;
    for (size_t t = 0; t < p.blocks.size(); t++) {
        const SpmvBlock &b = p.blocks[t];
        const int cb = p.cbase[t], po = p.poff[t];
        const int64_t len = b.k1 - b.k0, nrows = b.r1 > b.r0 ? b.r1 - b.r0 : 0;
        idx += po != kNoPack ? 4LL * g.iw : cb == kCbaseInt32 ? 4 * len : 2 * len;
        if (staged(cb)) {
            const StageCode sc = stage_decode(cb);
            nstaged++;
            desc += sc.list() ? 8 + 2LL * p.runs[2 * (size_t)sc.off + 1] : 8LL * (sc.nr + 1);
        }
        if (po != kNoPack && pack_decode(po).rows)
            rows16 += 4LL * rsp_pack::row_words((int)nrows);
        else
            rowptr += 4 * (nrows + 1);
    }
    out[0] = (int64_t)p.blocks.size();
    out[1] = p.tiles_packed;
    out[2] = p.nnz_packed;
    out[3] = 24 * (int64_t)p.blocks.size() + idx + desc + rows16;
    out[4] = rowptr;
    out[5] = nstaged;
    out[6] = idx;
    out[7] = rows16;
}

void tile_facts(const TilePlan &p, size_t t, int64_t out[RSP_SPMV_TILE_FACTS]) {
    const SpmvBlock &b = p.blocks[t];
    const int cb = p.cbase[t], po = p.poff[t];
    int64_t kind = 0, base = 0, U = 0, R = 0;
    if (staged(cb)) {
        const StageCode sc = stage_decode(cb);
        const int *r = p.runs.data() + 2 * (size_t)sc.off;
        base = r[0];
        if (sc.list()) {  // R: the runs its listed columns form
            const uint16_t *ofs = reinterpret_cast<const uint16_t *>(r + 2);
            kind = 3;
            U = r[1];
            R = 1;
            for (int u = 1; u < U; u++) R += ofs[u] != ofs[u - 1] + 1;
        } else {
            kind = 2;
            U = r[2 * sc.nr + 1];
            R = sc.nr;
        }
    } else if (cb != kCbaseInt32) {
        kind = 1;
        base = cb;
    }
    const int64_t f[RSP_SPMV_TILE_FACTS] = {b.r0, b.r1, b.k0, b.k1, kind, base, U, R, po != kNoPack,
                                            po != kNoPack && pack_decode(po).rows};
    std::copy(f, f + RSP_SPMV_TILE_FACTS, out);
}

namespace {

// The split schedule as `o` asks for it: tiles [0, nint) are interior, tile
// nint is not, and both parts keep the packing's ascending (r0, k0) order (the
// partition is stable).
bool verify_split(const int *ci, const PlanOptions &o, const TilePlan &p) {
    const size_t nt = p.blocks.size(), nint = (size_t)p.nint;
    if (p.nint < 0 || nint > nt || (o.local_cols < 0 && nint != 0)) return false;
    for (size_t t = 0; t < nt; t++) {
        const SpmvBlock &b = p.blocks[t];
        if (o.local_cols >= 0 && t <= nint && interior_tile(b, ci, o.local_cols) != (t < nint)) return false;
        if (t == 0 || t == nint) continue;
        const SpmvBlock &a = p.blocks[t - 1];
        if (a.r0 > b.r0 || (a.r0 == b.r0 && a.k0 >= b.k0)) return false;
    }
    return true;
}

}  // namespace

bool plan_verify(const int *rp, const int *ci, int m, const PlanOptions &o, const TilePlan &p) {
    const TileGeom g = geom(o.type);
    const int vw = g.vw, iw = g.iw;
    const int nnz_s = m > 0 ? rp[m] : 0;
    if (p.poff.size() != p.blocks.size() || p.cbase.size() != p.blocks.size()) return false;
    if (!p.c16.empty() && p.c16.size() != (size_t)nnz_s) return false;
    int64_t npk = 0, epk = 0;
    for (size_t t = 0; t < p.blocks.size(); t++) {
        const SpmvBlock &b = p.blocks[t];
        const int cb = p.cbase[t], po = p.poff[t];
        // rows and entries of the pattern; 16-bit entries only where the 16-bit array is
        if (b.r0 < 0 || b.r0 >= m || (b.r1 >= 0 && (b.r1 < b.r0 || b.r1 > m))) return false;
        if (b.k0 < 0 || b.k1 < b.k0 || b.k1 > nnz_s) return false;
        if (cb != kCbaseInt32 && p.c16.empty() && b.k1 > b.k0) return false;
        if (!o.use_c16 && cb != kCbaseInt32) return false;
        if (!o.use_stage && (staged(cb) || po != kNoPack)) return false;
        const uint32_t *rec = nullptr;
        if (po != kNoPack) {  // the record: a staged, eligible tile; inside `runs`, after the descriptors
            const PackCode pc = pack_decode(po);
            const int nrows = b.r1 - b.r0, kb = b.k0 & ~(vw - 1);
            const size_t words = (size_t)iw + (pc.rows ? rsp_pack::row_words(nrows) : 0);
            if (po < 0 || !staged(cb) || b.r1 < 0 || o.pack_mode == 0 || pc.rows != (o.pack_mode >= 2) ||
                !rsp_pack::eligible(rsp::kSpmvThreads, rsp::kSpmvIter * vw, b.k1 - b.k0) || (pc.word & 3) ||
                pc.word + words > p.runs.size())
                return false;
            rec = reinterpret_cast<const uint32_t *>(p.runs.data()) + pc.word;
            const int nwt = iw / rsp::kSpmvThreads;
            for (int tid = 0; tid < rsp::kSpmvThreads; tid++)  // fields outside [k0, k1) are 0
                for (int f = 0; f < rsp::kSpmvIter * vw; f++) {
                    const long long e = (long long)kb + (long long)((f / vw) * rsp::kSpmvThreads + tid) * vw + f % vw;
                    if ((e < b.k0 || e >= b.k1) && rsp_pack::get_field(rec + (size_t)tid * nwt, f) != 0) return false;
                }
            if (pc.rows)
                for (int i = 0; i <= nrows; i++)
                    if (rsp_pack::unpack_row(rec + iw, i) + kb != rp[b.r0 + i]) return false;
            npk++;
            epk += b.k1 - b.k0;
        }
        auto slot_of = [&](int k) {
            return rec ? (int)rsp_pack::unpack_slot(rec, b.k0, k, vw, rsp::kSpmvIter, rsp::kSpmvThreads)
                       : (int)p.c16[(size_t)k];
        };
        if (cb == kCbaseInt32 || b.k1 <= b.k0) continue;
        // a staged tile's descriptors, checked once: r, its U slots, the list's offsets
        const StageCode sc = staged(cb) ? stage_decode(cb) : StageCode{0, 0};
        const int off = sc.off, nr = sc.nr;
        const int *r = nullptr;
        const uint16_t *ofs = nullptr;
        int U = 0;
        if (staged(cb) && sc.list()) {  // list mode (fp64): {base, U}, then U uint16 offsets
            if (o.type != RSP_R_64F) return false;
            if ((size_t)2 * off + 2 > p.runs.size()) return false;
            r = p.runs.data() + 2 * (size_t)off;
            U = r[1];
            if (U < 1 || U > g.ucap || (size_t)2 * off + 2 + 2 * (size_t)((U + 3) / 4) > p.runs.size()) return false;
            ofs = reinterpret_cast<const uint16_t *>(r + 2);
            for (int u = 1; u < U; u++)
                if (ofs[u] <= ofs[u - 1]) return false;
        } else if (staged(cb)) {
            if (nr < 1 || nr > rsp::kStageRuns || (size_t)2 * (off + nr + 1) > p.runs.size()) return false;
            r = p.runs.data() + 2 * (size_t)off;
            U = r[2 * nr + 1];
            if (r[1] != 0 || U > g.ucap) return false;
            for (int j = 1; j <= nr; j++)
                if (r[2 * j + 1] <= r[2 * j - 1] ||
                    (j < nr && r[2 * j] <= r[2 * j - 2] + (r[2 * j + 1] - r[2 * j - 1]) - 1))
                    return false;
        }
        // a staged tile loads x for every slot below U: each is some entry's
        // (a U that is too large would read a column no entry names)
        std::vector<char> used(staged(cb) ? (size_t)std::max(U, 0) : 0, 0);
        for (int k = b.k0; k < b.k1; k++) {
            int col;
            if (cb >= 0) {
                col = cb + p.c16[(size_t)k];
            } else {
                const int u = slot_of(k);
                if (u >= U || (rec && p.c16[(size_t)k] != u)) return false;  // (the record repeats the 16-bit slots)
                used[(size_t)u] = 1;
                int j = 0;
                while (!ofs && j + 1 < nr && r[2 * (j + 1) + 1] <= u) j++;
                col = ofs ? r[0] + ofs[u] : r[2 * j] + (u - r[2 * j + 1]);
            }
            if (col != ci[k]) return false;
        }
        if (std::find(used.begin(), used.end(), 0) != used.end()) return false;
    }
    return npk == p.tiles_packed && epk == p.nnz_packed && verify_split(ci, o, p);
}

uint64_t digest(const TilePlan &p) {
    rsp_an::Fnv f;
    f.vec(p.blocks);
    f.vec(p.longrows);
    f.bytes(&p.nslots, sizeof(p.nslots));
    f.bytes(&p.nint, sizeof(p.nint));
    f.vec(p.cbase);
    f.vec(p.c16);
    f.vec(p.runs);
    f.vec(p.poff);
    for (const int64_t c : {p.nnz_c16, p.nnz_staged, p.tiles_packed, p.nnz_packed}) f.bytes(&c, sizeof(c));
    return f.h;
}

}  // namespace rsp_plan
