// spmv_plan.h — the host-side row-block schedule of SpMV (see spmv.hip
// header): tiles, long rows, per-tile column codes, 16-bit column offsets,
// staged tiles' runs and packed records, and the layout of all that in the
// matrix's device memory. Pure host C++ (no HIP calls): rsp_api.cpp downloads
// the pattern, calls make_tile_plan and uploads the result; rsp_spmv_plan_host,
// rsp_spmv_plan_tiles_host and rsp_spmv_plan_stats run it on host arrays; drivers/spmv_plan_check.cpp
// runs it under the sanitizers (make tsan-plan / asan-plan).
#ifndef RSP_SPMV_PLAN_H
#define RSP_SPMV_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "rsp.h"
#include "host_pool.h"
#include "rsp_kernels.h"

namespace rsp_plan {

using rsp::SpmvBlock;
using rsp::SpmvLongRow;
using rsp_an::hvec;

/* The two per-tile codes. The planner, plan_stats and plan_verify read and
 * write them through these helpers only; the kernels keep their own decode
 * (spmv.hip; the codes are described at rsp::SpmvArgs::cbases / poffs in
 * rsp_kernels.h, which points back here). */

// cbase (SpmvArgs::cbases): >= 0 the column base of a tile's 16-bit offsets,
// kCbaseInt32 a tile on the int32 colidx, <= -2 a STAGED tile: pair offset
// `off` of its descriptors in `runs` (< kStageOffLimit) and `nr`, the number
// of run descriptors before the sentinel, or kStageListCode: a column list.
constexpr int kCbaseInt32 = -1;
constexpr int kStageListCode = 255;
constexpr int64_t kStageOffLimit = 1LL << 22;
struct StageCode {
    int off, nr;
    bool list() const { return nr == kStageListCode; }
};
inline bool staged(int cbase) { return cbase <= -2; }
inline int stage_encode(int64_t off, int nr) { return -2 - (int)((off << 8) | nr); }
inline StageCode stage_decode(int cbase) { return {(-2 - cbase) >> 8, (-2 - cbase) & 255}; }

// poff (SpmvArgs::poffs): kNoPack, or a staged tile's packed record
// (spmv_pack.h) at 32-bit word `word` of `runs` (< kPackWordLimit); `rows`: the
// record carries the row offsets.
constexpr int kNoPack = -1;
constexpr int64_t kPackWordLimit = 1LL << 30;
struct PackCode {
    size_t word;
    int rows;
};
inline int pack_encode(int64_t word, int rows) { return (int)(word << 1) | rows; }
inline PackCode pack_decode(int poff) { return {(size_t)(poff >> 1), poff & 1}; }

struct SpmvBounds {
    size_t nblocks, nlong, nslots;
};

// Workspace: [tiles | long rows | chunk partials | per-tile column base |
// per-tile packed-record offset | 16-bit column offsets (2 B per stored
// entry) | staged tiles' runs, then their packed records].
struct SpmvLayout {
    size_t off_long, off_part, off_cbase, off_poff, off_cidx, off_runs, bytes;
};
SpmvLayout spmv_layout(const SpmvBounds &b, size_t elem, int64_t nnz, size_t run_ints = 0);

// What a plan depends on besides the pattern. The knobs are A/B and test
// switches read from the environment at every plan (plan_options).
struct PlanOptions {
    rsp_datatype_t type = RSP_R_64F;
    int64_t spread = 0;       // > 0: the resident workgroup slots a small plan is spread over
    int64_t local_cols = -1;  // >= 0: split schedule (rsp_spmat_set_local_cols)
    int row_align = 1;        // > 1: packed tiles end on multiples of this many rows
    bool use_c16 = true;      // 16-bit column offsets (off: every tile on the int32 colidx)
    bool use_stage = true;    // staged tiles
    int stage_list = 1;       // RSP_SPMV_STAGE_LIST: 0 no list tiles
    int list_cap = 1 << 30;   // RSP_SPMV_LIST_CAP: tile size of the list re-pack (A/B), clamped to [64, kStageSlots]
    int stage_pct = 80;       // RSP_SPMV_STAGE_PCT: a staged tile's distinct columns per 100 entries, at most
    // RSP_SPMV_PACK: 0 no packed records (the unpacked plan), 1 the slot fields
    // only, 2 (default) slot fields and row offsets. On the big set's batched
    // fp64 launch: 534.8 / 530.7 / 518.8 us (profiles/r07_pack_ab.txt).
    int pack_mode = 2;
};
// The default options for `type`, the knobs as the environment has them now.
PlanOptions plan_options(rsp_datatype_t type);

// Tiles and long rows of a greedy row packing (build_spmv_plan).
struct RowPlan {
    hvec<SpmvBlock> blocks;
    hvec<SpmvLongRow> longrows;
    int nslots = 0;
};
RowPlan build_spmv_plan(const int *rp, int m, int cap, int chunk, int maxrows, int row_align);

// A complete SpMV schedule over host row offsets `rp` and column indices `ci`:
// tiles (interior tiles first when local_cols >= 0), long rows, per-tile
// column base and the 16-bit column offsets.
struct TilePlan : RowPlan {
    int nint = 0;
    hvec<int> cbase;
    hvec<uint16_t> c16;
    hvec<int> runs;  // staged tiles' run descriptors (int pairs), then the packed records; SpmvArgs::runs
    hvec<int> poff;  // per tile: packed record (SpmvArgs::poffs), kNoPack = none
    int64_t nnz_c16 = 0;     // entries not read through the int32 colidx (16-bit offsets, slot indices, packed slots)
    int64_t nnz_staged = 0;  // ... of which in staged tiles
    int64_t tiles_packed = 0, nnz_packed = 0;  // ... of which in packed tiles
};

// The schedule of m rows; nnz_bound: the entries the matrix's arrays hold (a
// pattern with more gets no 16-bit offsets).
void make_tile_plan(const int *rp, const int *ci, int m, int64_t nnz_bound, const PlanOptions &o, TilePlan &p);

// Every 16-bit / staged column of `p` decoded back and compared with the
// pattern; a packed tile's slots are read from its record's fields, whose
// padding must be 0 and whose slots must be those of the 16-bit array, and its
// packed row offsets are compared with the row offsets; every slot of a staged
// tile is some entry's; the split schedule and the switched-off codes as `o` says. `o`: the
// options `p` was made with. false: the plan is wrong.
bool plan_verify(const int *rp, const int *ci, int m, const PlanOptions &o, const TilePlan &p);

// rsp_spmv_plan_stats: what one call over the schedule reads besides the
// values, x and y (see include/rsp.h for the rule).
void plan_stats(const TilePlan &p, rsp_datatype_t type, int64_t out[8]);

// rsp_spmv_plan_tiles_host: tile t of a verified plan as RSP_SPMV_TILE_FACTS
// integers (include/rsp.h), read through stage_decode / pack_decode alone.
void tile_facts(const TilePlan &p, size_t t, int64_t out[RSP_SPMV_TILE_FACTS]);

// 64-bit digest (rsp_an::Fnv) of every array and scalar of the plan.
uint64_t digest(const TilePlan &p);

}  // namespace rsp_plan

#endif
