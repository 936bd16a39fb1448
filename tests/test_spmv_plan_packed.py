"""Packed records of staged SpMV tiles on the host (no device): 12-bit slot
fields and 16-bit row offsets (csrc/spmv_pack.h, RSP_SPMV_PACK). Every pattern
the GPU tests run (tests/test_gpu_spmv_packed.py) goes through
rsp_spmv_plan_host, which reads each packed tile's slots and row offsets back
from its record and compares them with the pattern, for both dtypes and every
knob value; rsp_spmv_plan_stats' counts are compared with a numpy recount of
the rule in include/rsp.h.

The custom surrogate specs take the TOTAL entry count as their third field
(csrc/host/surrogate.c), so 18 and 73 entries per row are written as
rows * 18 and rows * 73."""
import ctypes as C
import functools

import numpy as np
import pytest

from respasol_amd import _lib, csr
from respasol_amd.sparse import spmv_plan_stats

R64, R32 = 0, 1  # RSP_R_64F / RSP_R_32F (include/rsp.h)
THREADS, ITER = 256, 4  # rsp_kernels.h kSpmvThreads / kSpmvIter
# per dtype: vector width, tile cap (kMaxNnz), rows per tile, staged slots, packed words per thread
GEO = {R64: dict(vw=2, cap=2047, maxrows=512, ucap=1536, nw=3), R32: dict(vw=4, cap=4093, maxrows=1024, ucap=2048, nw=6)}
STAGE_RUNS = 254
STENCILS = ("stencil3d:20000:360000:S", "stencil2d:8000:584000:G")
OTHERS = ("circuit:20000:120000:G", "randband:20000:400000:G")


def band_from_lens(lens, seed=5):
    """Row i holds lens[i] consecutive columns around the diagonal."""
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=rp[1:])
    start = np.clip(np.arange(n) - lens // 2, 0, n - lens)
    ci = (np.repeat(start, lens) + (np.arange(rp[-1]) - np.repeat(rp[:-1], lens))).astype(np.int32)
    va = np.random.default_rng(seed).uniform(-1.0, 1.0, len(ci))
    return csr.CsrMatrix(0, n, n, len(ci), rp, ci, va)


@functools.lru_cache(maxsize=None)
def band_cycle(n=20000):
    """Columns within +-40 of the diagonal, row lengths cycling 1 .. 9: full
    tiles start and end inside a 16-byte vector (kb < k0)."""
    rng = np.random.default_rng(3)
    lens = 1 + np.arange(n) % 9
    off = rng.permuted(np.tile(np.arange(-40, 41), (n, 1)), axis=1)[:, :9]
    rows = [np.unique(np.clip(i + off[i, :lens[i]], 0, n - 1)) for i in range(n)]
    rp = np.zeros(n + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    ci = np.concatenate(rows).astype(np.int32)
    return csr.CsrMatrix(0, n, n, len(ci), rp, ci, rng.uniform(-1.0, 1.0, len(ci)))


def edge_lens(last, dt, rem=0):
    """Two tiles of 7-entry band rows: a filler tile, then a last tile of
    exactly `last` entries; the total entry count is `rem` modulo the vector
    width (0: the last tile takes the vector path; else the scalar path)."""
    g = GEO[dt]
    for r in range(7, 0, -1):
        filler = (g["cap"] - r) // 7 * 7 + r
        if filler + 7 > g["cap"] and (filler + last) % g["vw"] == rem:
            lens = [7] * ((filler - r) // 7) + [r] + [7] * (last // 7)
            if last % 7:
                lens.append(last % 7)
            return lens, filler
    raise AssertionError("no filler")


@functools.lru_cache(maxsize=None)
def edge_matrix(last, dt, rem=0):
    lens, filler = edge_lens(last, dt, rem)
    return band_from_lens(lens), filler


EDGE = {R64: (1536, 1537), R32: (3072, 3073)}


def plan(A, dt):
    rp = np.ascontiguousarray(A.rowptr, np.int32)
    ci = np.ascontiguousarray(A.colidx, np.int32)
    t, e16, est = C.c_int64(), C.c_int64(), C.c_int64()
    st = _lib.rsp.rsp_spmv_plan_host(A.m, rp.ctypes.data, ci.ctypes.data, int(max(A.nnz, A.nnz_stored)), dt,
                                     C.byref(t), C.byref(e16), C.byref(est))
    return st, t.value, e16.value, est.value


def stats(A, dt):
    return spmv_plan_stats(A.rowptr, A.colidx, fp32=dt == R32, nnz=int(max(A.nnz, A.nnz_stored)))


WHOLE_ROW = -2**31  # SpmvBlock::r1 of a whole long row (rsp_kernels.h kSpmvWholeRow)
XELEM = {R64: 8, R32: 4}


def greedy_cuts(rp, dt):
    """(r0, r1, k0, k1) per tile of the full-tile schedule (spmv_plan.cpp
    build_spmv_plan, row_align 1): a row of more than 256 entries is a tile of
    its own (r1 = WHOLE_ROW) or, past cap entries, one tile per cap entries
    (r1 = -(slot + 1)); the others are packed greedily."""
    g = GEO[dt]
    m, r, slot, cuts = len(rp) - 1, 0, 0, []
    while r < m:
        ln = rp[r + 1] - rp[r]
        if ln > 256:
            if ln <= g["cap"]:
                cuts.append((r, WHOLE_ROW, int(rp[r]), int(rp[r + 1])))
            else:
                for k in range(int(rp[r]), int(rp[r + 1]), g["cap"]):
                    cuts.append((r, -(slot + 1), k, min(k + g["cap"], int(rp[r + 1]))))
                    slot += 1
            r += 1
            continue
        s, nn = r, 0
        while r < m and r - s < g["maxrows"]:
            ln = rp[r + 1] - rp[r]
            if ln > 256 or (r > s and nn + ln > g["cap"]):
                break
            nn += ln
            r += 1
        cuts.append((s, r, int(rp[s]), int(rp[r])))
    return cuts


def recount(A, dt, mode, pct=80, stage_list=True, cuts=None, use_c16=True, use_stage=True, tiles_out=None):
    """The rule of include/rsp.h in numpy, tile by tile: on the greedy tiles
    of the matrix, or on the tiles `cuts` names ((r0, r1, k0, k1) each, for
    schedules the planner re-packed). tiles_out (a list) receives every tile
    as a dict of respasol_amd.sparse.TILE_FACTS."""
    g = GEO[dt]
    rp, ci = np.asarray(A.rowptr, np.int64), np.asarray(A.colidx, np.int64)
    out = dict.fromkeys(("tiles", "packed_tiles", "packed_entries", "staged_tiles", "index_bytes",
                         "packed_rowoff_bytes", "rowptr_bytes"), 0)
    desc = 0
    for r0, r1, k0, k1 in (greedy_cuts(rp, dt) if cuts is None else cuts):
        nn, nrows = k1 - k0, max(r1 - r0, 0)
        kind, base, U, R = "int32", 0, 0, 0
        if nn > 0 and use_c16:
            cols = np.unique(ci[k0:k1])
            if cols[-1] - cols[0] <= 65535:
                u, runs = len(cols), 1 + int(np.count_nonzero(np.diff(cols) != 1))
                kind, base = "gather16", int(cols[0])
                if use_stage and r1 >= 0 and (cols[-1] + 1) * XELEM[dt] <= 0x7ffffffc and u <= g["ucap"]:
                    if runs <= STAGE_RUNS and 100 * u <= pct * nn:
                        kind, U, R = "runs", u, runs
                    elif runs > STAGE_RUNS and dt == R64 and stage_list:
                        kind, U, R = "list", u, runs
        staged = kind in ("runs", "list")
        packed = staged and mode >= 1 and THREADS * ITER * g["vw"] * 12 // 8 < 2 * nn
        out["tiles"] += 1
        out["staged_tiles"] += staged
        out["packed_tiles"] += packed
        out["packed_entries"] += nn if packed else 0
        out["index_bytes"] += 4 * THREADS * g["nw"] if packed else 4 * nn if kind == "int32" else 2 * nn
        desc += 8 * (R + 1) if kind == "runs" else 8 + 2 * U if kind == "list" else 0
        if packed and mode >= 2:
            out["packed_rowoff_bytes"] += 4 * ((nrows + 2) // 2)
        else:
            out["rowptr_bytes"] += 4 * (nrows + 1)
        if tiles_out is not None:
            tiles_out.append(dict(r0=r0, r1=r1, k0=k0, k1=k1, kind=kind, base=base, U=U, R=R, packed=int(packed),
                                  packed_rows=int(packed and mode >= 2)))
    out["schedule_bytes"] = 24 * out["tiles"] + out["index_bytes"] + desc + out["packed_rowoff_bytes"]
    return out


def patterns(dt):
    yield from (csr.surrogate(s) for s in STENCILS + OTHERS)
    yield band_cycle()
    for last in EDGE[dt]:
        yield edge_matrix(last, dt)[0]
    yield edge_matrix(EDGE[dt][1], dt, 1)[0]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", [R64, R32])
def test_packed_plans_decode(dt, mode, monkeypatch):
    monkeypatch.setenv("RSP_SPMV_PACK", str(mode))
    for A in patterns(dt):
        st, tiles, e16, est = plan(A, dt)
        assert st == 0 and tiles > 0 and est <= e16 <= A.nnz_stored
        s = stats(A, dt)
        assert s["tiles"] == tiles and s["packed_entries"] <= est
        if mode == 0:
            assert s["packed_tiles"] == 0 and s["packed_rowoff_bytes"] == 0
        if mode < 2:
            assert s["packed_rowoff_bytes"] == 0


@pytest.mark.parametrize("dt", [R64, R32])
def test_knob_leaves_the_tiles_alone(dt, monkeypatch):
    A = csr.surrogate(STENCILS[0])
    got = []
    for mode in (0, 1, 2):
        monkeypatch.setenv("RSP_SPMV_PACK", str(mode))
        got.append((plan(A, dt), stats(A, dt)))
    assert got[0][0] == got[1][0] == got[2][0]
    s0, s1, s2 = (g[1] for g in got)
    assert s0["packed_tiles"] == 0 and s1["packed_tiles"] == s2["packed_tiles"] > 0.9 * s0["tiles"]
    assert s1["index_bytes"] == s2["index_bytes"] < s0["index_bytes"]
    assert s2["rowptr_bytes"] < s1["rowptr_bytes"] == s0["rowptr_bytes"]
    # a packed tile's indices are 1.5 B per slot of the image instead of 2 B per entry
    assert s0["index_bytes"] - s1["index_bytes"] == 2 * s1["packed_entries"] - 4 * THREADS * GEO[dt]["nw"] * s1["packed_tiles"]


@pytest.mark.parametrize("dt", [R64, R32])
def test_eligibility_edge(dt, monkeypatch):
    """A last tile of exactly 1536 (fp64) / 3072 (fp32) entries has as many
    index bytes packed as unpacked and stays unpacked; one entry more packs."""
    monkeypatch.delenv("RSP_SPMV_PACK", raising=False)
    for last, packed in zip(EDGE[dt], (False, True)):
        A, filler = edge_matrix(last, dt)
        assert A.nnz_stored % GEO[dt]["vw"] == 0
        s = stats(A, dt)
        assert s["tiles"] == 2 and s["staged_tiles"] == 2
        assert s["packed_tiles"] == 1 + packed and s["packed_entries"] == filler + (last if packed else 0)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", [R64, R32])
def test_stats_against_numpy_recount(dt, mode, monkeypatch):
    monkeypatch.setenv("RSP_SPMV_PACK", str(mode))
    mats = [band_cycle(), csr.surrogate(STENCILS[0])] + [edge_matrix(last, dt)[0] for last in EDGE[dt]]
    for A in mats:
        s, want = stats(A, dt), recount(A, dt, mode)
        assert s == {k: want[k] for k in s}
