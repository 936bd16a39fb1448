"""The crafted SpMV patterns (tests/spmv_cases.py), proven on the CPU: for both
types every case's verified plan (rsp_spmv_plan_tiles_host) has the tiles the
case pins, tile by tile the facts are those of a numpy recount of the rule
(test_spmv_plan_packed.recount), rsp_spmv_plan_stats agrees with the same
recount, and the lanes per row and heavy-row counts of the reduce cases follow
from the restated rule (spmv_epilogue_ref.tile_lanes). Over the whole set every
limit of spmv_cases.limits is met at its value and one past it. Every case
also goes, as a pattern file, through the stand-alone planner check under
ASan + UBSan and under ThreadSanitizer (4 threads, the same lines from both),
and through its --mutate mode: plan_verify rejects every corrupted plan, and
every corruption is applied by some case.

The x-resource pair (xrsrc-at / xrsrc-past) is checked here only: its x would
be 2 GiB, no test of a few seconds on a shared machine.
tests/test_gpu_spmv_cases.py runs all the other cases through the kernels."""
import collections
import os
import subprocess

import numpy as np
import pytest

import spmv_cases as sc
import spmv_epilogue_ref as er
from respasol_amd.sparse import spmv_plan_tiles
from spmv_cases import R32, R64
from test_sanitize import _clean, plan_exes  # noqa: F401  (plan_exes: the fixture that builds the two drivers)
from test_spmv_plan_packed import WHOLE_ROW, recount, stats

IDS = [c.id for c in sc.CASES]
DT_IDS = {R64: "fp64", R32: "fp32"}
# the planner re-packs these (list_repack, spread, row_align, the split order): the recount takes the plan's cuts
RECUT = {c.id for c in sc.CASES if c.opts or c.id.startswith("list-repack")}
MUTANTS = ("c16", "cbase", "run-col", "run-slot", "sentinel", "slot-swap", "list-ofs", "list-u", "pack-pad",
           "pack-field", "pack-row", "poff", "nint", "tile-swap")


def plan(case, dt, monkeypatch, extra=()):
    sc.set_knobs(monkeypatch, case, extra)
    A = sc.build(case.id, dt)
    return A, spmv_plan_tiles(A.rowptr, A.colidx, fp32=dt == R32, **case.options(dt))


def knob(case, name, default):
    return int(dict(case.env).get(name, default))


def rows_of(t):
    return "whole" if t["r1"] == WHOLE_ROW else "chunk" if t["r1"] < 0 else t["r1"] - t["r0"]


@pytest.mark.parametrize("dt", sc.DTS, ids=DT_IDS.values())
@pytest.mark.parametrize("cid", IDS)
def test_case_reaches_its_facts(cid, dt, monkeypatch):
    case = sc.BY_ID[cid]
    A, p = plan(case, dt, monkeypatch)
    got = [sc.T(t["kind"], rows_of(t), t["k1"] - t["k0"], t["U"], t["R"], t["packed"]) for t in p["tiles"]]
    want = case.tiles(dt)
    assert len(got) == len(want), got
    for i, (g, w) in enumerate(zip(got, want)):
        assert all(b is None or a == b for a, b in zip(g, w)), (i, g, w)
    for t in p["tiles"]:  # mode 2 (the default): a packed record carries the row offsets
        assert t["packed_rows"] == t["packed"]
    for name, value in dict(case.counts(dt) if case.counts else ()).items():
        assert p[name] == value, (name, p[name])
    if case.lanes:
        lens = np.diff(np.asarray(A.rowptr, np.int64))
        found = [er.heavy_rows_of_tile(lens, t["r0"], t["r1"]) for t in p["tiles"] if t["r1"] >= 0]
        assert [L for L, _ in found] == case.lanes(dt)
        assert [len(h) for _, h in found] == case.heavy(dt)
        assert max(len(h) for _, h in found) <= 128  # rsp_kernels.h kSpmvHeavyMax


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("dt", sc.DTS, ids=DT_IDS.values())
@pytest.mark.parametrize("cid", IDS)
def test_facts_and_stats_agree_with_the_recount(cid, dt, mode, monkeypatch):
    case = sc.BY_ID[cid]
    A, p = plan(case, dt, monkeypatch, (("RSP_SPMV_PACK", mode),))
    cuts = [(t["r0"], t["r1"], t["k0"], t["k1"]) for t in p["tiles"]] if cid in RECUT else None
    tiles = []
    want = recount(A, dt, mode, pct=knob(case, "RSP_SPMV_STAGE_PCT", 80),
                   stage_list=knob(case, "RSP_SPMV_STAGE_LIST", 1) != 0, cuts=cuts, tiles_out=tiles,
                   use_c16=case.options(dt).get("use_c16", 1) != 0, use_stage=case.options(dt).get("use_stage", 1) != 0)
    assert p["tiles"] == tiles
    if not case.opts:  # rsp_spmv_plan_stats plans with the default options
        s = stats(A, dt)
        assert s == {k: want[k] for k in s}


@pytest.mark.parametrize("dt", sc.DTS, ids=DT_IDS.values())
def test_every_limit_is_met_and_passed(dt, monkeypatch):
    reached = collections.defaultdict(set)
    for case in sc.CASES:
        A, p = plan(case, dt, monkeypatch)
        for name, values in sc.measures(A, dt, p["tiles"], knob(case, "RSP_SPMV_STAGE_PCT", 80)).items():
            reached[name] |= values
    missing = [(name, v) for name, lim in sc.limits(dt).items() for v in lim if v is not None and v not in reached[name]]
    assert not missing, missing
    # the arrays end inside a vector (the scalar path), and a tile starts inside one, per kind of staged tile
    lists = {"list"} if dt == R64 else set()
    assert {"runs", "runs-packed"} | lists <= reached["scalar-tail"], reached["scalar-tail"]
    assert {"runs"} | lists <= reached["odd-k0"], reached["odd-k0"]


def write_pattern(A, path):
    hdr = np.array([A.m, A.n], np.int32)
    with open(path, "wb") as f:
        for a in (hdr, np.asarray(A.rowptr, np.int32), np.asarray(A.colidx, np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())


def test_cases_under_the_sanitizers_and_the_mutants(plan_exes, tmp_path):  # noqa: F811
    """fp64 and fp32 plans of the type's own matrix: the driver plans both
    types of the file it is given, so each case is written once per type."""
    base = dict(os.environ, OMP_NUM_THREADS="4", TSAN_OPTIONS="halt_on_error=1",
                ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for k in sc.PLAN_KNOBS:
        base.pop(k, None)
    rejected = {"f64": set(), "f32": set()}
    for case in sc.CASES:
        env = dict(base, **{k: str(v) for k, v in case.env})
        for dt in sc.DTS:
            path = tmp_path / "pattern.bin"
            write_pattern(sc.build(case.id, dt), path)
            for args in (["@" + str(path), case.id], ["--mutate", "@" + str(path), case.id]):
                outs = []
                for exe in plan_exes:
                    p = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=120)
                    ok, err = _clean(p)
                    assert ok and "ThreadSanitizer" not in err, (case.id, err)
                    assert p.returncode == 0, (case.id, args[0], p.returncode, err)
                    outs.append(p.stdout)
                assert outs[0] == outs[1], case.id
                if args[0] == "--mutate":
                    for line in outs[0].splitlines():
                        w = line.split()
                        assert w[2] == "rejected"
                        rejected[w[1]] |= set(w[3:w.index("absent")])
                else:
                    assert len(outs[0].splitlines()) == 14
    assert rejected["f64"] == set(MUTANTS)
    assert rejected["f32"] == set(MUTANTS) - {"list-ofs", "list-u"}  # no list tiles in fp32
