"""The block-inverse solve's test matrices (tests/blk_cases.py), proven with
the CPU oracle alone: every case reaches the planner rule it is named for, at
exact counts from the oracle's restated plan (oracle_trsv_blocks_facts); the
block order stays within the solve tolerance of the reference's order; the
LDS need of the dense and band cases is the one the product's planner
computes; and the planner clamps the knobs its kernels cannot honour.
tests/test_gpu_blocks_cases.py runs the same cases through the kernels."""
import ctypes as C

import numpy as np
import pytest

import blk_cases as bc
import oracle_bind as ob
from respasol_amd import _lib

STOL = {np.float64: 1e-12, np.float32: 1e-4}  # normwise, the STOL of test_gpu_blocks.py
IDS = [c.id for c in bc.CASES]


def F(blocks, long, chunks, cap_cuts, rounds, long_aligned, long_far, max_far, partial, max_near, lds, per_chunk):
    return dict(blocks=blocks, long=long, chunks=chunks, cap_cuts=cap_cuts, rounds=rounds, long_aligned=long_aligned,
                long_far=long_far, max_far=max_far, partial=partial, max_near=max_near, lds=lds, per_chunk=per_chunk)


# id: (the facts of the DAG the case is built for: L of the original, L^T of
# the reversal; the facts of the other DAG: L^T of the original, L of the
# reversal, where a hub row is a column that many rows depend on).
# F(blocks, long blocks, chunks, chunks cut by the long-row cap, {rounds: long
# blocks}, long blocks with x + far terms a multiple of 64, long blocks with
# far terms, most far terms of a row, normal blocks of < 64 rows, most in-chunk
# terms of a normal row, LDS need in bytes, blocks per chunk)
FACTS = {
    # 7 long blocks (row 2148's 13 dependencies lie in its own block): 12 rounds
    # twice (768 and 767 terms), far terms up to 300 (two strides of 256 in the
    # prologue), x + far terms 64, 128 and 256 (aligned) and 63, 65, 301, 257
    "hubs": (F(77, 7, 4, 0, {1: 2, 2: 2, 3: 1, 12: 2}, 3, 7, 300, 10, 1, 44968, [16, 18, 24, 19]),
             F(64, 0, 4, 0, {}, 0, 0, 5, 0, 2, 52724, [16, 16, 16, 16])),
    "hubs-sym": (F(77, 7, 4, 0, {1: 2, 2: 2, 3: 1, 12: 2}, 3, 7, 300, 10, 1, 44968, [16, 18, 24, 19]),
                 F(64, 0, 4, 0, {}, 0, 0, 5, 0, 2, 52724, [16, 16, 16, 16])),
    "hubs-default": (F(296, 5, 2, 0, {1: 1, 2: 1, 3: 1, 12: 2}, 2, 5, 300, 6, 1, 43408, [256, 40]),
                     F(288, 0, 2, 0, {}, 0, 0, 1, 0, 6, 53592, [256, 32])),
    # one cut by the cap; chunks of 15 and 38 blocks; long rounds {0, 1, 4, 4}
    "capcut": (F(53, 4, 2, 1, {0: 1, 1: 1, 4: 2}, 0, 3, 769, 4, 1, 43408, [15, 38]),
               F(47, 0, 1, 0, {}, 0, 0, 0, 1, 4, 53420, [47])),
    "capcut-pair": (F(54, 5, 2, 1, {0: 1, 1: 2, 4: 2}, 0, 4, 769, 4, 1, 43408, [15, 39]),
                    F(47, 0, 1, 0, {}, 0, 0, 0, 1, 5, 55460, [47])),
    # 12 near terms and 32 y terms stay normal (max_near 12); 13 and 33 are long
    "near-edge": (F(268, 2, 2, 0, {1: 2}, 0, 1, 21, 4, 12, 55828, [258, 10]),
                  F(264, 0, 2, 0, {}, 0, 0, 1, 0, 2, 44840, [256, 8])),
    "near-edge-ch1024": (F(28, 2, 2, 0, {1: 2}, 0, 1, 21, 4, 12, 55828, [18, 10]),
                         F(24, 0, 2, 0, {}, 0, 0, 1, 0, 2, 44840, [16, 8])),
    # no near term allowed: only a chunk's first 64 rows form a normal block
    "near-edge-nmax0": (F(1410, 1408, 2, 0, {1: 1408}, 0, 2, 21, 0, 0, 43408, [961, 449]),
                        F(1410, 1408, 2, 0, {1: 1408}, 0, 0, 1, 0, 0, 43408, [961, 449])),
    "near-edge-nmax4": (F(30, 3, 2, 0, {1: 3}, 0, 1, 21, 5, 1, 56164, [20, 10]),
                        F(24, 0, 2, 0, {}, 0, 0, 1, 0, 2, 44840, [16, 8])),
    # no y term allowed: every row but the first 64 is a long block
    "near-edge-ymax0": (F(1473, 1472, 2, 0, {0: 1, 1: 1471}, 0, 3, 21, 0, 0, 42120, [961, 512]),
                        F(1473, 1472, 2, 0, {0: 1, 1: 1471}, 0, 1, 1, 0, 0, 42120, [961, 512])),
    "near-edge-ymax4": (F(31, 4, 2, 0, {1: 4}, 0, 2, 21, 6, 1, 43408, [20, 11]),
                        F(24, 0, 2, 0, {}, 0, 0, 1, 0, 2, 44840, [16, 8])),
    "dense-56": (F(1, 0, 1, 0, {}, 0, 0, 0, 1, 0, 155136, [1]),) * 2,
    "dense-64": (F(1, 0, 1, 0, {}, 0, 0, 0, 0, 0, 224400, [1]),) * 2,
    "band11-512": (F(8, 0, 1, 0, {}, 0, 0, 0, 0, 11, 154288, [8]),) * 2,
    "band12-512": (F(8, 0, 1, 0, {}, 0, 0, 0, 0, 12, 166432, [8]),) * 2,
    "dense-64-tail": (F(2, 0, 1, 0, {}, 0, 0, 0, 1, 1, 224400, [2]),
                      F(33, 32, 1, 0, {1: 32}, 0, 0, 0, 0, 0, 125200, [33])),
}


def chain_facts(n):
    """ceil(n / 64) blocks in one chunk, the last partial unless 64 divides n;
    a row's only y term is the position before its block. The LDS need, the
    two maxima over the blocks: a block of r rows has r - 1 dependencies (the
    first block) or r (a later one, whose rows each carry the y term), row t
    has t + 1 (+ 1) entries and as many recipe items as the row before it has
    entries, and r intra-block levels."""
    b = (n + 63) // 64
    shapes = [(min(n, 64), False)] + [(64, True)] * (b > 2) + [(n - 64 * (b - 1), True)] * (b > 1)
    elems = words = 0
    for r, later in shapes:
        ne = r * (r + 1) // 2 + (r if later else 0)
        nd = r if later else r - 1
        last = r + 1 if later else r  # the last row's entries: no row's items
        items = ne - last + (1 if later else 0)  # (a later block's first row: the constant 1)
        elems, words = max(elems, nd + 1 + ne), max(words, 2 * ne + 1 + items + r + 1)
    return F(b, 0, 1, 0, {}, 0, 0, 0, int(n % 64 != 0), int(b > 1), elems * 8 + words * 4, [b])


def expected(case, reverse, kind):
    if case.id.startswith("chain"):
        return chain_facts(case.n)
    return FACTS[case.id][int((kind == 1) != reverse)]


def facts(case, reverse, kind):
    A, _ = bc.build(case, reverse)
    return ob.blocks_facts(kind, A.rowptr, A.colidx, ob.blk_params_env(case.knobs))


@pytest.mark.parametrize("reverse", [False, True], ids=["orig", "rev"])
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_case_reaches_its_planner_rules(case, reverse):
    """Exact facts of both DAGs' plans; no long block of more than 12 rounds
    (a record has 12 slots per lane: the cap rule cuts the chunk before)."""
    A, _ = bc.build(case, reverse)
    for kind in (0, 1):
        assert ob.dag_levels(kind, A.rowptr, A.colidx) == case.n  # the chain: positions are rows
        f = facts(case, reverse, kind)
        want = expected(case, reverse, kind)
        assert {k: f[k] for k in want} == want, (case.id, reverse, kind)
        assert f["rounds_over_12"] == 0 and max(f["rounds"], default=0) <= 12
        assert sum(f["rounds"].values()) == f["long"] and sum(f["per_chunk"]) == f["blocks"]


def test_cases_cover_every_edge():
    """What the cases are for, over the whole set: chunks cut by the cap, long
    blocks of 0 to 12 rounds, aligned and unaligned long blocks, far terms
    past one stride of the prologue, more than two chunks, full near width,
    blocks per chunk on both sides of the walk's unroll depths (6 and 8)."""
    fs = [facts(c, False, 0) for c in bc.CASES]
    rounds = set().union(*(f["rounds"] for f in fs))
    assert {0, 1, 2, 3, 4, 12} <= rounds
    assert any(f["cap_cuts"] for f in fs) and max(f["chunks"] for f in fs) >= 4
    assert any(0 < f["long_aligned"] < f["long"] for f in fs)
    assert max(f["max_far"] for f in fs) > 256 and max(f["max_near"] for f in fs) == 12
    per_chunk = {b for f in fs for b in f["per_chunk"]}
    assert {1, 2, 5, 6, 7, 8, 9, 12, 13, 16, 17} <= per_chunk
    dflt = [f for c, f in zip(bc.CASES, fs) if not c.env]  # the default knobs see them too
    assert any(f["rounds"].get(12) and f["max_far"] > 256 for f in dflt)


@pytest.mark.parametrize("reverse", [False, True], ids=["orig", "rev"])
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_block_order_within_solve_tolerance(case, reverse):
    """The oracle's block order against its reference order, fp64 and fp32,
    alpha 1 and -0.75: within the project's solve tolerance."""
    A, x = bc.build(case, reverse)
    prm = ob.blk_params_env(case.knobs)
    for dt in (np.float64, np.float32):
        rv, sz, zp = ob.ilu0(A.rowptr, A.colidx, A.values.astype(dt))
        assert sz == -1 and zp == -1 and np.all(np.isfinite(rv))
        for alpha in (1.0, -0.75):
            z = ob.trsv("lower_n_blocks", A.rowptr, A.colidx, rv, x.astype(dt), alpha=alpha, params=prm)
            y = ob.trsv("lower_t_blocks", A.rowptr, A.colidx, rv, z, alpha=alpha, params=prm)
            fz = ob.trsv("lower_n_ref", A.rowptr, A.colidx, rv, x.astype(dt), alpha=alpha).astype(np.float64)
            fy = ob.trsv("lower_t_ref", A.rowptr, A.colidx, rv, z, alpha=alpha).astype(np.float64)
            assert np.linalg.norm(fz) > 0 and np.linalg.norm(fy) > 0
            assert np.linalg.norm(z - fz) <= STOL[dt] * np.linalg.norm(fz), (dt, alpha)
            assert np.linalg.norm(y - fy) <= STOL[dt] * np.linalg.norm(fy), (dt, alpha)


@pytest.mark.parametrize("reverse", [False, True], ids=["orig", "rev"])
@pytest.mark.parametrize("case,need", bc.LDS_EDGES, ids=[c.id for c, _ in bc.LDS_EDGES])
def test_lds_need_and_refusal(monkeypatch, case, need, reverse):
    """The oracle's LDS need equals the product planner's lds_elems * 8 +
    lds_words * 4 of these patterns; blocks are wanted exactly where it fits
    a CU's 163,840 B, per DAG; trsv('lower_n' / 'lower_t') then follows the
    reference's order."""
    A, x = bc.build(case, reverse)
    rv, _, _ = ob.ilu0(A.rowptr, A.colidx, A.values)
    for kind in (0, 1):
        want = need[kind ^ int(reverse)]
        assert ob.blocks_facts(kind, A.rowptr, A.colidx)["lds"] == want
        fits = want <= bc.LDS_MAX
        assert fits == (case.id not in ("dense-64", "band12-512") and not (case.id == "dense-64-tail"
                                                                           and kind == int(reverse)))
        for force in (None, "1"):
            monkeypatch.delenv("RSP_ILU_BLOCKS", raising=False)
            if force:
                monkeypatch.setenv("RSP_ILU_BLOCKS", force)
            assert ob.blocks_wanted(kind, A.rowptr, A.colidx) == fits
            name = ("lower_n", "lower_t")[kind]
            got = ob.trsv(name, A.rowptr, A.colidx, rv, x)
            assert np.array_equal(got, ob.trsv(name + ("_blocks" if fits else "_ref"), A.rowptr, A.colidx, rv, x))


def _digest(A):
    dg = C.c_uint64()
    rp = np.ascontiguousarray(A.rowptr, np.int32)
    ci = np.ascontiguousarray(A.colidx, np.int32)
    assert _lib.rsp.rsp_ilu0_analysis_host(A.n, rp.ctypes.data, ci.ctypes.data, None, None, C.byref(dg), None) == 0
    return dg.value


@pytest.mark.parametrize("reverse", [False, True], ids=["orig", "rev"])
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_product_planner_agrees_with_the_oracle(monkeypatch, capfd, case, reverse):
    """The product's host planner (no device) under the case's knobs, by its
    diagnostics line (RSP_ILU_BLK_STATS=1): blocks, long blocks, chunks and the
    two LDS maxima of each DAG equal the oracle's; a plan that does not fit
    the LDS prints none."""
    import re
    A, _ = bc.build(case, reverse)
    monkeypatch.delenv("RSP_ILU_BLOCKS", raising=False)
    for k in ("RSP_BLK_CH", "RSP_BLK_NMAX", "RSP_BLK_YMAX", "RSP_BLK_NW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("RSP_ILU_BLK_STATS", "1")
    capfd.readouterr()
    _digest(A)
    err = capfd.readouterr().err
    got = {int(m.group(1)): tuple(int(m.group(i)) for i in range(2, 7)) for m in re.finditer(
        r"plan_blocks kind=(\d) n=\d+ levels=\d+ blocks=(\d+) long=(\d+) segments=(\d+) .*? lds_elems=(\d+) "
        r"lds_words=(\d+)", err)}
    want = {}
    for kind in (0, 1):
        f = facts(case, reverse, kind)
        if f["lds"] <= bc.LDS_MAX:
            want[kind] = (f["blocks"], f["long"], f["chunks"], f["lds_elems"], f["lds_words"])
    assert got == want


def test_planner_clamps_knobs_the_kernels_cannot_honour(monkeypatch):
    """The host analysis' digest covers the block plans. A chunk longer than
    the LDS window (RSP_BLK_CH > 16384), more near terms than a record has
    slots (RSP_BLK_NMAX > 12) and a finite near window (RSP_BLK_NW) leave the
    plan unchanged on a matrix where each would change it: n > 16384, a row
    with 13 near terms, near terms 12 positions back. Knobs within range do
    change it."""
    A, _ = bc.build(bc.BY_ID["near-edge"])
    for k in ("RSP_BLK_CH", "RSP_BLK_NMAX", "RSP_BLK_NW", "RSP_BLK_YMAX", "RSP_ILU_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    base = _digest(A)
    assert base != 0 and _digest(A) == base
    for knob, values in (("RSP_BLK_CH", (20000, 16385, 1 << 30)), ("RSP_BLK_NMAX", (13, 64)),
                         ("RSP_BLK_NW", (0, 8, 100))):
        for v in values:
            monkeypatch.setenv(knob, str(v))
            assert _digest(A) == base, (knob, v)
        monkeypatch.delenv(knob)
    for knob, v in (("RSP_BLK_CH", 1024), ("RSP_BLK_NMAX", 4), ("RSP_BLK_YMAX", 4), ("RSP_ILU_BLOCKS", 0)):
        monkeypatch.setenv(knob, str(v))
        assert _digest(A) != base, (knob, v)
        monkeypatch.delenv(knob)


def test_refused_plan_changes_the_digest_only_by_its_absence(monkeypatch):
    """A refused plan is no plan: dense-64's digest equals the one with blocks
    switched off, dense-56's does not."""
    for cid, same in (("dense-64", True), ("dense-56", False)):
        A, _ = bc.build(bc.BY_ID[cid])
        monkeypatch.delenv("RSP_ILU_BLOCKS", raising=False)
        d = _digest(A)
        monkeypatch.setenv("RSP_ILU_BLOCKS", "0")
        assert (_digest(A) == d) == same
