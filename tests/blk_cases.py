"""Generators for the block-inverse solve tests (helper module, no conftest):
matrices that reach every rule of the block planner (ilu_blocks.cpp) at a
position chosen by construction.

Every case is built on a chain: row i holds (i, i - 1) and the diagonal, so L's
DAG has n levels of one row, position == row, blocks are wanted by default
(n <= 32 x levels) and every extra dependency lands at a known position. Each
case also comes as its reversed transpose, (i, j) -> (n - 1 - j, n - 1 - i):
the L^T DAG of the reversal is the L DAG of the original, dependency order
included, so L^T meets every edge L meets.

tests/test_blk_cases.py pins the facts of every case with the CPU oracle
alone; tests/test_gpu_blocks_cases.py runs them through the kernels."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from respasol_amd import csr

WIN = 16384  # the default chunk length (rsp::kBlkWin)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    n: int
    extra: tuple = ()      # ((row, (columns < row, ...)), ...) besides the chain
    env: tuple = ()        # ((knob, value), ...) set before the analysis
    symmetric: bool = False  # the pattern's transpose stored too: a real factor feeds the solve
    seed: int = 0

    @property
    def knobs(self):
        return dict(self.env)


def _span(hi, count):
    """`count` columns ending just before hi."""
    return range(hi - count, hi)


def _lower_sets(case):
    low = [{i - 1} if i else set() for i in range(case.n)]
    for row, cols in case.extra:
        assert all(0 <= c < row < case.n for c in cols), (case.id, row)
        low[row].update(cols)
    return low


@functools.lru_cache(maxsize=None)
def build(case, reverse=False):
    """(A, x): the case's matrix (its reversed transpose with reverse=True) and
    a right-hand side. Off-diagonals uniform(-1, 1), diagonal 1 + the sum of
    the row's |off-diagonals| (the ILU fuzz's scheme), x uniform(-1, 1). Built
    once and shared between tests: not to be written."""
    n = case.n
    low = _lower_sets(case)
    rows = np.fromiter((i for i, s in enumerate(low) for _ in s), np.int64)
    cols = np.fromiter((c for s in low for c in sorted(s)), np.int64)
    if reverse:
        rows, cols = n - 1 - cols, n - 1 - rows
    d = np.arange(n, dtype=np.int64)
    if case.symmetric:
        rows, cols = np.concatenate((rows, cols, d)), np.concatenate((cols, rows, d))
    else:
        rows, cols = np.concatenate((rows, d)), np.concatenate((cols, d))
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int32)
    rng = np.random.default_rng([case.seed, int(reverse), n])
    vals = rng.uniform(-1.0, 1.0, rows.size)
    off = np.where(rows != cols, np.abs(vals), 0.0)
    vals[rows == cols] = 1.0 + np.bincount(rows, off, minlength=n)
    x = rng.uniform(-1.0, 1.0, n)
    return csr.CsrMatrix(0, n, n, int(rows.size), rowptr, cols.astype(np.int32), vals), x


# ------------------------------------------------------------------- chain
# Blocks per chunk around the chunk walk's unroll depth D (6 records in flight
# for fp64, 8 for fp32): b < D, = D, D + 1, 2 D, 2 D + 1, the last block full
# (n = 64 b) or of one row (n = 64 b - 63); and the smallest sizes.
CHAIN_N = (1, 2, 63, 64, 65) + tuple(v for b in (5, 6, 7, 8, 9, 12, 13, 16, 17) for v in (64 * b - 63, 64 * b))
CHAINS = tuple(Case(f"chain-{n}", n) for n in CHAIN_N) + tuple(
    Case(f"chain-sym-{n}", n, symmetric=True) for n in (65, 385, 1088))


# -------------------------------------------------------------------- hubs
def hub(h, m, f, c0):
    """Row h with m dependencies just before it (its chain entry among them)
    and f just before its chunk's start c0."""
    assert h - m >= c0 >= f
    return h, tuple(_span(c0, f)) + tuple(_span(h, m))


# (row, in-chunk dependencies, far dependencies), chunks of 1024 positions
HUBS = ((1824, 768, 63), (2148, 13, 0), (2248, 64, 62), (2348, 65, 64), (2548, 128, 127), (2748, 129, 300),
        (3172, 33, 256), (3972, 767, 255))
_hubs = tuple(hub(h, m, f, h // 1024 * 1024) for h, m, f in HUBS)
# the default chunk length: the hubs in the second chunk
HUBS_DEFAULT = ((800, 768, 63), (900, 64, 62), (1000, 65, 64), (1200, 129, 300), (2000, 767, 255))
_hubs_default = tuple(hub(WIN + h, m, f, WIN) for h, m, f in HUBS_DEFAULT)

HUB_CASES = (Case("hubs", 4096, _hubs, (("RSP_BLK_CH", 1024),)),
             Case("hubs-sym", 4096, _hubs, (("RSP_BLK_CH", 1024),), symmetric=True),
             Case("hubs-default", WIN + 2048, _hubs_default))

# ------------------------------------------------------------------ capcut
# Row 900: 769 dependencies at or after its chunk's start: it starts a chunk
# and is a long block of 0 rounds and 769 far terms. Row 1000: 60, all in the
# new chunk. Row 1100: 200 in the chunk, 100 far. Row 1101: 201 in the chunk
# and 579 far: no second cut. In capcut-pair row 901 holds 769 dependencies as
# well: it cannot cut again (at most its chain entry lies at or after the new
# chunk's start, whatever the row holds), and is a long block of one in-chunk
# term right behind the chunk's start.
_capcut = ((900, tuple(_span(900, 769))), (1000, tuple(_span(1000, 60))), (1100, tuple(_span(1100, 300))),
           (1101, tuple(_span(1101, 780))))
CAPCUTS = (Case("capcut", 3000, _capcut),
           Case("capcut-pair", 3000, _capcut[:1] + ((901, tuple(_span(901, 769))),) + _capcut[1:]))


# --------------------------------------------------------------- near_edge
def near_edge(c1):
    """Rows at the near and y caps, c1 the second chunk's start. Blocks start
    at multiples of 64 until a long row closes one.
      row 200 (block 192..): 180..191 = 12 in-chunk terms outside the block
        (the block's own term 191 among them): stays, kn = 12;
      row 300 (block 256..): 243..255 = 13: the block closes, a long block of
        one round (299 and the 13);
      row c1 + 116 (block c1 + 64..): 20 far + 12 near = 32 y terms: stays;
      row c1 + 216 (block c1 + 192..): 21 far + 12 near = 33: long, 13 in-chunk
        terms (its chain entry too), 1 + 21 x and far terms."""
    return ((200, tuple(_span(192, 12))), (300, tuple(_span(256, 13))),
            (c1 + 116, tuple(_span(c1 - 300, 20)) + tuple(_span(c1 + 64, 12))),
            (c1 + 216, tuple(_span(c1 - 200, 21)) + tuple(_span(c1 + 192, 12))))


_CH1K = (("RSP_BLK_CH", 1024),)
NEAR_EDGES = (Case("near-edge", WIN + 512, near_edge(WIN)),
              Case("near-edge-ch1024", 1536, near_edge(1024), _CH1K)) + tuple(
    Case(f"near-edge-{k.lower()}{v}", 1536, near_edge(1024), _CH1K + ((f"RSP_BLK_{k}", v),))
    for k in ("NMAX", "YMAX") for v in (0, 4))


# ---------------------------------------------------------------- lds_edge
def dense(n):
    return tuple((i, tuple(range(i))) for i in range(1, n))


def band(n, hw):
    return tuple((i, tuple(range(max(i - hw, 0), i))) for i in range(1, n))


# (case, the coefficient build's LDS need at fp64 in bytes of the L and of the
# L^T plan); a CU has 163,840 B. dense-64-tail: a dense 64-row block, then 32
# chain rows: one block for L, but in L^T's order the chain rows come first and
# the dense rows fall into two blocks, so only L's plan is refused (the
# reversal: only L^T's).
LDS_MAX = 160 * 1024
LDS_EDGES = ((Case("dense-56", 56, dense(56)), (155136, 155136)),
             (Case("dense-64", 64, dense(64)), (224400, 224400)),
             (Case("band11-512", 512, band(512, 11)), (154288, 154288)),
             (Case("band12-512", 512, band(512, 12)), (166432, 166432)),
             (Case("dense-64-tail", 96, dense(64)), (224400, 125200)))

CASES = CHAINS + HUB_CASES + CAPCUTS + NEAR_EDGES + tuple(c for c, _ in LDS_EDGES)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
