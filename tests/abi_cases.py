"""What the tests of the C-ABI's worded promises share (test_gpu_streams.py,
test_gpu_set_values.py): the two SpMV matrices that between them take every
kind of tile, bit views, and the test kit's bounded occupant."""
import ctypes
import functools
import os

import numpy as np

from respasol_amd import csr
from test_spmv_plan_packed import STENCILS

TESTKIT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "respasol_amd", "lib",
                       "librsp_testkit.so")
HUB_N, HUB_ROW, HUB_LEN = 6000, 997, 5000


@functools.lru_cache(maxsize=None)
def hub_matrix():
    """The hub matrix of test_gpu_spmv.test_long_row_tickets_repeat cut to
    6000 rows with ONE hub row of 5000 entries (chunked: 3 fp64 / 2 fp32
    tiles' worth), the other rows a 5-entry random band."""
    rng = np.random.default_rng(11)
    cols = []
    for i in range(HUB_N):
        if i == HUB_ROW:
            c = np.sort(rng.choice(HUB_N, HUB_LEN, replace=False)).astype(np.int32)
        else:
            c = np.unique(np.clip(i + rng.integers(-30, 31, 5), 0, HUB_N - 1)).astype(np.int32)
        cols.append(c)
    rp = np.zeros(HUB_N + 1, np.int32)
    np.cumsum([len(c) for c in cols], out=rp[1:])
    ci = np.concatenate(cols)
    return csr.CsrMatrix(0, HUB_N, HUB_N, len(ci), rp, ci, rng.uniform(-1, 1, len(ci)))


@functools.lru_cache(maxsize=None)
def stencil_matrix():
    """A 3-D stencil: staged tiles, packed records (tests/test_spmv_plan_packed.py)."""
    return csr.surrogate(STENCILS[0])


SPMV_MATRICES = {"hub": hub_matrix, "stencil": stencil_matrix}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def occupant_kit():
    """librsp_testkit.so (test-only): rsp_testkit_occupy(stream, workgroups, microseconds)."""
    tk = ctypes.CDLL(TESTKIT)
    tk.rsp_testkit_occupy.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong]
    tk.rsp_testkit_occupy.restype = ctypes.c_int
    return tk
