"""The SpMV planner's digest lines (drivers/spmv_plan_check.cpp: per matrix,
type and option set: tiles, 16-bit entries, staged entries, packed tiles,
digest of the whole plan) over the matrices the plan tests use, under each
plan-time knob setting. No GPU. profiles/r09_spmv_plan_digest.txt is its
output; a planner change that is meant to keep the plans must reproduce it.

    python scripts/spmv_plan_digest.py > lines.txt
        runs respasol_amd/build/asan/spmv_plan_check_asan (make asan-plan)
    python scripts/spmv_plan_digest.py --hook-lib <librsp.so> > lines.txt
        calls rsp_spmv_plan_digest_lines(name, m, cols, rowptr, colidx) of a
        librsp.so that has such a hook (an older tree with the hook of the
        profile's header appended to its rsp_api.cpp)
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--hook-lib")
args = ap.parse_args()
if args.hook_lib:
    os.environ["RSP_PROBE_LIB"] = os.path.abspath(args.hook_lib)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from respasol_amd import _lib, csr  # noqa: E402
from test_gpu_spmv_fuzz import RECT_SEEDS, random_rect_matrix  # noqa: E402

EXE = os.path.join(ROOT, "respasol_amd", "build", "asan", "spmv_plan_check_asan")
SURROGATES = [("Serena", 0.02), ("Hook_1498", 0.02), ("atmosmodd", 0.05), ("ecology2", 0.05), ("cage13", 1.0),
              ("ASIC_320ks", 0.2), ("dc1", 0.3)]  # tests/test_spmv_plan.py::test_plan_decodes
KNOBS = [{}, {"RSP_SPMV_PACK": "0"}, {"RSP_SPMV_PACK": "1"}, {"RSP_SPMV_STAGE_LIST": "0"}, {"RSP_SPMV_STAGE_PCT": "30"}]


def band(seed, n, width, maxlen):
    """tests/test_spmv_plan.py: test_plan_odd_rows_and_bands (7), test_plan_list_tiles_ragged_band (11)"""
    rng = np.random.default_rng(seed)
    rows = [np.unique(np.clip(i + rng.integers(-width, width + 1, 1 + i % maxlen), 0, n - 1)) for i in range(n)]
    rp = np.zeros(n + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    return n, n, rp, np.concatenate(rows).astype(np.int32)


def matrices():
    for name, scale in SURROGATES:
        A = csr.surrogate(name, scale)
        yield f"{name}@{scale}", (A.m, A.n, A.rowptr, A.colidx)
    yield "band7", band(7, 20000, 700, 9)
    yield "band11", band(11, 60000, 20000, 15)
    for seed in RECT_SEEDS:
        A = random_rect_matrix(seed)
        yield f"rect{A.m}x{A.n}", (A.m, A.n, A.rowptr, A.colidx)


def main():
    if not args.hook_lib:
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "respasol_amd", "csrc"), "asan-plan"], check=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (m, cols, rp, ci) in matrices():
            rp = np.ascontiguousarray(rp, np.int32)
            ci = np.ascontiguousarray(ci[:rp[-1]], np.int32)
            path = os.path.join(tmp, "pattern.bin")
            if not args.hook_lib:
                with open(path, "wb") as f:
                    np.array([m, cols], np.int32).tofile(f)
                    rp.tofile(f)
                    ci.tofile(f)
            for knobs in KNOBS:
                tag = ",".join(f"{k}={v}" for k, v in knobs.items()) or "knobs-default"
                print(f"# {tag}", flush=True)
                if args.hook_lib:
                    saved = {k: os.environ.get(k) for k in knobs}
                    os.environ.update(knobs)
                    _lib.rsp.rsp_spmv_plan_digest_lines(name.encode(), m, cols, rp.ctypes.data_as(_lib.vp),
                                                        ci.ctypes.data_as(_lib.vp))
                    for k, v in saved.items():
                        os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
                else:
                    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
                               UBSAN_OPTIONS="halt_on_error=1", **knobs)
                    subprocess.run([EXE, "@" + path, name], env=env, check=True)


if __name__ == "__main__":
    main()
