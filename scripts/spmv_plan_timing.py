"""Wall time of the SpMV planner on the host (no GPU): one process per run,
libraries alternating, one untimed call (the host pool maps its blocks), then
one timed respasol_amd.sparse.spmv_plan_stats per matrix, fp64.

    OMP_NUM_THREADS=16 python scripts/spmv_plan_timing.py <old librsp.so> <new librsp.so> [runs]
    (inner: python scripts/spmv_plan_timing.py --one, the library chosen with RSP_PROBE_LIB)
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = [("Serena", 0.2), ("cage13", 1.0)]


def one():
    sys.path.insert(0, ROOT)
    from respasol_amd import csr, sparse
    out = {}
    for name, scale in MATS:
        A = csr.surrogate(name, scale)
        sparse.spmv_plan_stats(A.rowptr, A.colidx)
        t0 = time.perf_counter()
        st = sparse.spmv_plan_stats(A.rowptr, A.colidx)
        out[name] = {"ms": (time.perf_counter() - t0) * 1e3, "tiles": st["tiles"]}
    print(json.dumps(out))


def main():
    libs = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.abspath(sys.argv[2])}
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    got = {k: {n: [] for n, _ in MATS} for k in libs}
    for r in range(runs):
        for side, lib in libs.items():
            p = subprocess.run([sys.executable, __file__, "--one"], env=dict(os.environ, RSP_PROBE_LIB=lib),
                               capture_output=True, text=True, check=True)
            res = json.loads(p.stdout.strip().splitlines()[-1])
            for n, v in res.items():
                got[side][n].append(v["ms"])
            print(f"run {r + 1} {side:6s} " + "  ".join(f"{n} {v['ms']:8.2f} ms ({v['tiles']} tiles)"
                                                       for n, v in res.items()), flush=True)
    for n, _ in MATS:
        lo, hi = min(got["parent"][n]), max(got["parent"][n])
        med = statistics.median(got["new"][n])
        print(f"{n}: parent min {lo:.2f} median {statistics.median(got['parent'][n]):.2f} max {hi:.2f} ms; "
              f"new median {med:.2f} ms (min {min(got['new'][n]):.2f} max {max(got['new'][n]):.2f}): "
              f"{'inside' if lo <= med <= hi else 'OUTSIDE'} the parent's interval")


if __name__ == "__main__":
    one() if "--one" in sys.argv else main()
