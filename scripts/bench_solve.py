#!/usr/bin/env python3
"""ILU(0)- or Chebyshev-preconditioned BiCGStab, GMRES(m) or CG on the moderate
surrogates: does a narrower preconditioner, or one made of SpMVs alone, reach the
same residual in less time?

    python scripts/bench_solve.py [--names A,B] [--scale S] [--rtol R] [--maxit N]
                                  [--method bicgstab|gmres|cg] [--restart M]
                                  [--both-triangles] [--out FILE.jsonl]
                                  [--refine] [--inner-rtol R]
                                  [--cheby K[,K..]] [--cheby-ratio R]

Per matrix (b = 1, x0 = 0, fp64 iteration) and per configuration
    fp64      fp64 ILU(0) factor and solves
    fp32      fp32 factor and solves, the handle without FTZ
    fp32ftz   fp32 factor and solves, the handle with FTZ
one JSON line: iterations, reason (0 converged, 1 max iterations, 2
breakdown), the recurrence residual, the TRUE relative residual (fp64, host),
solve_ms (event-timed, median of 5 solves after one warm-up), and the cost of
the same work's library calls stand-alone: spmv_ms (one A x) and apply_ms (one
L solve + U solve in the preconditioner's type), each the median over 5 event
-timed loops of 2 * max(iterations, 1) calls. own_ms = solve_ms - iterations *
(2 spmv_ms + 2 apply_ms) is what the solver adds: its five vector kernels per
iteration (seven with a narrower preconditioner), the read-back, and the
launch gaps. With --method gmres (restarted flexible GMRES, restart length
--restart) an iteration is one SpMV and one apply, so applies = iterations,
own_ms = solve_ms - iterations * (spmv_ms + apply_ms), and what the solver
adds is its four kernels per iteration (five with a narrower preconditioner),
the cycle ends and the read-backs; BiCGStab's applies = 2 iterations. A matrix that ends in MAX_ITERS or BREAKDOWN is a result, not a
failure. A symmetric surrogate is its stored lower triangle (as everywhere in
this project), so its ILU(0) is exact and one iteration solves it.

--method cg (preconditioned conjugate gradients, rsp_cg_*) needs the whole
symmetric matrix: it runs on the surrogates whose surrogate_info(...)
["symmetric"] is set, each expanded on the host to both triangles (A + A^T -
diag, rows sorted), and skips the others with a note. An iteration is one SpMV
and one apply: applies = iterations, own_ms = solve_ms - iterations * (spmv_ms
+ apply_ms), what the solver adds being its four kernels per iteration (five
with a narrower preconditioner) and the read-backs. A surrogate expanded this
way is not guaranteed positive definite: BREAKDOWN is then the result.
--both-triangles gives BiCGStab and GMRES the same expanded matrices (and the
same skipping), for a comparison on equal systems.

--cheby K[,K..]: after the ILU(0) configurations (all of them, or those of
--configs; "--configs none" leaves the polynomial ones alone), two more per
degree K: chebyK (an fp64 Chebyshev polynomial preconditioner, rsp_cheby_*,
Jacobi scaling, on [lmax / R, lmax] with lmax the Gershgorin bound and R =
--cheby-ratio, default 30) and chebyK-fp32 (the polynomial on the fp32 values,
under the fp64 iteration). The record has the same fields; apply_ms is one
polynomial apply (K - 1 SpMVs and K kernels), setup_ms the host-blocking
rsp_cheby_create (wall clock), and ms_per_iter = solve_ms / iterations is added
to every record, ILU ones included.

--refine: instead of the three configurations, one line per matrix for
mixed-precision iterative refinement (rsp_refine_*: fp64 residuals and updates
around all-fp32 solves by --method to --inner-rtol, default 1e-4, each of at
most --maxit iterations; fp32 matrix, fp32 ILU(0), no FTZ): steps,
inner_iters, reason (3 = stagnated), relres and true_relres of the refined x
and refine_ms, and beside it the fp64 iteration under the same fp32
preconditioner by the same method (base_iters, base_reason, base_true_relres,
base_ms); ratio = refine_ms / base_ms. Times as above (median of 5 after one
warm-up).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from respasol_amd import _lib, csr  # noqa: E402
from respasol_amd.sparse import (CG, GMRES, BiCGStab, Cheby, Handle, Ilu0, Refine, RspError, SpMat,  # noqa: E402
                                 convert_scaled, upload_csr)

CONFIGS = (("fp64", torch.float64, False), ("fp32", torch.float32, False), ("fp32ftz", torch.float32, True))


def timed_ms(fn, reps=5):
    """Median event time of fn() over reps runs (after the caller's warm-up)."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def true_relres(A, x):
    ax = np.empty(A.m)
    xx = np.ascontiguousarray(x, np.float64)
    _lib.host.rsp_host_spmv_f64(A.m, A.rowptr.ctypes.data_as(_lib.ip), A.colidx.ctypes.data_as(_lib.ip),
                                A.values.ctypes.data, xx.ctypes.data, ax.ctypes.data)
    return float(np.linalg.norm(1.0 - ax) / np.sqrt(A.m))


def both_triangles(A):
    """A + A^T - diag of a stored lower triangle, rows sorted (host)."""
    rows = np.repeat(np.arange(A.m, dtype=np.int64), np.diff(A.rowptr))
    cols = A.colidx.astype(np.int64)
    off = rows != cols
    r = np.concatenate([rows, cols[off]])
    c = np.concatenate([cols, rows[off]])
    v = np.concatenate([A.values, A.values[off]])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    if np.any((r[1:] == r[:-1]) & (c[1:] == c[:-1])):
        raise ValueError("the stored part holds both (i, j) and (j, i)")
    rp = np.zeros(A.m + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(r, minlength=A.m))
    return csr.CsrMatrix(1, A.m, A.n, len(c), rp, c.astype(np.int32), np.ascontiguousarray(v), 0)


def run_one(name, A, cfg, rtol, maxit, method="bicgstab", restart=30):
    label, pdt, ftz = cfg
    rec = {"matrix": name, "config": label, "method": method, "n": A.m, "nnz": A.nnz_stored}
    per_iter = 2 if method == "bicgstab" else 1  # SpMVs (and applies) per iteration
    h = Handle(ftz=ftz)
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values)
    mat = SpMat(h, rp, ci, va, A.n)
    ilu = Ilu0(h, rp, ci)
    solver = None
    try:
        ilu.analysis()
        fac = va.to(pdt, copy=True)  # the factor overwrites it: never A's own values
        ilu.factor(fac)
        try:
            solver = (GMRES(h, mat, ilu, fac, restart=restart) if method == "gmres"
                      else CG(h, mat, ilu, fac) if method == "cg" else BiCGStab(h, mat, ilu, fac))
        except RspError as e:
            rec["error"] = str(e)
            return rec
        b = torch.ones(A.m, dtype=torch.float64, device="cuda")
        res = solver.solve(b, rtol=rtol, max_iters=maxit)  # warm-up
        rec.update(iters=res.iters, applies=per_iter * res.iters, reason=res.reason, relres=res.relres,
                   true_relres=true_relres(A, res.x.cpu().numpy()))
        rec["solve_ms"] = timed_ms(lambda: solver.solve(b, rtol=rtol, max_iters=maxit))
        calls = 2 * max(res.iters, 1)
        x = torch.ones(A.m, dtype=torch.float64, device="cuda")
        y = torch.empty_like(x)
        spmv = mat.bind(x, y)
        spmv()
        rec["spmv_ms"] = timed_ms(lambda: [spmv() for _ in range(calls)]) / calls
        px = torch.ones(A.m, dtype=pdt, device="cuda")
        pz, py = torch.empty_like(px), torch.empty_like(px)

        def apply():
            ilu.solve_lower(fac, px, pz)
            ilu.solve_upper(fac, pz, py)
        apply()
        rec["apply_ms"] = timed_ms(lambda: [apply() for _ in range(calls)]) / calls
        rec["own_ms"] = rec["solve_ms"] - res.iters * per_iter * (rec["spmv_ms"] + rec["apply_ms"])
        rec["own_share"] = rec["own_ms"] / rec["solve_ms"] if rec["solve_ms"] > 0 else 0.0
        rec["ms_per_iter"] = rec["solve_ms"] / max(res.iters, 1)
        return rec
    finally:
        if solver is not None:
            solver.close()
        ilu.close()
        mat.close()
        h.close()


def run_cheby(name, A, degree, pdt, rtol, maxit, method="bicgstab", restart=30, ratio=30.0):
    """As run_one, with the degree-`degree` Chebyshev polynomial of type pdt as M^-1."""
    label = f"cheby{degree}" + ("-fp32" if pdt == torch.float32 else "")
    rec = {"matrix": name, "config": label, "method": method, "n": A.m, "nnz": A.nnz_stored, "degree": degree,
           "ratio": ratio}
    per_iter = 2 if method == "bicgstab" else 1
    h = Handle()
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values)
    mat = SpMat(h, rp, ci, va, A.n)
    low = SpMat(h, rp, ci, convert_scaled(h, va, exp2=0, dtype=torch.float32), A.n) if pdt == torch.float32 else None
    poly = solver = None
    try:
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            poly = Cheby(h, low if low is not None else mat, degree, "jacobi", ratio)
            rec["setup_ms"] = (time.perf_counter() - t0) * 1e3
            rec["lmin"], rec["lmax"] = poly.bounds
            solver = (GMRES(h, mat, restart=restart, cheby=poly) if method == "gmres"
                      else CG(h, mat, cheby=poly) if method == "cg" else BiCGStab(h, mat, cheby=poly))
        except RspError as e:
            rec["error"] = str(e)
            return rec
        b = torch.ones(A.m, dtype=torch.float64, device="cuda")
        res = solver.solve(b, rtol=rtol, max_iters=maxit)  # warm-up
        rec.update(iters=res.iters, applies=per_iter * res.iters, reason=res.reason, relres=res.relres,
                   true_relres=true_relres(A, res.x.cpu().numpy()))
        rec["solve_ms"] = timed_ms(lambda: solver.solve(b, rtol=rtol, max_iters=maxit))
        calls = 2 * max(res.iters, 1)
        x = torch.ones(A.m, dtype=torch.float64, device="cuda")
        y = torch.empty_like(x)
        spmv = mat.bind(x, y)
        spmv()
        rec["spmv_ms"] = timed_ms(lambda: [spmv() for _ in range(calls)]) / calls
        px = torch.ones(A.m, dtype=pdt, device="cuda")
        pz = torch.empty_like(px)
        poly.apply(px, pz)
        rec["apply_ms"] = timed_ms(lambda: [poly.apply(px, pz) for _ in range(calls)]) / calls
        rec["own_ms"] = rec["solve_ms"] - res.iters * per_iter * (rec["spmv_ms"] + rec["apply_ms"])
        rec["own_share"] = rec["own_ms"] / rec["solve_ms"] if rec["solve_ms"] > 0 else 0.0
        rec["ms_per_iter"] = rec["solve_ms"] / max(res.iters, 1)
        return rec
    finally:
        if solver is not None:
            solver.close()
        if poly is not None:
            poly.close()
        if low is not None:
            low.close()
        mat.close()
        h.close()


def run_refine(name, A, rtol, maxit, method="bicgstab", restart=30, inner_rtol=1e-4):
    """The refined solve and, beside it, the fp64 iteration under the same fp32 factor."""
    rec = {"matrix": name, "config": "refine", "method": method, "n": A.m, "nnz": A.nnz_stored,
           "inner_rtol": inner_rtol}
    h = Handle()
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values)
    mat = SpMat(h, rp, ci, va, A.n)
    low = convert_scaled(h, va, exp2=0, dtype=torch.float32)
    mat_low = SpMat(h, rp, ci, low, A.n)
    ilu = Ilu0(h, rp, ci)
    solver = base = None
    try:
        ilu.analysis()
        fac = low.clone()  # the factor overwrites it: never A_low's own values
        ilu.factor(fac)
        try:
            solver = Refine(h, mat, mat_low, ilu, fac, method=method, restart=restart)
            base = (GMRES(h, mat, ilu, fac, restart=restart) if method == "gmres"
                    else CG(h, mat, ilu, fac) if method == "cg" else BiCGStab(h, mat, ilu, fac))
        except RspError as e:
            rec["error"] = str(e)
            return rec
        b = torch.ones(A.m, dtype=torch.float64, device="cuda")
        kw = dict(rtol=rtol, inner_rtol=inner_rtol, inner_max_iters=maxit)
        res = solver.solve(b, **kw)  # warm-up
        rec.update(steps=res.steps, inner_iters=res.iters, reason=res.reason, relres=res.relres,
                   true_relres=true_relres(A, res.x.cpu().numpy()))
        rec["refine_ms"] = timed_ms(lambda: solver.solve(b, **kw))
        bres = base.solve(b, rtol=rtol, max_iters=maxit)  # warm-up
        rec.update(base_iters=bres.iters, base_reason=bres.reason,
                   base_true_relres=true_relres(A, bres.x.cpu().numpy()))
        rec["base_ms"] = timed_ms(lambda: base.solve(b, rtol=rtol, max_iters=maxit))
        rec["ratio"] = rec["refine_ms"] / rec["base_ms"] if rec["base_ms"] > 0 else 0.0
        return rec
    finally:
        for s in (solver, base):
            if s is not None:
                s.close()
        ilu.close()
        mat_low.close()
        mat.close()
        h.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--names", default="", help="comma-separated surrogates (default: the 21 moderate ones)")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--maxit", type=int, default=200)
    ap.add_argument("--method", choices=("bicgstab", "gmres", "cg"), default="bicgstab")
    ap.add_argument("--restart", type=int, default=30, help="GMRES restart length")
    ap.add_argument("--both-triangles", action="store_true",
                    help="symmetric surrogates only, expanded to both triangles (implied by --method cg)")
    ap.add_argument("--configs", default="", help="comma-separated subset of fp64,fp32,fp32ftz")
    ap.add_argument("--out", default="", help="also append the records to this file")
    ap.add_argument("--refine", action="store_true",
                    help="mixed-precision iterative refinement beside the fp64 iteration under the fp32 factor")
    ap.add_argument("--inner-rtol", type=float, default=1e-4, help="--refine: the inner solves' rtol")
    ap.add_argument("--cheby", default="", help="comma-separated degrees of Chebyshev polynomial configurations")
    ap.add_argument("--cheby-ratio", type=float, default=30.0, help="--cheby: lmin = lmax / this")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_solve.py needs an MI355X: there is no CPU fallback")
    names = [s for s in args.names.split(",") if s] or csr.surrogate_names(0)
    out = open(args.out, "a") if args.out else None
    for name in names:
        A = csr.surrogate(name, args.scale)
        if args.method == "cg" or args.both_triangles:
            if not csr.surrogate_info(name)["symmetric"]:
                print(f"# {name}: not symmetric, skipped", file=sys.stderr, flush=True)
                continue
            A = both_triangles(A)
        if args.refine:
            line = json.dumps(run_refine(name, A, args.rtol, args.maxit, args.method, args.restart, args.inner_rtol))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            continue
        for cfg in CONFIGS:
            if args.configs and cfg[0] not in args.configs.split(","):
                continue
            line = json.dumps(run_one(name, A, cfg, args.rtol, args.maxit, args.method, args.restart))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        for degree in [int(k) for k in args.cheby.split(",") if k]:
            for pdt in (torch.float64, torch.float32):
                line = json.dumps(run_cheby(name, A, degree, pdt, args.rtol, args.maxit, args.method, args.restart,
                                            args.cheby_ratio))
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
