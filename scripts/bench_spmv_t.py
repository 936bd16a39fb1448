"""Transposed SpMV: what rsp_spmv(op = TRANSPOSE) costs, in ONE process.

    python scripts/bench_spmv_t.py [--set moderate|big|name,name] [--dtype f64,f32]
                                   [--rounds 7] [--reps 20] [--scale 1.0] [--out FILE]

Per matrix and type, event-timed on the device (hot: --reps back-to-back calls
between one event pair after a warm-up call; the four measurements alternate
inside every round, so a drift of the box hits all of them; median over the
rounds, and the spread = (max - min) / 2 of the rounds next to it):

  a   rsp_spmv(op = T) on A
  b   rsp_spmv(op = N) on a descriptor over the rsp_csr2csc transpose
  c   the permutation pass alone (rsp_spmv_transpose_permute)
  g   rsp_gather of the same values by the same permutation widened to int64

and on the host (wall clock, one cold call each): bufferSize(op = T) in all,
the transposer alone (rsp_csr_transpose_host on the host pattern), the plan of
A^T alone (bufferSize(op = N) on the explicit transpose, its pattern download
included); the remainder is the pattern's download and the upload of A^T.

Two conditions are printed per line and counted at the end:
  c <= g + spread             the permutation is no slower than rsp_gather
  |a - (b + c)| <= spread     op = T costs the permutation plus the forward
                              product: no hidden synchronisation or re-plan
(spread: the larger of the spreads involved). Reported beside them: the
permutation's bytes per second, nnz * (4 + 2 * element) bytes over c, against
the 8 TB/s peak. One line per matrix and type, `key=value` fields; --out
appends them to a file as well.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from respasol_amd import _lib, csr  # noqa: E402
from respasol_amd.sparse import Handle, SpMat, csr2csc, csr_transpose_host, upload_csr  # noqa: E402

PEAK = 8.0e12


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def buffer_size_t(h, M):
    size = C.c_size_t()
    one, zero = (C.c_double(1.0), C.c_double(0.0)) if M.dtype == torch.float64 else (C.c_float(1.0), C.c_float(0.0))
    _lib.check(_lib.rsp.rsp_spmv_buffer_size(h.ptr, _lib.OP_T, C.byref(one), M._mat, C.byref(zero),
                                             _lib.R_64F if M.dtype == torch.float64 else _lib.R_32F, C.byref(size)),
               "rsp_spmv_buffer_size")


def timed(fn, reps, e0, e1):
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="moderate")
    ap.add_argument("--dtype", default="f64,f32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spmv_t.py needs the MI355X"
    names = (csr.surrogate_names({"big": 1, "moderate": 0}[args.set]) if args.set in ("big", "moderate")
             else args.set.split(","))
    dtypes = [{"f64": torch.float64, "f32": torch.float32}[d] for d in args.dtype.split(",")]
    h = Handle()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = open(args.out, "a") if args.out else None
    fails = {"perm_vs_gather": 0, "additive": 0}
    lines = 0
    for name in names:
        A = csr.surrogate(name, args.scale)
        host_tr, _ = wall(lambda: csr_transpose_host(A.rowptr, A.colidx, A.n))
        for dt in dtypes:
            elem = 8 if dt == torch.float64 else 4
            rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, dt)
            nnz = A.nnz_stored
            M = SpMat(h, rp, ci, va, A.n)
            host_all, _ = wall(lambda: buffer_size_t(h, M))
            t_rp, t_ci, t_va = csr2csc(h, rp, ci, va, A.n)
            host_plan, E = wall(lambda: SpMat(h, t_rp, t_ci, t_va, A.m))
            perm64 = torch.from_numpy(csr_transpose_host(A.rowptr, A.colidx, A.n)[2]).to(torch.int64).cuda()
            x = torch.from_numpy(csr.dlarnv(1, [0, 0, 0, 1], A.m)[0]).to(dt).cuda()
            y = torch.empty(A.n, dtype=dt, device="cuda")
            dst = torch.empty(nnz, dtype=dt, device="cuda")
            assert torch.equal(M.spmv(x, transpose=True).view(torch.uint8), E.spmv(x).view(torch.uint8))
            # the C arguments converted once (as SpMat.bind): a call is one ctypes call
            one, zero = (C.c_double(1.0), C.c_double(0.0)) if elem == 8 else (C.c_float(1.0), C.c_float(0.0))
            typ = _lib.R_64F if elem == 8 else _lib.R_32F
            px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
            args_a = (h.ptr, _lib.OP_T, C.byref(one), M._mat, px, C.byref(zero), py, typ, None)
            args_g = (h.ptr, typ, nnz, C.c_void_p(perm64.data_ptr()), C.c_void_p(va.data_ptr()),
                      C.c_void_p(dst.data_ptr()))
            spmv, permute, gath = _lib.rsp.rsp_spmv, _lib.rsp.rsp_spmv_transpose_permute, _lib.rsp.rsp_gather
            calls = {
                "a": lambda: spmv(*args_a),
                "b": E.bind(x, y),
                "c": lambda: permute(h.ptr, M._mat),
                "g": lambda: gath(*args_g),
            }
            assert calls["a"]() == 0 and calls["c"]() == 0 and calls["g"]() == 0
            assert torch.equal(dst.view(torch.uint8), t_va.view(torch.uint8))
            t = {k: [] for k in calls}
            for _ in range(args.rounds):
                for k, fn in calls.items():
                    t[k].append(timed(fn, args.reps, e0, e1))
            med = {k: statistics.median(v) for k, v in t.items()}
            spr = {k: (max(v) - min(v)) / 2 for k, v in t.items()}
            ok_g = med["c"] <= med["g"] + max(spr["c"], spr["g"])
            ok_add = abs(med["a"] - (med["b"] + med["c"])) <= max(spr.values())
            fails["perm_vs_gather"] += not ok_g
            fails["additive"] += not ok_add
            perm_bps = nnz * (4 + 2 * elem) / (med["c"] * 1e-6) if med["c"] > 0 else 0.0
            line = (f"matrix={name} type={'f64' if elem == 8 else 'f32'} n={A.m} nnz={nnz} "
                    + " ".join(f"{k}_us={med[k]:.2f} {k}_spread={spr[k]:.2f}" for k in calls)
                    + f" a_minus_bc_us={med['a'] - med['b'] - med['c']:.2f} perm_GBps={perm_bps / 1e9:.0f}"
                    f" perm_frac_of_peak={perm_bps / PEAK:.3f} perm_le_gather={int(ok_g)} additive={int(ok_add)}"
                    f" host_bufferSizeT_ms={host_all:.2f} host_transposer_ms={host_tr:.2f}"
                    f" host_child_plan_ms={host_plan:.2f} host_rest_ms={host_all - host_tr - host_plan:.2f}")
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            lines += 1
            M.close()
            E.close()
            del rp, ci, va, t_rp, t_ci, t_va, perm64, x, y, dst
        del A
    summary = (f"summary set={args.set} lines={lines} rounds={args.rounds} reps={args.reps} "
               f"perm_slower_than_gather={fails['perm_vs_gather']} not_additive={fails['additive']}")
    print(summary)
    if out:
        out.write(summary + "\n")
        out.close()
    h.close()


if __name__ == "__main__":
    main()
