"""Interleaved A/B of the packed staged tiles (RSP_SPMV_PACK = 0 / 1 / 2) on
the batched launch that bench.py times, in ONE process (as scripts/spmv_ab.py).

    python scripts/spmv_pack_ab.py [--set big] [--rounds 7] [--reps 10] [--dtype f64,f32]
    python scripts/spmv_pack_ab.py --stats-only      (host only: no device needed)

RSP_SPMV_PACK is read when a schedule is built, so the three arms are three
SpmvBatch objects over the same device matrices, planned under the three knob
values. A round times, per arm, `reps` back-to-back batched launches (each over
the whole set, so nothing stays in the Infinity Cache from one launch to the
next) between one event pair; arms alternate inside a round. Reported per arm:
median, minimum and maximum over the rounds of the time per launch, and the gain
against arm 0. --stats-only prints the bytes one launch reads besides values,
x and y (rsp_spmv_plan_stats, exact) per arm, summed over the set.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from respasol_amd import csr  # noqa: E402

ARMS = (0, 1, 2)


def set_names(which):
    return csr.surrogate_names({"big": 1, "moderate": 0}[which]) if which in ("big", "moderate") else which.split(",")


def plan_stats(names, dtypes):
    from respasol_amd.sparse import spmv_plan_stats
    out = {}
    for n in names:
        A = csr.surrogate(n)
        for dt in dtypes:
            for arm in ARMS:
                os.environ["RSP_SPMV_PACK"] = str(arm)
                s = spmv_plan_stats(A.rowptr, A.colidx, fp32=dt == "f32", nnz=int(max(A.nnz, A.nnz_stored)))
                s["entries"] = int(A.nnz_stored)
                tot = out.setdefault(dt, {}).setdefault(arm, {})
                for k, v in s.items():
                    tot[k] = tot.get(k, 0) + v
                out[dt].setdefault("per_matrix", {}).setdefault(n, {})[arm] = s
        del A
    os.environ.pop("RSP_SPMV_PACK", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="big")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", default="f64,f32")
    ap.add_argument("--stats-only", action="store_true")
    ap.add_argument("--json", default=None, help="also write the result here")
    args = ap.parse_args()
    names = set_names(args.set)
    dtypes = args.dtype.split(",")
    result = {"set": args.set, "matrices": len(names)}
    if args.stats_only:
        st = plan_stats(names, dtypes)
        for dt in dtypes:
            for arm in ARMS:
                s = st[dt][arm]
                print(f"{dt} RSP_SPMV_PACK={arm}: tiles {s['tiles']} packed {s['packed_tiles']} "
                      f"({s['packed_entries']} of {s['entries']} entries)  schedule {s['schedule_bytes']} B "
                      f"(indices {s['index_bytes']}, packed row offsets {s['packed_rowoff_bytes']})  "
                      f"rowptr {s['rowptr_bytes']} B  together {s['schedule_bytes'] + s['rowptr_bytes']} B")
            d1 = st[dt][0]["schedule_bytes"] + st[dt][0]["rowptr_bytes"]
            for arm in ARMS[1:]:
                print(f"{dt} saved by {arm}: {d1 - st[dt][arm]['schedule_bytes'] - st[dt][arm]['rowptr_bytes']} B per launch")
        result["stats"] = st
    else:
        import torch
        from respasol_amd.sparse import Handle, SpMat, SpmvBatch, upload_csr
        h = Handle()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        result["ab"] = {}
        for dts in dtypes:
            dt = torch.float64 if dts == "f64" else torch.float32
            dev, xs, ys = [], [], []
            for n in names:
                A = csr.surrogate(n)
                dev.append((upload_csr(A.rowptr, A.colidx, A.values, dt), A.n))
                xs.append(torch.from_numpy(csr.dlarnv(1, [0, 0, 0, 1], A.n)[0]).to(dt).cuda())
                ys.append(torch.empty(A.m, dtype=dt, device="cuda"))
                del A
            batches, keep = {}, []
            for arm in ARMS:
                os.environ["RSP_SPMV_PACK"] = str(arm)
                mats = [SpMat(h, *d, n) for d, n in dev]
                batches[arm] = SpmvBatch(h, mats, xs, ys)
                keep.append(mats)
            os.environ.pop("RSP_SPMV_PACK", None)
            ref = None
            for arm in ARMS:  # the same bits from every arm
                batches[arm].run()
                torch.cuda.synchronize()
                got = [y.clone() for y in ys]
                if ref is None:
                    ref = got
                assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(ref, got)), \
                    f"arm {arm}: y differs from arm 0"
            for _ in range(30):  # clocks up
                batches[0].run()
            torch.cuda.synchronize()
            times = {arm: [] for arm in ARMS}
            for r in range(args.rounds):
                for arm in (ARMS if r % 2 == 0 else ARMS[::-1]):
                    batches[arm].run()
                    e0.record()
                    for _ in range(args.reps):
                        batches[arm].run()
                    e1.record()
                    torch.cuda.synchronize()
                    times[arm].append(e0.elapsed_time(e1) / args.reps * 1e3)
            base = statistics.median(times[0])
            result["ab"][dts] = {}
            for arm in ARMS:
                t = times[arm]
                med = statistics.median(t)
                print(f"{dts} RSP_SPMV_PACK={arm}: median {med:8.2f} us  min {min(t):8.2f}  max {max(t):8.2f}  "
                      f"spread {100 * (max(t) - min(t)) / med:5.2f} %  gain vs 0 {100 * (base / med - 1):+6.2f} %  "
                      f"rounds {' '.join(f'{v:.1f}' for v in t)}", flush=True)
                result["ab"][dts][arm] = {"median_us": med, "min_us": min(t), "max_us": max(t), "rounds_us": t}
            for b in batches.values():
                b.close()
            del batches, keep, dev, xs, ys
            torch.cuda.empty_cache()
        h.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
