#!/usr/bin/env python
"""Times the BSI aggregates on config 5's shape (generate_bsi(64, 100_000_000)) on one MI355X, one process.

bsi_sum (the fused k_bsi_sum pass) next to the composed path a caller had before it — one
rbgpu_pairwise_cardinality(AND) call of 64 (slice, found) pairs, whose code this aggregate does not touch — with
found = None (ebM) and found = the result of a RANGE compare; the two paths alternate inside one timed loop and
their sums are compared.  Then bsi_topk at k = 10, 10^4 and 10^7.  Kernel times are the library's device events
(rb_stats), wall times a host clock around calls that end in a stream wait.  There is no CPU fallback: without a
GPU the context fails to open.

    python scripts/bsi_agg_bench.py [--steps 20] [--warmup 3] [--out profiles/bsi_agg/bsi_agg_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NSLICES, NROWS = 64, 100_000_000
LO, HI = 0x3A00_0000_0000_0000, 0xB100_0000_0000_0000  # bench.py's config-5 RANGE window
PEAK_BYTES_PER_S = 8e12                                 # MI355X HBM3E peak
M64 = 2**64 - 1


def med(xs):
    return float(statistics.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nslices", type=int, default=NSLICES)
    ap.add_argument("--nrows", type=int, default=NROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsi_agg", "bsi_agg_bench.json"))
    args = ap.parse_args()
    import roaringbitmap_amd as rb

    ns = args.nslices
    out = {"shape": f"generate_bsi({ns}, {args.nrows})", "steps": args.steps, "warmup": args.warmup, "sum": {},
           "topk": {}}
    with rb.Context(0) as ctx:
        d = ctx.generate_bsi(ns, args.nrows, seed=42)
        vmax = (1 << ns) - 1
        ranged = ctx.bsi_compare(rb.BSI_RANGE, d, LO & vmax, HI & vmax, 0, vmax)
        ranged.wait()
        slices = list(range(ns))
        for name, f in (("found=None", None), ("found=RANGE", ranged)):
            def fused():
                t0 = time.perf_counter()
                r = ctx.bsi_sum(d, f)
                wall = (time.perf_counter() - t0) * 1e3
                st = ctx.stats()
                return r, wall, st

            def composed():
                t0 = time.perf_counter()
                c = ctx.pairwise_cardinality(rb.AND, d, d if f is None else f, slices, [ns if f is None else 0] * ns)
                wall = (time.perf_counter() - t0) * 1e3
                st = ctx.stats()
                return c, wall, st

            rows = {"fused": [], "composed": []}
            for it in range(args.warmup + args.steps):
                r, fw, fs = fused()
                c, cw, cs = composed()
                if sum(int(c[i]) << i for i in range(ns)) & M64 != r[0]:
                    raise SystemExit(f"{name}: the fused sum and the composed counts disagree")
                if it >= args.warmup:
                    rows["fused"].append((fw, fs["main_kernel_ms"], fs["input_bytes"], fs["total_ms"]))
                    rows["composed"].append((cw, cs["main_kernel_ms"], cs["input_bytes"], cs["total_ms"]))
            res = {"sum": r[0], "count": r[1], "keys_walked": fs["tasks"]}
            for k, v in rows.items():
                kms, b = med([x[1] for x in v]), int(v[-1][2])
                res[k] = {"wall_ms": med([x[0] for x in v]), "wall_ms_min": min(x[0] for x in v),
                          "wall_ms_max": max(x[0] for x in v), "device_total_ms": med([x[3] for x in v]),
                          "main_kernel": (fs if k == "fused" else cs)["main_kernel"], "main_kernel_ms": kms,
                          "algorithmic_bytes": b,
                          "fraction_of_8TBps_peak": (b / (kms * 1e-3) / PEAK_BYTES_PER_S) if kms > 0 else None}
            res["composed_over_fused_wall"] = res["composed"]["wall_ms"] / res["fused"]["wall_ms"]
            res["composed_over_fused_device"] = res["composed"]["device_total_ms"] / res["fused"]["device_total_ms"]
            out["sum"][name] = res
        fcard = int(ranged.cardinalities()[0])
        for k in (10, 10**4, 10**7):
            walls, kern = [], []
            for it in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                r = ctx.bsi_topk(d, ranged, k)
                w = (time.perf_counter() - t0) * 1e3
                st = ctx.stats_raw()
                if it >= args.warmup:
                    walls.append(w)
                    kern.append([float(st.kernel_ms[i]) for i in range(int(st.n_kernels))])
            out["topk"][f"k={k}"] = {
                "found_cardinality": fcard, "result_cardinality": int(r.cardinalities()[0]),
                "wall_ms": med(walls), "wall_ms_min": min(walls), "wall_ms_max": max(walls),
                "descent_ms": med([x[0] for x in kern]), "emit_ms": med([x[1] for x in kern]),
                # fixed by the code: one count launch per slice, one emit, the found set's key list
                # (index, active, scan, list) and the keyed compaction (keep, scan, write); one read-back in phase A
                "launches": {"descent": ns, "emit": 1, "key_list": 4, "compaction": 3, "total": ns + 8}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
