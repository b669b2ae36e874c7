#!/usr/bin/env python
"""Times Roaring64BitmapSliceIndex.add on the device (rbgpu_bsi_add) on one MI355X, one process, and — apart from it,
never inside the same timed loop — the two routes a caller had before.

Input: two generate_bsi(--slices, --rows) indexes with different seeds (every row in both: every (slice, key) pair is
combined), and a second pair over disjoint key ranges (the merge shape: every container is a copy).  One route per
invocation (--route), so that each can run under a time limit of its own; every timed call prints one line as it ends,
and the medians (with min and max) are merged into --out under the route's name:

  fused   ctx.bsi_add: wall time, the call's device time (rb_stats total_ms: the slice passes, not ebM's union before
          them nor the min / max pass after), its measuring and emitting spans, and the share of the 8 TB/s peak by the
          call's own byte count (payload + 16 B of every slice container read and of every result container) over
          that device time.  On the disjoint pair ctx.bsi_merge is timed too (wall time only: it is a sequence of
          library calls).
  chain   the same call with RB_BSI_ADD_CHAIN: the reference's per-digit and / in-place xor over the pairwise entry
          points, the only device route a caller could have assembled before.  Wall time.
  host    toPairList of both indexes, numpy addition, from_pairs of the sums; at most 3 steps.

Kernel times are the library's device events (rb_stats), wall times a host clock around calls that end in a stream
wait.  There is no CPU fallback: without a GPU the context fails to open.

    python scripts/bsi_arith_bench.py --route fused [--slices 32] [--rows 10000000] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E peak


def med(xs):
    return float(statistics.median(xs))


def spread(xs, name):
    return {name: med(xs), name + "_min": min(xs), name + "_max": max(xs)}


def say(**kw):
    print(json.dumps(kw, sort_keys=True), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["fused", "chain", "host"], required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsi_arith", "bsi_arith_bench.json"))
    args = ap.parse_args()

    import roaringbitmap_amd as rb

    keys = (args.rows + 65535) >> 16
    res = {"steps": args.steps, "warmup": args.warmup, "slices": args.slices, "rows": args.rows, "cases": {}}
    with rb.Context(0) as ctx:
        pairs = {
            "overlap": (ctx.generate_bsi(args.slices, args.rows, seed=1), ctx.generate_bsi(args.slices, args.rows, seed=2)),
            "disjoint": (ctx.generate_bsi(args.slices, args.rows, seed=1, key_range=(0, keys // 2)),
                         ctx.generate_bsi(args.slices, args.rows, seed=2, key_range=(keys // 2, keys))),
        }
        for name, (a, b) in pairs.items():
            say(route=args.route, pair=name, a_containers=a.n_containers, b_containers=b.n_containers,
                a_mix=a.type_stats(), b_mix=b.type_stats())
            ops = ["add"] + (["merge"] if args.route == "fused" and name == "disjoint" else [])
            for op in ops:
                walls, calls, k_m, k_e = [], [], [], []
                steps = min(args.steps, 3) if args.route == "host" else args.steps
                st, d = None, None
                for it in range(args.warmup + steps):
                    t0 = time.perf_counter()
                    if op == "merge":
                        d = ctx.bsi_merge(a, b)
                    elif args.route == "host":
                        ca, va = ctx.bsi_values(a)
                        cb, vb = ctx.bsi_values(b)
                        cols = np.union1d(ca, cb)
                        vals = np.zeros(len(cols), np.uint64)
                        vals[np.searchsorted(cols, ca)] += va
                        vals[np.searchsorted(cols, cb)] += vb
                        d = ctx.bsi_build(cols, vals)[0]
                    else:
                        d = ctx.bsi_add(a, b, chain=args.route == "chain")[0]
                    w = (time.perf_counter() - t0) * 1e3
                    timed = args.route == "fused" and op == "add"
                    st = ctx.stats() if timed else None
                    if timed and not st["main_kernel"].startswith("k_bsi_add"):
                        # a Run at a shared key sent the call to the chain: its rb_stats are a pairwise call's
                        raise SystemExit(f"the planner took the chain on pair {name!r} (main kernel "
                                         f"{st['main_kernel']!r}): this input does not time the fused route")
                    say(route=args.route, pair=name, op=op, it=it, wall_ms=round(w, 3),
                        device_ms=round(st["total_ms"], 3) if timed else None,
                        main_kernel=st["main_kernel"] if timed else None)
                    if it >= args.warmup:
                        walls.append(w)
                        if timed:
                            calls.append(st["total_ms"])
                            k_m.append(st["kernels"][0]["ms"])
                            k_e.append(st["kernels"][1]["ms"])
                    if it == 0:
                        shape = {"bitmaps": len(d), "containers": d.n_containers, "mix": d.type_stats()}
                    del d
                case = dict(spread(walls, "wall_ms"), result=shape)
                if calls:
                    nbytes = int(st["input_bytes"] + st["output_bytes"])
                    case.update(spread(calls, "call_device_ms"), **spread(k_m, "measure_ms"), **spread(k_e, "emit_ms"),
                                main_kernel=st["main_kernel"], keys_walked=int(st["tasks"]), input_bytes=int(st["input_bytes"]),
                                output_bytes=int(st["output_bytes"]), algorithmic_bytes=nbytes,
                                fraction_of_8TBps_peak=nbytes / (med(calls) * 1e-3) / PEAK_BYTES_PER_S,
                                emit_fraction_of_8TBps_peak=nbytes / (med(k_e) * 1e-3) / PEAK_BYTES_PER_S)
                res["cases"][f"{op} {name}"] = case
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged[args.route] = res
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    say(route=args.route, written=os.path.relpath(args.out, ROOT))


if __name__ == "__main__":
    main()
