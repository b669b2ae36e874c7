#!/usr/bin/env python
"""Times the range mutations (rbgpu_set_range_op: RoaringBitmap.add / remove / flip over [start, end)) on one MI355X,
one process, and — apart from them, never inside the same timed loop — the two routes a caller had before.

Input: generate(WL_WIDE_MIXED, --bitmaps) (70 % Bitmap / 20 % Array / 10 % Run containers, a key with probability
1/16), every bitmap under the same range: a key-sized one, [0, 65536), and the whole universe, [0, 2^32).  One route
per invocation (--route), so that each can run under a time limit of its own; every timed call prints one line as it
ends, and the medians (with min and max) are merged into --out under the route's name:

  range_op   ctx.range_op: wall time, the call's device time (rb_stats total_ms), its measuring and emitting spans,
             and the share of the 8 TB/s peak by the call's own byte count (payload + 16 B of every source container
             copied or edited, payload + 16 B of every result container) over the call's device time.
  pairwise   baseline 1, the only device route before: pairwise(OR | ANDNOT | XOR) of every bitmap against one
             pre-uploaded range bitmap (tests/datasets.range_bitmap_bytes).  The same SETS, other container types;
             its results' cardinalities are written beside range_op's for comparison.
  host       baseline 2: download() of ONE bitmap, its decode into per-container values, and the reference
             restatement of the op on the host (tests/range_ops_ref.py), at most 3 steps; re-encoding and uploading
             the result, which a caller would also pay, is not included.

Kernel times are the library's device events (rb_stats), wall times a host clock around calls that end in a stream
wait.  There is no CPU fallback: without a GPU the context fails to open.

    python scripts/range_ops_bench.py --route range_op [--bitmaps 16] [--ranges key,universe] [--steps 10] [--warmup 2]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E peak
RANGES = {"key": ("key [0, 65536)", 0, 1 << 16), "universe": ("universe [0, 2^32)", 0, 1 << 32)}


def med(xs):
    return float(statistics.median(xs))


def spread(xs, name):
    return {name: med(xs), name + "_min": min(xs), name + "_max": max(xs)}


def say(**kw):
    print(json.dumps(kw, sort_keys=True), flush=True)


def host_conts(h, b):
    """Bitmap b of a HostSoA as the restatement's [(key, type, values)]."""
    out = []
    for i in range(int(h.begin[b]), int(h.begin[b + 1])):
        p, t = h.container_payload(i), int(h.type[i])
        if t == 0:
            low = p.view(np.uint16).astype(np.uint32)
        elif t == 1:
            low = np.nonzero(np.unpackbits(p, bitorder="little"))[0].astype(np.uint32)
        else:
            rl = p.view(np.uint16).reshape(-1, 2).astype(np.int64)
            low = np.concatenate([np.arange(s, s + n + 1, dtype=np.uint32) for s, n in rl])
        out.append((int(h.key[i]), t, low))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["range_op", "pairwise", "host"], required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bitmaps", type=int, default=16)
    ap.add_argument("--ranges", default="key,universe")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_ops", "range_ops_bench.json"))
    args = ap.parse_args()

    import datasets
    import range_ops_ref as ref

    import roaringbitmap_amd as rb

    n = args.bitmaps
    ops = [("add", rb.RANGE_ADD, rb.OR), ("remove", rb.RANGE_REMOVE, rb.ANDNOT), ("flip", rb.RANGE_FLIP, rb.XOR)]
    res = {"steps": args.steps, "warmup": args.warmup, "bitmaps": n, "cases": {}}
    with rb.Context(0) as ctx:
        s, _ = ctx.generate(rb.WL_WIDE_MIXED, n, seed=42)
        res["input"] = {"containers": s.n_containers, "payload_bytes": s.payload_capacity, "mix": s.type_stats()}
        say(route=args.route, input=res["input"])
        for rkey in args.ranges.split(","):
            rname, start, end = RANGES[rkey]
            if args.route == "pairwise":
                rset = ctx.upload_serialized([datasets.range_bitmap_bytes(end)])
                a_idx, b_idx = np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32)
                say(route=args.route, range=rname, uploaded_range_containers=rset.n_containers)
            if args.route == "host":
                t0 = time.perf_counter()
                h = s.download(0, 1)
                dl = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                conts = host_conts(h, 0)
                dec = (time.perf_counter() - t0) * 1e3
                say(route=args.route, range=rname, download_ms=dl, decode_ms=dec, containers=len(conts))
            for oname, rop, pop in ops:
                walls, calls, k_m, k_e = [], [], [], []
                steps = min(args.steps, 3) if args.route == "host" else args.steps
                for it in range(args.warmup + steps):
                    t0 = time.perf_counter()
                    if args.route == "range_op":
                        d = ctx.range_op(rop, s, start, end)
                    elif args.route == "pairwise":
                        d = ctx.pairwise(pop, s, rset, a_idx, b_idx)
                    else:
                        d = ref.range_op(rop, conts, start, end)
                    w = (time.perf_counter() - t0) * 1e3
                    st = ctx.stats() if args.route != "host" else {"total_ms": 0.0, "kernels": []}
                    say(route=args.route, range=rname, op=oname, it=it, wall_ms=round(w, 3),
                        device_ms=round(st["total_ms"], 3))
                    if it >= args.warmup:
                        walls.append(w)
                        calls.append(st["total_ms"])
                        if args.route == "range_op":
                            k_m.append(st["kernels"][0]["ms"])
                            k_e.append(st["kernels"][1]["ms"])
                    if it == 0 and args.route != "host":
                        cards = [int(x) for x in d.cardinalities()]
                        mix = d.type_stats()
                    del d
                case = dict(spread(walls, "wall_ms"))
                if args.route == "host":
                    case.update(bitmaps=1, download_ms=dl, decode_ms=dec)
                else:
                    b = int(st["input_bytes"] + st["output_bytes"])
                    case.update(spread(calls, "call_device_ms"), result_mix=mix, result_cardinalities=cards,
                                input_bytes=int(st["input_bytes"]), output_bytes=int(st["output_bytes"]),
                                algorithmic_bytes=b)
                    if med(calls) > 0:
                        case["fraction_of_8TBps_peak"] = b / (med(calls) * 1e-3) / PEAK_BYTES_PER_S
                if args.route == "range_op":
                    case.update(spread(k_m, "measure_ms"), **spread(k_e, "emit_ms"),
                                result_containers=int(st["result_containers"]))
                res["cases"][f"{oname} {rname}"] = case
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
