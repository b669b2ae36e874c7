#!/usr/bin/env python
"""Times the value build (rbgpu_set_from_values_device / rbgpu_bsi_from_pairs) on one MI355X, one process.

Rebuilds, from uint32 ids already in HBM (a torch buffer filled by rbgpu_set_values_device), with runOptimize:
the decoded ids of config 2's batched AND result (generate(WL_FILTER_POSTING, --pairs), then pairwise(AND)) up to
--max-values, a Run-heavy set (WL_WIDE_RUNS), and one bitmap of --shuffled random ids in no order (the only one of the
three that sorts).  For each: the call's device time (rb_stats total_ms: every kernel, scan and read-back wait of the
call), the two k_set_build passes, the wall time, and the share of the 8 TB/s peak by the call's own byte count (4 B
per value in, payload + 16 B per container out) over the call's device time.  Each rebuilt set's cardinalities are
compared with the source's.

Then, at a size the host path finishes in seconds, the device build next to the path a caller had before it —
Context.upload_values (soa_from_values on the host, then an upload), code this feature does not touch — alternating
inside one timed loop, their serialized bytes compared.  The same for a BSI: Roaring64BitmapSliceIndex.from_pairs next
to setValues(pairs) + the first query's host build (_device()).  Kernel times are the library's device events
(rb_stats), wall times a host clock around calls that end in a stream wait.  There is no CPU fallback: without a GPU
the context fails to open.

    python scripts/set_build_bench.py [--steps 10] [--warmup 2] [--out profiles/set_build/set_build_bench.json]
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


def time_rebuild(ctx, ptr, offs, want_cards, warmup, steps):
    """rbgpu_set_from_values_device(RB_BUILD_RUN_OPTIMIZE) over the ids at ptr."""
    walls, calls, kms = [], [], []
    for it in range(warmup + steps):
        t0 = time.perf_counter()
        d = ctx.build_values_device(ptr, offs, run_optimize=True)
        w = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
        if it == 0 and not np.array_equal(d.cardinalities(), want_cards):
            raise SystemExit("the rebuilt set's cardinalities differ from the source's")
        if it >= warmup:
            walls.append(w)
            calls.append(st["total_ms"])
            kms.append(sum(k["ms"] for k in st["kernels"] if k["name"] == "k_set_build"))
        mix = d.type_stats() if it == 0 else mix
        del d
    assert st["main_kernel"] == "k_set_build"
    b = int(st["input_bytes"] + st["output_bytes"])
    c = med(calls)
    return dict(spread(walls, "wall_ms"), **spread(calls, "call_device_ms"), **spread(kms, "k_set_build_two_passes_ms"),
                bitmaps=len(offs) - 1, values=int(offs[-1] - offs[0]), containers=int(st["tasks"]), container_mix=mix,
                input_bytes=int(st["input_bytes"]), output_bytes=int(st["output_bytes"]), algorithmic_bytes=b,
                fraction_of_8TBps_peak=b / (c * 1e-3) / PEAK_BYTES_PER_S if c > 0 else None)


def decoded(torch, d, max_values):
    """The leading bitmaps of d that hold at most max_values members, decoded into a torch buffer."""
    offs = d.values_device(0, 0)
    count = max(int(np.searchsorted(offs, max_values, "right")) - 1, min(len(d), 1))
    total = int(offs[count])
    buf = torch.empty(max(total, 1), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    d.values_device(buf.data_ptr(), total, 0, count)
    return buf, offs[:count + 1].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--wide-bitmaps", type=int, default=8)
    ap.add_argument("--shuffled", type=int, default=1 << 26)
    ap.add_argument("--composed-pairs", type=int, default=3_000)
    ap.add_argument("--bsi-rows", type=int, default=300_000)
    ap.add_argument("--max-values", type=int, default=1 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_build", "set_build_bench.json"))
    args = ap.parse_args()
    import torch

    import roaringbitmap_amd as rb

    n_it = args.warmup + args.steps
    out = {"steps": args.steps, "warmup": args.warmup, "rebuild": {}, "composed": {}, "bsi": {}}
    with rb.Context(0) as ctx:
        # ---- the three rebuilds from ids in HBM
        a, b = ctx.generate(rb.WL_FILTER_POSTING, args.pairs, seed=42)
        res = ctx.pairwise(rb.AND, a, b)
        del a, b
        buf, offs = decoded(torch, res, args.max_values)
        cards = res.cardinalities()[:len(offs) - 1]
        del res
        out["rebuild"][f"ids of pairwise(AND) of generate(WL_FILTER_POSTING, {args.pairs})"] = \
            time_rebuild(ctx, buf.data_ptr(), offs, cards, args.warmup, args.steps)
        del buf
        s, _ = ctx.generate(rb.WL_WIDE_RUNS, args.wide_bitmaps, seed=42)
        buf, offs = decoded(torch, s, args.max_values)
        cards = s.cardinalities()[:len(offs) - 1]
        del s
        out["rebuild"][f"ids of generate(WL_WIDE_RUNS, {args.wide_bitmaps})"] = \
            time_rebuild(ctx, buf.data_ptr(), offs, cards, args.warmup, args.steps)
        del buf
        g = torch.Generator(device="cuda:0")
        g.manual_seed(7)
        buf = torch.randint(0, 1 << 28, (args.shuffled,), dtype=torch.int32, device="cuda:0", generator=g)
        cards = np.array([int(torch.unique(buf).numel())], np.uint64)
        torch.cuda.synchronize()
        out["rebuild"][f"one bitmap of {args.shuffled} random ids below 2^28, unsorted"] = \
            time_rebuild(ctx, buf.data_ptr(), np.array([0, args.shuffled], np.uint64), cards, args.warmup, args.steps)
        del buf
        # ---- the device build next to upload_values, from host arrays
        a, b = ctx.generate(rb.WL_FILTER_POSTING, args.composed_pairs, seed=42)
        bitmaps = ctx.pairwise(rb.AND, a, b).to_arrays()
        del a, b
        dev_w, host_w = [], []
        for it in range(n_it):
            t0 = time.perf_counter()
            dev = ctx.build_values(bitmaps, run_optimize=True)
            dw = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            host = ctx.upload_values(bitmaps, run_optimize=True)
            hw = (time.perf_counter() - t0) * 1e3
            if it == 0 and dev.serialize() != host.serialize():
                raise SystemExit("the device build and upload_values disagree")
            if it >= args.warmup:
                dev_w.append(dw)
                host_w.append(hw)
            del dev, host
        out["composed"] = {"shape": f"to_arrays() of pairwise(AND) of generate(WL_FILTER_POSTING, {args.composed_pairs})",
                           "bitmaps": len(bitmaps), "values": int(sum(len(x) for x in bitmaps)),
                           "build_values": spread(dev_w, "wall_ms"), "upload_values": spread(host_w, "wall_ms"),
                           "host_over_device_wall": med(host_w) / med(dev_w)}
        # ---- a BSI from pairs next to setValues + the host build
        rng = np.random.default_rng(3)
        cols = rng.permutation(np.arange(args.bsi_rows, dtype=np.uint32) * np.uint32(3))
        vals = rng.integers(0, 1 << 32, args.bsi_rows).astype(np.uint64)
        dev_w, stage_w, host_w, calls, kms = [], [], [], [], []
        for it in range(n_it):
            t0 = time.perf_counter()
            dev = rb.Roaring64BitmapSliceIndex.from_pairs(cols, vals, run_optimize=True)
            dw = (time.perf_counter() - t0) * 1e3
            st = ctx_stats(rb)
            nbm = len(dev._device())
            t0 = time.perf_counter()
            host = rb.Roaring64BitmapSliceIndex()
            host.setValues(zip(cols.tolist(), vals.tolist()))
            host.runOptimize()
            sw = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            hd = host._device()
            hw = (time.perf_counter() - t0) * 1e3
            if it == 0 and (dev._device().serialize() != hd.serialize() or
                            (dev.minValue, dev.maxValue) != (host.minValue, host.maxValue)):
                raise SystemExit("from_pairs and the host-built index disagree")
            if it >= args.warmup:
                dev_w.append(dw)
                stage_w.append(sw)
                host_w.append(hw)
                calls.append(st["total_ms"])
                kms.append(sum(k["ms"] for k in st["kernels"] if k["name"] == "k_set_build"))
            del dev, host, hd
        bts = int(st["input_bytes"] + st["output_bytes"])
        out["bsi"] = {"rows": args.bsi_rows, "value_bits": 32, "containers": int(st["tasks"]),
                      "from_pairs": dict(spread(dev_w, "wall_ms"), **spread(calls, "call_device_ms"),
                                         **spread(kms, "k_set_build_two_passes_ms")),
                      # each of the two passes reads a key's columns once per bitmap and its values once per slice
                      "bitmaps": nbm, "pair_bytes_read_by_k_set_build": 2 * args.bsi_rows * (4 * nbm + 8 * (nbm - 1)),
                      "algorithmic_bytes": bts,
                      "fraction_of_8TBps_peak": bts / (med(calls) * 1e-3) / PEAK_BYTES_PER_S,
                      "setValues_host_staging": spread(stage_w, "wall_ms"),
                      "host_build_and_upload": spread(host_w, "wall_ms"),
                      "host_build_over_from_pairs_wall": med(host_w) / med(dev_w),
                      "staging_and_host_build_over_from_pairs_wall": (med(host_w) + med(stage_w)) / med(dev_w)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


def ctx_stats(rb):
    """rb_stats of the default context's last call (the BSI mirror runs on it)."""
    return rb.default_context().stats()


if __name__ == "__main__":
    main()
