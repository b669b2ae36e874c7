#!/usr/bin/env python
"""Times the value read-out of plain sets (rbgpu_set_values_device / contains / rank / select) on one MI355X, one
process.

Decode (rbgpu_set_values_device into a torch buffer) over the result of config 2's batched AND
(generate(WL_FILTER_POSTING, 1_000_000), then pairwise(AND)), over a Bitmap-heavy set (WL_WIDE_DENSE) and over a
Run-heavy set (WL_WIDE_RUNS): the kernel time from rb_stats and its share of the 8 TB/s peak by the call's own
accounting (payload + 16 B per container read, 4 B per member written).  A set whose members exceed --max-values is
decoded up to the last whole bitmap below it.  Then, at a size where it finishes in seconds, the device read-out
next to the path a caller had before it — download() of the payload arena and HostSoA.values on the host, code this
feature does not touch — alternating inside one timed loop, their answers compared.  Then contains, rank and select
for 1, 1 000 and 1 000 000 random queries over the AND result.  Kernel times are the library's device events
(rb_stats), wall times a host clock around calls that end in a stream wait.  There is no CPU fallback: without a GPU
the context fails to open.

    python scripts/set_values_bench.py [--steps 20] [--warmup 3] [--out profiles/set_values/set_values_bench.json]
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


def spread(xs, unit):
    return {f"wall_{unit}": med(xs), f"wall_{unit}_min": min(xs), f"wall_{unit}_max": max(xs)}


def time_decode(ctx, torch, d, max_values, warmup, steps):
    """rbgpu_set_values_device over the leading bitmaps of d that hold at most max_values members."""
    offs = d.values_device(0, 0)
    count = max(int(np.searchsorted(offs, max_values, "right")) - 1, min(len(d), 1))  # one bitmap at the least
    total = int(offs[count])
    buf = torch.empty(max(total, 1), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    walls, kms = [], []
    for it in range(warmup + steps):
        t0 = time.perf_counter()
        got = d.values_device(buf.data_ptr(), total, 0, count)
        w = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
        if it >= warmup:
            walls.append(w)
            kms.append(st["main_kernel_ms"])
    assert st["main_kernel"] == "k_set_values" and int(got[count]) == total and st["output_bytes"] == 4 * total
    b, k = int(st["input_bytes"] + st["output_bytes"]), med(kms)
    res = dict(spread(walls, "ms"), bitmaps=count, bitmaps_in_set=len(d), containers=int(st["tasks"]), values=total,
               container_mix=d.type_stats(), k_set_values_ms=k, k_set_values_ms_min=min(kms), k_set_values_ms_max=max(kms),
               input_bytes=int(st["input_bytes"]), output_bytes=int(st["output_bytes"]), algorithmic_bytes=b,
               fraction_of_8TBps_peak=b / (k * 1e-3) / PEAK_BYTES_PER_S if k > 0 else None,
               prefix_setup=d.setup_stats())
    return res, buf, offs, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--wide-bitmaps", type=int, default=8)
    ap.add_argument("--composed-pairs", type=int, default=20_000)
    ap.add_argument("--max-values", type=int, default=1 << 31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_values", "set_values_bench.json"))
    args = ap.parse_args()
    import torch

    import roaringbitmap_amd as rb

    n_it = args.warmup + args.steps
    out = {"steps": args.steps, "warmup": args.warmup, "decode": {}, "composed": {}, "lookup": {}}
    rng = np.random.default_rng(1)
    with rb.Context(0) as ctx:
        # ---- the decode
        a, b = ctx.generate(rb.WL_FILTER_POSTING, args.pairs, seed=42)
        res = ctx.pairwise(rb.AND, a, b)
        name = f"pairwise(AND) of generate(WL_FILTER_POSTING, {args.pairs})"
        out["decode"][name], buf, offs, count = time_decode(ctx, torch, res, args.max_values, args.warmup, args.steps)
        for wl, label in ((rb.WL_WIDE_DENSE, "WL_WIDE_DENSE"), (rb.WL_WIDE_RUNS, "WL_WIDE_RUNS")):
            s, _ = ctx.generate(wl, args.wide_bitmaps, seed=42)
            out["decode"][f"generate({label}, {args.wide_bitmaps})"] = \
                time_decode(ctx, torch, s, args.max_values, args.warmup, args.steps)[0]
            del s
        # ---- the three lookups over the AND result: members of the decoded bitmaps and their neighbours
        total = int(offs[count])
        cards = np.diff(offs[:count + 1])
        for nq in (1, 1_000, 1_000_000):
            pos = np.sort(rng.integers(0, max(total, 1), nq))
            vals = buf[torch.from_numpy(pos).to("cuda:0")].cpu().numpy().view(np.uint32) if total else \
                np.zeros(nq, np.uint32)
            col = (np.searchsorted(offs[:count + 1], pos, "right") - 1).astype(np.uint32)
            vals = vals + (rng.integers(0, 2, nq)).astype(np.uint32)  # about half of them absent neighbours
            perm = rng.permutation(nq)
            vals, col = vals[perm], col[perm]
            js = (rng.random(nq) * (cards[col] + 1)).astype(np.uint64)
            entry = {}
            for kind, call in (("contains", lambda: res.contains(vals, bitmap=col)),
                               ("rank", lambda: res.rank(vals, bitmap=col)),
                               ("select", lambda: res.select(js, bitmap=col)[1])):
                walls, kms = [], []
                for it in range(n_it):
                    t0 = time.perf_counter()
                    r = call()
                    w = (time.perf_counter() - t0) * 1e6
                    if it >= args.warmup:
                        walls.append(w)
                        kms.append(ctx.stats()["main_kernel_ms"])
                assert ctx.stats()["main_kernel"] == "k_set_" + kind
                entry[kind] = dict(spread(walls, "us"), us_per_query=med(walls) / nq, kernel_us=med(kms) * 1e3,
                                   hits=int(np.count_nonzero(r)))
            out["lookup"][f"n={nq}"] = entry
        del buf, res, a, b
        # ---- the device read-out next to download() + HostSoA.values, at a size the host path finishes in seconds
        a, b = ctx.generate(rb.WL_FILTER_POSTING, args.composed_pairs, seed=42)
        s = ctx.pairwise(rb.AND, a, b)
        dev_w, host_w = [], []
        for it in range(n_it):
            t0 = time.perf_counter()
            dev = s.to_arrays()
            dw = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            h = s.download()
            host = [h.values(i) for i in range(len(s))]
            hw = (time.perf_counter() - t0) * 1e3
            if it == 0 and not all(np.array_equal(x, y) for x, y in zip(dev, host)):
                raise SystemExit("the device read-out and the host decode disagree")
            if it >= args.warmup:
                dev_w.append(dw)
                host_w.append(hw)
        out["composed"] = {"shape": f"pairwise(AND) of generate(WL_FILTER_POSTING, {args.composed_pairs})",
                           "containers": s.n_containers, "values": int(sum(len(x) for x in dev)),
                           "to_arrays": spread(dev_w, "ms"), "download_and_host_values": spread(host_w, "ms"),
                           "host_over_device_wall": med(host_w) / med(dev_w)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
