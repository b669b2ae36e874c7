#!/usr/bin/env python
"""Times the BSI value read-back on config 5's shape (generate_bsi(64, 100_000_000)) on one MI355X, one process.

Export (rbgpu_bsi_values_device into torch buffers) with found = None (every row: 1.2 GB out), found = the result of
a RANGE compare (about half the rows) and found = 10 000 scattered rows (the tile skip).  Then, at a size where it
finishes in seconds, the device export next to the path a caller had before it — download() of the whole index and
a numpy decode on the host, code this feature does not touch — alternating inside one timed loop, their answers
compared.  Then bsi_get_values for 1, 1 000 and 1 000 000 random columns.  Kernel times are the library's device
events (rb_stats), wall times a host clock around calls that end in a stream wait.  There is no CPU fallback: without
a GPU the context fails to open.

    python scripts/bsi_values_bench.py [--steps 20] [--warmup 3] [--out profiles/bsi_values/bsi_values_bench.json]
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

NSLICES, NROWS, COMPOSED_ROWS = 64, 100_000_000, 1_000_000
LO, HI = 0x3A00_0000_0000_0000, 0xB100_0000_0000_0000  # bench.py's config-5 RANGE window
PEAK_BYTES_PER_S = 8e12                                 # MI355X HBM3E peak


def med(xs):
    return float(statistics.median(xs))


def spread(xs, unit):
    return {f"wall_{unit}": med(xs), f"wall_{unit}_min": min(xs), f"wall_{unit}_max": max(xs)}


def host_decode(h, ns):
    """(cols, vals) from a downloaded index (slices then ebM): every slice's rows looked up in ebM's."""
    cols = h.values(ns)
    vals = np.zeros(len(cols), np.uint64)
    for i in range(ns):
        vals[np.searchsorted(cols, h.values(i))] |= np.uint64(1 << i)
    return cols, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nslices", type=int, default=NSLICES)
    ap.add_argument("--nrows", type=int, default=NROWS)
    ap.add_argument("--composed-rows", type=int, default=COMPOSED_ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsi_values", "bsi_values_bench.json"))
    args = ap.parse_args()
    import torch

    import roaringbitmap_amd as rb

    ns, n_it = args.nslices, args.warmup + args.steps
    out = {"shape": f"generate_bsi({ns}, {args.nrows})", "steps": args.steps, "warmup": args.warmup, "export": {},
           "composed": {}, "lookup": {}}
    rng = np.random.default_rng(1)
    with rb.Context(0) as ctx:
        d = ctx.generate_bsi(ns, args.nrows, seed=42)
        vmax = (1 << ns) - 1
        ranged = ctx.bsi_compare(rb.BSI_RANGE, d, LO & vmax, HI & vmax, 0, vmax)
        ranged.wait()
        scattered = ctx.upload_values([np.unique(rng.integers(0, args.nrows, 10_000)).astype(np.uint32)])
        tc = torch.empty(args.nrows, dtype=torch.int32, device="cuda:0")
        tv = torch.empty(args.nrows, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        for name, f in (("found=None", None), ("found=RANGE", ranged), ("found=10000 rows", scattered)):
            walls, kb, ka = [], [], []
            for it in range(n_it):
                t0 = time.perf_counter()
                n = ctx.bsi_values_device(d, tc.data_ptr(), tv.data_ptr(), args.nrows, found=f)
                w = (time.perf_counter() - t0) * 1e3
                st = ctx.stats()
                if it >= args.warmup:
                    walls.append(w)
                    kb.append(st["kernels"][0]["ms"])
                    ka.append(st["kernels"][1]["ms"])
            assert st["main_kernel"] == "k_bsi_values" and st["output_bytes"] == 12 * n
            b, kms = int(st["input_bytes"] + st["output_bytes"]), med(kb)
            out["export"][name] = dict(spread(walls, "ms"), rows=n, keys_walked=int(st["tasks"]), k_bsi_values_ms=kms,
                                       phase_a_ms=med(ka), phase_a_share=med(ka) / (med(ka) + kms),
                                       algorithmic_bytes=b,
                                       fraction_of_8TBps_peak=b / (kms * 1e-3) / PEAK_BYTES_PER_S if kms > 0 else None)
        # ---- the device export next to download() + a host decode, at a size the host path finishes in seconds
        s = ctx.generate_bsi(ns, args.composed_rows, seed=42)
        dev_w, host_w = [], []
        for it in range(n_it):
            t0 = time.perf_counter()
            n = ctx.bsi_values_device(s, tc.data_ptr(), tv.data_ptr(), args.nrows)
            dw = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            hc, hv = host_decode(s.download(), ns)
            hw = (time.perf_counter() - t0) * 1e3
            if it == 0:
                gc, gv = tc[:n].cpu().numpy().view(np.uint32), tv[:n].cpu().numpy().view(np.uint64)
                if not (np.array_equal(gc, hc) and np.array_equal(gv, hv)):
                    raise SystemExit("the device export and the host decode disagree")
            if it >= args.warmup:
                dev_w.append(dw)
                host_w.append(hw)
        out["composed"] = {"shape": f"generate_bsi({ns}, {args.composed_rows})", "rows": n,
                           "device_export": spread(dev_w, "ms"), "download_and_host_decode": spread(host_w, "ms"),
                           "host_over_device_wall": med(host_w) / med(dev_w)}
        # ---- point lookups
        for nq in (1, 1_000, 1_000_000):
            q = rng.integers(0, args.nrows + args.nrows // 8, nq).astype(np.uint32)
            walls, kms = [], []
            for it in range(n_it):
                t0 = time.perf_counter()
                v, e = ctx.bsi_get_values(d, q)
                w = (time.perf_counter() - t0) * 1e6
                if it >= args.warmup:
                    walls.append(w)
                    kms.append(ctx.stats()["main_kernel_ms"])
            out["lookup"][f"n={nq}"] = dict(spread(walls, "us"), us_per_query=med(walls) / nq,
                                            k_bsi_get_us=med(kms) * 1e3, found=int(e.sum()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
