"""Run lists shared by test_light_stage_model.py (numpy model) and test_gpu_light_stage.py (device): the
shapes at which the staging of a Run as a toggle image, the carry fold and the parity probe can go wrong.
A run list is a sorted list of (start, end) pairs, end inclusive, runs not adjacent (canonical)."""
import numpy as np


def random_runs(nruns, seed):
    """nruns canonical runs from 2 * nruns distinct sorted positions in [0, 65536]: (p0, p1 - 1), (p2, p3 - 1) ..."""
    rng = np.random.default_rng(seed)
    p = np.sort(rng.choice(65537, 2 * nruns, replace=False)).astype(np.int64)
    return [(int(p[2 * i]), int(p[2 * i + 1]) - 1) for i in range(nruns)]


def run_lists():
    """(name, runs): at most 2047 runs each (a payload of at most 8 KiB)."""
    out = [
        ("full", [(0, 65535)]),
        ("first_and_last", [(0, 9), (65000, 65535)]),                    # starts at 0; its end + 1 = 65536 is dropped
        ("even2047", [(2 * i, 2 * i) for i in range(2047)]),
        # start / end + 1 on bits 31|32, 63|64, 127|128 (lane boundary) and 8191|8192 (row boundary)
        ("edges_single", [(31, 31), (63, 63), (127, 127), (8191, 8191)]),
        ("edges_wide", [(32, 62), (64, 126), (128, 8190), (8192, 8300)]),
        ("edges_across", [(20, 40), (60, 130), (8000, 9000), (16383, 16384)]),
    ]
    for n in (1, 4, 5, 255, 256, 257, 2047):
        out.append((f"random{n}", random_runs(n, 1000 + n)))
    return out


def big_run_lists():
    """More than 2047 runs, which no runOptimize'd bitmap holds.  2048 runs are exactly 8 KiB in the set layout (the
    run count lives in the metadata): the last size staged through the registers.  From 2049 runs on the payload
    is over 8 KiB and staged straight from global memory."""
    return [
        ("big2048", [(3 + 31 * i, 3 + 31 * i + 4) for i in range(2048)]),
        ("big2049", [(1 + 31 * i, 1 + 31 * i + 5) for i in range(2049)]),
        ("big3000_to_end", [(21 * i, 21 * i + 6) for i in range(2999)] + [(65000, 65535)]),
        ("big_random5000", random_runs(5000, 77)),
    ]


def run_values(runs):
    return np.concatenate([np.arange(s, e + 1, dtype=np.uint32) for s, e in runs])


def edge_probe_values(runs, limit=4096):
    """start - 1, start, end, end + 1 of every run, clipped to 0..65535, at most `limit` values (evenly thinned)."""
    v = []
    for s, e in runs:
        v += [s - 1, s, e, e + 1]
    v = np.unique(np.clip(np.array(v, np.int64), 0, 65535)).astype(np.uint32)
    if len(v) > limit:
        v = v[np.unique(np.linspace(0, len(v) - 1, limit).astype(np.int64))]
    return v
