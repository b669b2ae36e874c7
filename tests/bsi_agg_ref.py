"""Reference restatements of the BSI aggregates (a helper, not a test).

ref_sum / ref_topk restate Roaring64BitmapSliceIndex.sum / topK
(bsi/src/main/java/org/roaringbitmap/bsi/longlong/Roaring64BitmapSliceIndex.java:559-594) line by line over the
oracle's pieces (R = oracle.rbref: op, op_inplace, op_cardinality, RefBitmap.clone); the slices, the found set and
every intermediate are oracle bitmaps, so the result carries the reference's container types.  model_sum /
model_topk are independent value models in plain numpy / Python ints."""
import numpy as np

M64 = 2**64 - 1


def _empty(R):
    return R.RefBitmap.of(np.zeros(0, np.uint32))


def ref_sum(R, slices, found):
    """sum(foundSet) -> (sum mod 2^64, count)."""
    if found is None or found.cardinality() == 0:          # :560-562
        return 0, 0
    count = found.cardinality()                            # :563
    s = sum((1 << x) * R.op_cardinality(R.AND, slices[x], found) for x in range(len(slices)))  # :565-567
    return s & M64, count                                  # a Java long keeps the low 64 bits


def ref_topk(R, slices, found, k):
    """topK(foundSet, k)."""
    if found is None or found.cardinality() == 0:          # :573-575
        return _empty(R)
    if k >= found.cardinality():                           # :576-578
        return found
    re = _empty(R)                                         # :579
    cand = found.clone()                                   # :580
    x = len(slices) - 1
    while x >= 0 and cand.cardinality() > 0 and k > 0:     # :582
        t = R.op(R.AND, cand, slices[x])                   # :583
        c = t.cardinality()
        if c > k:
            R.op_inplace(R.AND, cand, slices[x])           # :586
        else:
            R.op_inplace(R.OR, re, t)                      # :588
            R.op_inplace(R.ANDNOT, cand, slices[x])        # :589
            k -= c                                         # :590
        x -= 1
    return re


def bitmap_pin_case():
    """(cols, vals, found rows, k, key): the case that separates Container.ior from the static or.  All 65536 rows
    of high key 1 are in found, 61440 with value 2 and 4096 with value 1; keys 0, 2 and 3 hold value 0 only;
    k = 65536.  topK emits and(cand, bA[1]) (a Bitmap of 61440) and then ors and(cand, bA[0]) (an Array of 4096)
    into it: BitmapContainer.ior(ArrayContainer) keeps the Bitmap, now of cardinality 65536, where the static or
    would return a full Run."""
    key1 = np.arange(65536, 131072, dtype=np.uint64)
    others = np.concatenate([np.arange(100, 200), 2 * 65536 + np.arange(0, 300, 3), 3 * 65536 + np.arange(50, 150)])
    cols = np.sort(np.concatenate([key1, others.astype(np.uint64)]))
    vals = np.zeros(len(cols), np.uint64)
    in1 = (cols >> np.uint64(16)) == 1
    vals[in1] = 2
    vals[in1 & ((cols & np.uint64(0xFFFF)) >= 61440)] = 1
    return cols, vals, cols.astype(np.uint32), 65536, 1


def found_values(cols, vals, rows):
    """The value of every row of `rows` (sorted unique): the index's value where the row is in cols (sorted
    unique), else 0 — a row outside ebM has no bit in any slice."""
    cols = np.asarray(cols, np.uint64)
    rows = np.asarray(rows, np.uint64)
    out = np.zeros(len(rows), np.uint64)
    if len(cols):
        pos = np.minimum(np.searchsorted(cols, rows), len(cols) - 1)
        hit = cols[pos] == rows
        out[hit] = np.asarray(vals, np.uint64)[pos[hit]]
    return out


def model_sum(cols, vals, rows):
    """(sum of the values of rows in found AND ebM, mod 2^64; |found|) in Python ints."""
    return sum(int(v) for v in found_values(cols, vals, rows)) & M64, len(rows)


def model_topk(cols, vals, rows, k):
    """The rows topK keeps: with v* the k-th largest value over found, {v >= v*} when that set has exactly k rows,
    else {v > v*} (the descent never splits a tie); found itself when k >= |found|, nothing when k == 0."""
    rows = np.asarray(rows, np.uint64)
    if k >= len(rows):
        return rows.astype(np.uint32)
    if k <= 0:
        return np.zeros(0, np.uint32)
    v = found_values(cols, vals, rows)
    vstar = np.sort(v)[::-1][k - 1]
    ge = rows[v >= vstar]
    return (ge if len(ge) == k else rows[v > vstar]).astype(np.uint32)
