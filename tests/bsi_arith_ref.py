"""The reference's BSI arithmetic restated over the CPU oracle (oracle.rbref), for the tests of rbgpu_bsi_add /
rbgpu_bsi_merge / rbgpu_bsi_min_max.

An index is a pair (slices, ebm): a list of RefBitmap (bA[0..n)) and the existence bitmap.

  add        Roaring64BitmapSliceIndex.add / addDigit (longlong/Roaring64BitmapSliceIndex.java:64-93): per digit of the
             other index the static and (the carry) and the in-place xor, rippling upwards while the carry is not
             empty; ebM by the in-place or.  The oracle's bitmaps are RoaringBitmaps, whose xor drops a container that
             ends empty (RoaringBitmapSliceIndex.add, bsi/RoaringBitmapSliceIndex.java:66-95) — the form a device set
             can hold.
  merge      :357-383: the static or per slice, runOptimize when either side was run-optimised, ebM by the in-place or.
  min_max    :95-125: the descent over the slices, with the true unsigned value of the column it ends on (valueAt
             accumulates `1 << i` in an int and agrees for bitCount <= 31).
  add_model  the one-pass rule the fused kernel implements (DESIGN: BSI arithmetic): per high key a carry walks the
             slices once; a container no digit and no carry touches is copied as it is, every other one is the
             canonical Array / Bitmap of a ^ b ^ c, dropped when empty.  It holds where no Run container is touched.
"""
from __future__ import annotations

import numpy as np

from oracle import rbref

ARRAY, BITMAP, RUN = rbref.ARRAY, rbref.BITMAP, rbref.RUN
MAX_ARRAY = 4096


def empty():
    return rbref.RefBitmap.of(np.zeros(0, np.uint32))


def build(cols, vals, run_optimize: bool = False):
    """setValues on a fresh index, then runOptimize of every slice and of ebM when asked."""
    slices, ebm, _, _ = rbref.bsi_build(cols, vals)
    if run_optimize:
        for s in slices:
            s.run_optimize()
        ebm.run_optimize()
    return list(slices), ebm


def from_blobs(blobs):
    """An index from the serialized bitmaps of a device BSI (slices, then ebM)."""
    bm = [rbref.RefBitmap.deserialize(b) for b in blobs]
    return bm[:-1], bm[-1]


def blobs(index):
    slices, ebm = index
    return [s.serialize() for s in slices] + [ebm.serialize()]


def pairs(index):
    """(cols uint32 ascending, vals as Python ints) of the index."""
    slices, ebm = index
    cols = ebm.to_array()
    vals = [0] * len(cols)
    for i, s in enumerate(slices):
        for p in np.flatnonzero(np.isin(cols, s.to_array(), assume_unique=True)):
            vals[p] |= 1 << i
    return cols, vals


def add(a, b):
    """a.add(b) on clones; OverflowError where the reference would grow a 65th slice."""
    sa, ea = [s.clone() for s in a[0]], a[1].clone()
    sb, eb = b
    if eb.cardinality() == 0:
        return sa, ea
    rbref.op_inplace(rbref.OR, ea, eb)
    while len(sa) < len(sb):  # grow(otherBsi.bitCount())
        sa.append(empty())

    def add_digit(found, i):
        carry = rbref.op(rbref.AND, sa[i], found)
        rbref.op_inplace(rbref.XOR, sa[i], found)
        if carry.cardinality():
            if i + 1 >= len(sa):
                sa.append(empty())
            add_digit(carry, i + 1)

    for i in range(len(sb)):
        add_digit(sb[i], i)
    if len(sa) > 64:
        raise OverflowError("the sum needs a 65th slice")
    return sa, ea


def merge(a, b, run_optimize: bool = False):
    """a.merge(b) on clones; ValueError when the existence bitmaps intersect."""
    sa, ea = a
    sb, eb = b
    if eb.cardinality() == 0:
        return [s.clone() for s in sa], ea.clone()
    if rbref.op_cardinality(rbref.AND, ea, eb):
        raise ValueError("merge can be used only in bsiA  bsiB  is null")
    out = []
    for i in range(max(len(sa), len(sb))):
        r = rbref.op(rbref.OR, sa[i] if i < len(sa) else empty(), sb[i] if i < len(sb) else empty())
        if run_optimize:
            r.run_optimize()
        out.append(r)
    e = ea.clone()
    rbref.op_inplace(rbref.OR, e, eb)
    return out, e


def min_max(index):
    slices, ebm = index
    if ebm.cardinality() == 0:
        return 0, 0
    res = []
    for opcode in (rbref.ANDNOT, rbref.AND):
        m = ebm
        for i in range(len(slices) - 1, -1, -1):
            t = rbref.op(opcode, m, slices[i])
            if t.cardinality():
                m = t
        col = np.uint32(m.to_array()[0])
        one = rbref.RefBitmap.of([col])
        res.append(sum(1 << i for i, s in enumerate(slices) if rbref.op_cardinality(rbref.AND, s, one)))
    return res[0], res[1]


# ---- the one-pass rule ------------------------------------------------------------------------------------------
def _by_key(bm):
    """{key: (type, card, nruns, bool[65536])} of one bitmap."""
    vals = bm.to_array()
    out = {}
    for key, ty, card, nr in bm.containers():
        bits = np.zeros(65536, bool)
        lo, hi = np.searchsorted(vals, [key << 16, (key + 1) << 16])
        bits[vals[lo:hi] & 0xFFFF] = True
        out[key] = (ty, card, nr if ty == RUN else 0, bits)
    return out


def add_model(a, b):
    """[(per slice) [(key, type, card, nruns, values)]] of a.add(b)'s slices by the one-pass rule; the slice count
    follows the carry out of the top slice.  Not defined where a touched container is a Run."""
    sa, sb = a[0], b[0]
    if b[1].cardinality() == 0:
        n = len(sa)
    else:
        n = max(len(sa), len(sb))
    A = [_by_key(s) for s in sa] + [{} for _ in range(n + 1 - len(sa))]
    B = ([_by_key(s) for s in sb] if b[1].cardinality() else []) + [{}] * (n + 1)
    keys = sorted({k for t in A for k in t} | {k for t in B[:n + 1] for k in t})
    out = [[] for _ in range(n + 1)]
    zero = np.zeros(65536, bool)
    for key in keys:
        c = zero
        for j in range(n + 1):
            ca, cb = A[j].get(key), B[j].get(key)
            carried = bool(c.any())
            if cb is None and not carried:
                if ca is not None:
                    out[j].append((key, ca[0], ca[1], ca[2], np.flatnonzero(ca[3])))
                continue
            if ca is None and not carried:
                out[j].append((key, cb[0], cb[1], cb[2], np.flatnonzero(cb[3])))
                continue
            x = ca[3] if ca is not None else zero
            y = cb[3] if cb is not None else zero
            s = x ^ y ^ c
            c = (x & y) | (c & (x ^ y))
            card = int(s.sum())
            if card:
                out[j].append((key, ARRAY if card <= MAX_ARRAY else BITMAP, card, 0, np.flatnonzero(s)))
    if not out[n]:
        out.pop()
    return out


def describe(bm):
    """[(key, type, card, nruns, values)] of an oracle bitmap, the model's form."""
    vals = bm.to_array()
    res = []
    for key, ty, card, nr in bm.containers():
        lo, hi = np.searchsorted(vals, [key << 16, (key + 1) << 16])
        res.append((key, ty, card, nr if ty == RUN else 0, (vals[lo:hi] & 0xFFFF).astype(np.int64)))
    return res


def same_containers(x, y) -> bool:
    return len(x) == len(y) and all(p[:4] == q[:4] and np.array_equal(p[4], q[4]) for p, q in zip(x, y))
