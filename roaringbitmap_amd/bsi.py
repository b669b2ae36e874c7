"""Host-side mirror of the reference's bit-sliced index (bsi module) for the compare hot path.

  Roaring64BitmapSliceIndex / RoaringBitmapSliceIndex   bsi/src/main/java/org/roaringbitmap/bsi/
    setValue(columnId, value)        longlong/Roaring64BitmapSliceIndex.java:291-326
    compare(op, startOrValue, end, foundSet)              :460-503 (O'Neil, oNeilCompare :410-446)
    getExistenceBitmap / bitCount / runOptimize          :141-168
    sum / topK                                            :559-594
    getValue / valueExist / transpose                     :177-184, 284-286, 596-601
    add / merge / minValue / maxValue                     :64-93, 357-383, 95-125
    toPairList                                            buffer/BitSliceIndexBase.java:534-549

The slices and the existence bitmap live in HBM as one DeviceSet (slices bA[0..n), then ebM) and a
query runs as one fused MI355X pass per high key (librbgpu rbgpu_bsi_compare).  Values are
unsigned 64-bit; the reference stores Java longs and cannot hold bit 63 (setValue tests
`(value & (1L << i)) > 0`), so the two agree on every value below 2^63.
"""
from __future__ import annotations

from typing import Iterable, Optional, Tuple

import numpy as np

from . import _lib as L
from .engine import DeviceSet, default_context
from .roaring import Roaring64Bitmap, RoaringBitmap

Operation = type("Operation", (), {"EQ": L.BSI_EQ, "NEQ": L.BSI_NEQ, "LE": L.BSI_LE, "LT": L.BSI_LT,
                                   "GE": L.BSI_GE, "GT": L.BSI_GT, "RANGE": L.BSI_RANGE})


class Roaring64BitmapSliceIndex:
    def __init__(self, min_value: int = 0, max_value: int = 0):
        if min_value < 0:
            raise ValueError("Values should be non-negative")
        self._cols = {}                 # columnId -> value (host staging until the next query)
        self.minValue, self.maxValue = 0, 0
        self._nbits = max(0, int(max_value).bit_length())
        self._dev: Optional[DeviceSet] = None
        self._run_optimized = False

    # ---- construction (setValue semantics, Roaring64BitmapSliceIndex.java:291-326)
    def setValue(self, column_id: int, value: int) -> None:
        if not self._cols:
            self.minValue = self.maxValue = value
            self._nbits = max(self._nbits, max(1, int(value).bit_length()))
        elif self.minValue > value:
            self.minValue = value
        elif self.maxValue < value:
            self.maxValue = value
            self._nbits = max(self._nbits, int(value).bit_length())
        self._cols[int(column_id)] = int(value)
        self._dev = None

    def setValues(self, pairs: Iterable[Tuple[int, int]]) -> None:
        for c, v in pairs:
            self.setValue(c, v)

    @classmethod
    def from_device(cls, dset: DeviceSet, min_value: Optional[int] = None,
                    max_value: Optional[int] = None) -> "Roaring64BitmapSliceIndex":
        """Wrap a device-resident BSI (slices then ebM), e.g. rbgpu_generate_bsi's.  min_value / max_value left
        out: computed on the device (rbgpu_bsi_min_max) — compare short-circuits on them, so they must be true."""
        if min_value is None or max_value is None:
            lo, hi = dset.ctx.bsi_min_max(dset)
            min_value = lo if min_value is None else min_value
            max_value = hi if max_value is None else max_value
        b = cls()
        b._dev, b.minValue, b.maxValue, b._nbits = dset, min_value, max_value, len(dset) - 1
        b._cols = None
        return b

    @classmethod
    def from_pairs(cls, cols, vals, run_optimize: bool = False) -> "Roaring64BitmapSliceIndex":
        """setValues(pairs) on a fresh index (Roaring64BitmapSliceIndex.java:291-348), then runOptimize when asked,
        built on the device from the two arrays (rbgpu_bsi_from_pairs): any order, the last value of a column
        kept, values unsigned 64-bit."""
        dset, lo, hi = default_context().bsi_build(cols, vals, run_optimize)
        return cls.from_device(dset, lo, hi)

    def runOptimize(self) -> None:
        self._run_optimized = True
        self._dev = None

    # ---- arithmetic (Roaring64BitmapSliceIndex.java:64-93, 357-383): both leave the index device-resident, as
    # after from_device
    def _adopt(self, dset: DeviceSet, min_value: int, max_value: int) -> None:
        self._dev, self._cols, self._nbits = dset, None, len(dset) - 1
        self.minValue, self.maxValue = min_value, max_value

    def add(self, other: Optional["Roaring64BitmapSliceIndex"]) -> None:
        """add(otherBsi): value[c] += other[c] over the union of the columns, on the device (rbgpu_bsi_add);
        minValue / maxValue are recomputed, as the reference does.  None or an empty other index changes nothing."""
        if other is None or other._no_rows():
            return
        d, o = self._device(), other._device()
        self._adopt(*d.ctx.bsi_add(d, o))

    def merge(self, other: Optional["Roaring64BitmapSliceIndex"]) -> None:
        """merge(otherBsi): the union with an index over disjoint columns (rbgpu_bsi_merge); the slices are
        run-optimised when either index was, minValue / maxValue are the min / max of the two fields, like the
        reference.  Common columns raise ValueError (InvalidArgument)."""
        if other is None or other._no_rows():
            return
        d, o = self._device(), other._device()
        if int(o.cardinalities()[-1]) == 0:
            return
        ro = self._run_optimized or other._run_optimized
        res = d.ctx.bsi_merge(d, o, run_optimize=ro)
        self._adopt(res, min(self.minValue, other.minValue), max(self.maxValue, other.maxValue))
        self._run_optimized = ro

    def bitCount(self) -> int:
        return self._nbits

    def _device(self) -> DeviceSet:
        if self._dev is None:
            cols = np.fromiter(self._cols.keys(), dtype=np.uint64, count=len(self._cols))
            vals = np.fromiter(self._cols.values(), dtype=np.uint64, count=len(self._cols))
            order = np.argsort(cols)
            cols, vals = cols[order], vals[order]
            bitmaps = [cols[((vals >> np.uint64(i)) & np.uint64(1)) == 1].astype(np.uint32)
                       for i in range(self._nbits)] + [cols.astype(np.uint32)]
            self._dev = default_context().upload_values(bitmaps, run_optimize=self._run_optimized)
        return self._dev

    def getExistenceBitmap(self) -> RoaringBitmap:
        d = self._device()
        return RoaringBitmap(default_context().extract(d, len(d) - 1))

    def getLongCardinality(self) -> int:
        return int(self._device().cardinalities()[-1])

    # ---- the query hot path
    def compare(self, operation: int, start_or_value: int, end: int = 0,
                found_set: Optional[RoaringBitmap] = None) -> RoaringBitmap:
        d = self._device()
        found = found_set._set if found_set is not None else None
        return RoaringBitmap(d.ctx.bsi_compare(operation, d, start_or_value, end, self.minValue, self.maxValue,
                                               found))

    # ---- the aggregates (Roaring64BitmapSliceIndex.java:559-594)
    def sum(self, found_set: Optional[RoaringBitmap]) -> Tuple[int, int]:
        """sum(foundSet) -> (sum, count): the values of foundSet's rows added up (mod 2^64, the bits of Java's
        wrapped long) and foundSet's cardinality; None or an empty set gives (0, 0).  One fused pass per high key
        (rbgpu_bsi_sum).  The 32-bit class weights slice x by (long)(1 << x), an int shift: it agrees for
        bitCount <= 31, and Context.bsi_slice_counts serves a caller who needs that arithmetic."""
        if found_set is None or found_set.isEmpty():
            return 0, 0
        d = self._device()
        return d.ctx.bsi_sum(d, found_set._set)

    def topK(self, found_set: Optional[RoaringBitmap], k: int) -> RoaringBitmap:
        """topK(foundSet, k): the rows of foundSet holding the k largest values, by the reference's descent over the
        slices (a tie at the k-th value may leave fewer than k rows); None or an empty set gives an empty bitmap,
        k >= cardinality returns found_set itself (rbgpu_bsi_topk).  BitSliceIndexBase.topK (buffer/, with its
        exact-k tie trimming) is not covered; the rows' values come from getValues / toPairList."""
        if found_set is None or found_set.isEmpty():
            return RoaringBitmap()
        if k >= found_set.getCardinality():
            return found_set
        d = self._device()
        return RoaringBitmap(d.ctx.bsi_topk(d, found_set._set, k))

    # ---- value read-back (Roaring64BitmapSliceIndex.java:127-136, 177-184, 284-286, 596-601;
    # buffer/BitSliceIndexBase.java:534-549)
    def _no_rows(self) -> bool:
        return self._cols is not None and not self._cols

    def getValues(self, column_ids) -> Tuple[np.ndarray, np.ndarray]:
        """getValue for a batch of column ids (any order, duplicates allowed) -> (values uint64, exists bool): one
        wave per column probes the 64 slices at once (rbgpu_bsi_get_values).  A column outside the existence
        bitmap has value 0.  Values are the true unsigned values; the reference's valueAt accumulates `1 << i` in
        an int and agrees for bitCount <= 31."""
        c = np.asarray(column_ids, dtype=np.uint32).ravel()
        if self._no_rows():
            return np.zeros(len(c), np.uint64), np.zeros(len(c), bool)
        d = self._device()
        return d.ctx.bsi_get_values(d, c)

    def getValue(self, column_id: int) -> Tuple[int, bool]:
        """getValue(columnId) -> (value, exists): (0, False) for a column outside the existence bitmap."""
        v, e = self.getValues([column_id])
        return int(v[0]), bool(e[0])

    def valueExist(self, column_id: int) -> bool:
        return self.getValue(column_id)[1]

    def toPairList(self, found_set: Optional[RoaringBitmap] = None) -> Tuple[np.ndarray, np.ndarray]:
        """toPairList() / toPairList(foundSet): the (columnId, value) pairs of the rows of the existence bitmap (AND
        foundSet), ascending columnId — as two arrays (cols uint32, vals uint64), not a list of Pair objects: one
        transposing pass per high key on the device (rbgpu_bsi_values)."""
        if self._no_rows():
            return np.zeros(0, np.uint32), np.zeros(0, np.uint64)
        d = self._device()
        return d.ctx.bsi_values(d, found_set._set if found_set is not None else None)

    def transpose(self, found_set: Optional[RoaringBitmap] = None) -> Roaring64Bitmap:
        """transpose(foundSet): the distinct values of the rows of the existence bitmap (AND foundSet) as a
        Roaring64Bitmap, the reference's re.add(getValue(x)) loop; an empty index or found set gives an empty
        bitmap."""
        _, vals = self.toPairList(found_set)
        return Roaring64Bitmap.bitmapOf(np.unique(vals))


RoaringBitmapSliceIndex = Roaring64BitmapSliceIndex  # the 32-bit index runs the same compare
