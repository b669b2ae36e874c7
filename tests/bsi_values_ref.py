"""Expected answers of the BSI value read-back (a helper, not a test), from two independent sources.

model_pairs / model_values work on the input (cols, vals) in plain numpy.  ref_pairs / ref_values restate
Roaring64BitmapSliceIndex.getValue / valueAt (bsi/src/main/java/org/roaringbitmap/bsi/longlong/
Roaring64BitmapSliceIndex.java:127-136, 177-184) and BitSliceIndexBase.toPairList
(bsi/.../buffer/BitSliceIndexBase.java:534-549) over oracle bitmaps: membership of every row in every slice, read from
the bitmaps' own value arrays.  Values are unsigned 64-bit (valueAt's int accumulator agrees below 2^31)."""
import numpy as np

from bsi_agg_ref import found_values


def model_pairs(cols, vals, rows=None):
    """(cols uint32, vals uint64) of the rows of `rows` that the index holds (rows None: every column); cols sorted
    unique."""
    cols = np.asarray(cols, np.uint64)
    vals = np.asarray(vals, np.uint64)
    keep = cols if rows is None else np.intersect1d(cols, np.asarray(rows, np.uint64))
    return keep.astype(np.uint32), found_values(cols, vals, keep)


def model_values(cols, vals, columns):
    """(values uint64, exists bool) of arbitrary columns: 0 / False outside the index."""
    cols = np.asarray(cols, np.uint64)
    columns = np.asarray(columns, np.uint64)
    return found_values(cols, vals, columns), np.isin(columns, cols)


def _value_bits(slices, rows):
    """valueAt for every row: bit i = bA[i].contains(row)."""
    out = np.zeros(len(rows), np.uint64)
    for i, s in enumerate(slices):
        out[np.isin(rows, s.to_array())] |= np.uint64(1 << i)
    return out


def ref_values(slices, ebm, columns):
    """getValue(columnId) for every column: (0, False) outside ebM, else (valueAt, True)."""
    columns = np.asarray(columns, np.uint32)
    exists = np.isin(columns, ebm.to_array())
    vals = _value_bits(slices, columns)
    vals[~exists] = 0
    return vals, exists


def ref_pairs(R, slices, ebm, found=None):
    """toPairList() / toPairList(foundSet): getValue over ebM, or over and(ebM, foundSet)."""
    rows = (ebm if found is None else R.op(R.AND, ebm, found)).to_array().astype(np.uint32)
    return rows, _value_bits(slices, rows)
