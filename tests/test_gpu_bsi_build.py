"""A bit-sliced index built from (column, value) pairs on the MI355X: rbgpu_bsi_from_pairs / rbgpu_bsi_from_pairs_device,
Context.bsi_build / bsi_build_device and Roaring64BitmapSliceIndex.from_pairs.  The serialized bytes of every bitmap of
the result (the slices, then ebM), the bitmap count, min and max equal oracle.rbref.bsi_build(cols, vals), each oracle
bitmap run-optimized when the flag is set.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L

pytestmark = pytest.mark.gpu

A, B, R = rb.ARRAY, rb.BITMAP, rb.RUN


def _rng(seed):
    return np.random.default_rng(seed)


def _one_pair():
    return np.array([70000], np.uint32), np.array([5], np.uint64)


def _only_zero():
    return np.array([3, 9, 65536 + 4], np.uint32), np.zeros(3, np.uint64)


def _bit63():
    return np.array([1, 2, 200000], np.uint32), np.array([1 << 63, 7, (1 << 63) | 12345], np.uint64)


def _three_keys():
    """Keys 0, 7 and 65535; 5000 columns in key 7, so its ebM container is a Bitmap while every slice holds about half
    of them, an Array."""
    rng = _rng(5)
    cols = np.concatenate([rng.choice(65536, 300, replace=False), (7 << 16) + rng.choice(65536, 5000, replace=False),
                           (65535 << 16) + rng.choice(65536, 40, replace=False), [0, 2**32 - 1]])
    cols = np.unique(cols).astype(np.uint32)
    return cols, rng.integers(0, 1 << 20, len(cols)).astype(np.uint64)


def _full_key():
    cols = np.arange(1 << 16, 2 << 16, dtype=np.uint32)
    return cols, cols.astype(np.uint64)


def _unsorted_repeats():
    """Unsorted columns, each given up to four times with different values: the last value of a column stands."""
    rng = _rng(6)
    base = rng.choice(1 << 19, 6000, replace=False).astype(np.uint32)
    cols = rng.permutation(np.concatenate([base, base[:4000], base[1000:3000], base[:500]])).astype(np.uint32)
    return cols, rng.integers(0, 1 << 33, len(cols)).astype(np.uint64)


CASES = {"one-pair": _one_pair, "only-zero": _only_zero, "bit-63": _bit63, "three-keys": _three_keys,
         "full-key": _full_key, "unsorted-repeats": _unsorted_repeats}


def check(ctx, oracle, cols, vals, ro, built=None):
    if built is None:
        built = ctx.bsi_build(cols, vals, run_optimize=ro)
    d, lo, hi = built
    sl, ebm, vmin, vmax = oracle.bsi_build(cols, vals)
    refs = sl + [ebm]
    if ro:
        for r in refs:
            r.run_optimize()
    assert (lo, hi) == (vmin, vmax)
    assert len(d) == len(refs) == max(1, int(vmax).bit_length()) + 1
    got = d.serialize()
    for i, r in enumerate(refs):
        assert got[i] == r.serialize(), (i, ro)
    h = d.download()
    conts = [c for r in refs for c in r.containers()]
    assert list(zip(h.key.tolist(), h.type.tolist(), h.card.tolist(), h.nruns.tolist())) == conts
    sizes = [8192 if t == B else 2 * c if t == A else 4 * r for _, t, c, r in conts]
    assert d.payload_capacity == sum((b + 15) & ~15 for b in sizes)
    return d, h, refs


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("ro", [False, True])
def test_bsi_build(ctx, oracle, name, ro):
    cols, vals = CASES[name]()
    d, h, refs = check(ctx, oracle, cols, vals, ro)
    s = ctx.stats()
    assert s["main_kernel"] == "k_set_build" and s["tasks"] == d.n_containers == s["result_containers"]
    assert s["input_bytes"] == 12 * len(cols) and s["result_cardinality"] == sum(r.cardinality() for r in refs)
    if name == "only-zero":  # slice 0 is an empty bitmap
        assert len(d) == 2 and h.begin.tolist() == [0, 0, 2]
    if name == "bit-63":
        assert len(d) == 65
    if name == "three-keys":
        ebm = h.begin[-2]
        assert h.key[ebm:].tolist() == [0, 7, 65535] and h.type[ebm:].tolist() == [A, B, A]
        assert set(h.type[:ebm].tolist()) == {A}
    if name == "full-key":
        # slice i holds runs of 2^i columns: 2^(15 - i) of them, a Run once that is at most 2047; slice 16 and ebM are
        # the whole key
        assert h.type.tolist() == ([B] * 5 + [R] * 13 if ro else [B] * 18)
    if name == "unsorted-repeats":
        assert len(np.unique(cols)) < len(cols) and refs[-1].cardinality() == len(np.unique(cols))


def test_empty_index(ctx):
    d, lo, hi = ctx.bsi_build([], [])
    assert (len(d), d.n_containers, lo, hi) == (1, 0, 0, 0)


def test_device_form(ctx, oracle):
    import torch
    cols, vals = _unsorted_repeats()
    tc = torch.from_numpy(cols.view(np.int32).copy()).to("cuda:0")
    tv = torch.from_numpy(vals.view(np.int64).copy()).to("cuda:0")
    bc, bv = tc.clone(), tv.clone()
    torch.cuda.synchronize()
    for ro in (False, True):
        check(ctx, oracle, cols, vals, ro, built=ctx.bsi_build_device(tc.data_ptr(), tv.data_ptr(), len(cols), ro))
    assert torch.equal(tc, bc) and torch.equal(tv, bv)
    # columns that already ascend strictly are read where they lie
    cols, vals = _three_keys()
    tc = torch.from_numpy(cols.view(np.int32).copy()).to("cuda:0")
    tv = torch.from_numpy(vals.view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    check(ctx, oracle, cols, vals, True, built=ctx.bsi_build_device(tc.data_ptr(), tv.data_ptr(), len(cols), True))


def test_bad_arguments(ctx):
    cols, vals = _one_pair()
    fn = L.lib().rbgpu_bsi_from_pairs
    out = C.c_void_p()
    assert fn(ctx.h, None, vals.ctypes.data, 1, 0, C.byref(out), None, None) == L.RB_EINVAL
    assert fn(ctx.h, cols.ctypes.data, None, 1, 0, C.byref(out), None, None) == L.RB_EINVAL
    assert fn(ctx.h, cols.ctypes.data, vals.ctypes.data, 1, 0, None, None, None) == L.RB_EINVAL
    assert fn(ctx.h, cols.ctypes.data, vals.ctypes.data, 1, 4, C.byref(out), None, None) == L.RB_EINVAL
    assert not out.value
    assert fn(ctx.h, cols.ctypes.data, vals.ctypes.data, 1, 1, C.byref(out), None, None) == L.RB_OK  # min / max optional
    assert len(rb.DeviceSet(ctx, out.value)) == 4


@pytest.mark.parametrize("name", ["three-keys", "unsorted-repeats"])
def test_from_pairs_answers_like_the_host_built_index(ctx, name):
    """compare (EQ, RANGE), sum and toPairList of from_pairs(...) against the index built pair by pair on the host."""
    cols, vals = CASES[name]()
    dev = rb.Roaring64BitmapSliceIndex.from_pairs(cols, vals)
    host = rb.Roaring64BitmapSliceIndex()
    host.setValues(zip(cols.tolist(), vals.tolist()))
    assert dev.bitCount() == host.bitCount()
    hc, hv = host.toPairList()
    dc, dv = dev.toPairList()
    assert np.array_equal(hc, dc) and np.array_equal(hv, dv)
    some = int(hv[len(hv) // 2])
    lo, hi = int(np.percentile(hv, 25)), int(np.percentile(hv, 75))
    for op, a, b in ((rb.BSI_EQ, some, 0), (rb.BSI_EQ, int(hv.max()) + 1, 0), (rb.BSI_RANGE, lo, hi),
                     (rb.BSI_RANGE, 0, 2**63)):
        assert np.array_equal(dev.compare(op, a, b).toArray(), host.compare(op, a, b).toArray()), (op, a, b)
    found = rb.RoaringBitmap.bitmapOf(hc[::3])
    assert dev.sum(found) == host.sum(found)
    assert dev.sum(dev.getExistenceBitmap()) == (int(hv.astype(object).sum()) % 2**64, len(hv))
