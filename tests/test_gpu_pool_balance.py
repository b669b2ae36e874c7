"""The device pool's balance on the MI355X: after one call of every family and every argument error that follows
an allocation, with every set freed, the pool holds as many blocks handed out as right after rbgpu_open
(rbgpu_internal_pool_outstanding: +1 per alloc, -1 per release).  A block leaked on some return path leaves the
count high, one released twice leaves it low.  The error-path releases that only a HIP failure reaches are not
run here (no failure is provoked): they are verified by reading the code.
"""
import ctypes as C

import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L

pytestmark = pytest.mark.gpu


def _outstanding(ctx) -> int:
    fn = L.lib().rbgpu_internal_pool_outstanding
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
    return int(fn(ctx.h))


class _Sets:
    """Every set a call hands back, freed together at the end."""

    def __init__(self):
        self.held = []

    def __call__(self, s):
        self.held.append(s)
        return s

    def close(self):
        for s in self.held:
            s.close()
        self.held = []


def _pairwise_family(c, keep, s):
    a_idx, b_idx = np.array([0, 1, 2], np.uint32), np.array([1, 2, 0], np.uint32)
    for op in (rb.AND, rb.OR, rb.XOR, rb.ANDNOT):
        keep(c.pairwise(op, s, s, a_idx, b_idx))
    keep(c.pairwise(rb.AND, s, s))  # identity pairing: one segment per pair
    keep(c.pairwise_async(rb.OR, s, s, a_idx, b_idx)).wait()
    keep(c.pairwise_async(rb.XOR, s, s, a_idx, b_idx))  # left pending: freeing it settles it
    assert len(c.pairwise_cardinality(rb.AND, s, s, a_idx, b_idx)) == 3
    keep(c.pairwise_inplace(rb.XOR, s, s, a_idx, b_idx))
    with pytest.raises(rb.InvalidArgument):
        c.pairwise(rb.AND, s, s, np.array([0, 7], np.uint32), np.array([0, 1], np.uint32))


def test_pool_balance(monkeypatch):
    import torch
    if rb.Context.device_count() < 1:
        pytest.fail("no HIP device visible: gpu tests must run on the MI355X box")
    rng = np.random.default_rng(11)
    c = rb.Context(0)
    keep = _Sets()
    try:
        base = _outstanding(c)  # after the warm-up launches of rbgpu_open
        # ---- one Array, one Bitmap and one Run container (all at key 0: a dense set), and a set that is not dense
        vals = [np.array([1, 5, 9, 70], np.uint32), np.sort(rng.choice(65536, 5000, replace=False)).astype(np.uint32),
                np.arange(100, 3000, dtype=np.uint32)]
        s = keep(c.upload_values(vals, run_optimize=True))
        assert s.type_stats()["array"] == s.type_stats()["bitmap"] == s.type_stats()["run"] == 1
        sparse = keep(c.upload_values([vals[0], vals[1] + np.uint32(65536), vals[2] + np.uint32(3 * 65536)],
                                      run_optimize=True))
        assert _outstanding(c) == base + 14  # two sets of seven arrays each

        # ---- pairwise: the small-batch path, then the general pipeline
        _pairwise_family(c, keep, s)
        monkeypatch.setenv("RBGPU_NO_SMALL_PAIRS", "1")
        _pairwise_family(c, keep, s)
        _pairwise_family(c, keep, sparse)
        monkeypatch.delenv("RBGPU_NO_SMALL_PAIRS")

        # ---- wide: dense and grouped members, in set order and out of it
        for src in (s, sparse):
            for sem in (rb.FAST_OR, rb.WORKSHY_AND, rb.FAST_XOR, rb.HORIZONTAL_OR, rb.PQ_OR, rb.PQ_XOR,
                        rb.BUFFER_PQ_OR, rb.BUFFER_PQ_XOR):
                keep(c.wide(sem, src))
                keep(c.wide(sem, src, members=[2, 0, 1]))
            assert c.wide_cardinality(rb.OR, src) >= 5000
            keep(c.wide(rb.PQ_XOR, src, members=[1]))  # one member: a copy
            keep(c.wide(rb.PQ_OR, src, members=[]))    # none: the empty bitmap
        with pytest.raises(rb.InvalidArgument):  # BufferFastAggregation.priorityqueue_xor wants two bitmaps
            c.wide(rb.BUFFER_PQ_XOR, s, members=[0])
        with pytest.raises(rb.InvalidArgument):
            c.wide(rb.FAST_OR, s, members=[0, 7])

        # ---- serialize and deserialize, host and device forms
        blobs = s.serialize()
        sizes = s.serialized_sizes()
        total = int(sizes.sum())
        keep(c.upload_serialized(blobs))
        dbuf = torch.zeros(total + 8, dtype=torch.uint8, device="cuda:0")
        offs = s.serialize_device(dbuf.data_ptr(), total)
        torch.cuda.synchronize()
        assert bytes(dbuf.cpu().numpy()[:total]) == b"".join(blobs)
        keep(c.upload_serialized_device(dbuf.data_ptr(), offs))
        host = C.create_string_buffer(total)
        o4 = np.zeros(4, np.uint64)
        with pytest.raises(rb.InvalidArgument):  # cap one short, after the workspace was taken
            L.check(L.lib().rbgpu_set_serialize(s.h, 0, 3, host, total - 1, o4.ctypes.data_as(L._U64P)))
        with pytest.raises(rb.InvalidArgument):
            s.serialize_device(dbuf.data_ptr(), total - 1)
        with pytest.raises(rb.RbError):  # a truncated bitmap: the parse fails with its workspace taken
            c.upload_serialized([blobs[0][:5]])

        # ---- values, contains, rank, select
        arrays = s.to_arrays()
        assert all(np.array_equal(g, v) for g, v in zip(arrays, vals))
        nvals = sum(len(v) for v in vals)
        vbuf = torch.zeros(nvals, dtype=torch.int32, device="cuda:0")
        assert int(s.values_device(vbuf.data_ptr(), nvals)[-1]) == nvals
        hv = np.zeros(nvals, np.uint32)
        with pytest.raises(rb.InvalidArgument):  # cap one short: host, then device destination
            L.check(L.lib().rbgpu_set_values(s.h, 0, 3, hv.ctypes.data, nvals - 1, o4.ctypes.data_as(L._U64P)))
        with pytest.raises(rb.InvalidArgument):
            s.values_device(vbuf.data_ptr(), nvals - 1)
        q, qb = np.array([5, 6, 100, 2999], np.uint32), np.array([0, 1, 2, 2], np.uint32)
        assert list(s.contains(q, qb)) == [True, bool(np.isin(6, vals[1])), True, True]
        assert s.rank(q, qb)[2] == 1
        assert s.select(np.array([0, 10**6], np.uint64), np.array([2, 2], np.uint32))[1].tolist() == [True, False]
        with pytest.raises(rb.InvalidArgument):
            s.contains(q, np.array([0, 1, 2, 3], np.uint32))

        # ---- building from values, run-optimize, extract, gather, the metadata queries
        keep(c.build_values([v[::-1] for v in vals], run_optimize=True))  # descending: the sort path
        keep(c.build_values(vals))
        keep(c.build_values([]))
        keep(c.build_values_device(vbuf.data_ptr(), s._value_offsets(0, 3)))
        keep(s.run_optimize()[0])
        keep(c.extract(s, 1, 2))
        s64 = keep(c.upload_values64([vals[0].astype(np.uint64) + (np.uint64(7) << np.uint64(32)), vals[2]]))
        keep(s64.bucket_set(0))
        keep(c.pairwise64(rb.RB64_BITMAP, rb.XOR, s64, s64))
        assert s.range_counts(key_range=(0, 1)).tolist() == [1, 1, 1]
        assert sparse.range_counts(members=[2, 1], key_range=(1, 2)).tolist() == [0, 1]
        with pytest.raises(rb.InvalidArgument):
            s.range_counts(members=[3])
        assert s.cardinalities().tolist() == [len(v) for v in vals]
        assert [m["cardinality"] for m in s.summaries()] == [len(v) for v in vals]
        assert s.key_bytes()[0] > 0 and len(s.download().key) == 3
        for g in c.generate(L.WL_FILTER_POSTING, 4):
            keep(g)
        keep(c.generate_keys(L.WL_WIDE_MIXED, 3, 0, 64))
        keep(c.generate_bsi(3, 1000))

        # ---- BSI: built from pairs, compared with every op, aggregated, read back
        cols = rng.permutation(np.concatenate([np.arange(0, 300), np.arange(65536, 65536 + 40)])).astype(np.uint32)
        bvals = rng.integers(0, 1000, len(cols)).astype(np.uint64)
        bsi, mn, mx = c.bsi_build(cols, bvals, run_optimize=True)
        keep(bsi)
        tcols = torch.from_numpy(cols.astype(np.int32)).to("cuda:0")
        tvals = torch.from_numpy(bvals.astype(np.int64)).to("cuda:0")
        keep(c.bsi_build_device(tcols.data_ptr(), tvals.data_ptr(), len(cols))[0])
        found = keep(c.upload_values([np.sort(cols)[::3].copy()]))
        mid = int(np.median(bvals))
        for op in (rb.BSI_EQ, rb.BSI_NEQ, rb.BSI_LE, rb.BSI_LT, rb.BSI_GE, rb.BSI_GT):
            keep(c.bsi_compare(op, bsi, mid, 0, mn, mx))
            keep(c.bsi_compare(op, bsi, mid, 0, mn, mx, found=found, key_range=(1, 2)))
        for f in (None, found):
            keep(c.bsi_compare(rb.BSI_RANGE, bsi, mn + 1, mx - 1, mn, mx, found=f))
            keep(c.bsi_compare(rb.BSI_RANGE, bsi, mn + 1, mx - 1, mn, mx, found=f, key_range=(0, 1)))
            keep(c.bsi_compare(rb.BSI_LE, bsi, mx, 0, mn, mx, found=f))  # the min / max shortcut: all
            keep(c.bsi_compare(rb.BSI_LE, bsi, mx, 0, mn, mx, found=f, key_range=(1, 2)))
            keep(c.bsi_compare(rb.BSI_GT, bsi, mx, 0, mn, mx, found=f))  # ... and none
            assert c.bsi_sum(bsi, f)[1] == (len(cols) if f is None else len(np.sort(cols)[::3]))
            gc, gv = c.bsi_values(bsi, f)
            assert len(gc) == len(gv) == c.bsi_sum(bsi, f)[1]
        keep(c.bsi_topk(bsi, found, 3))
        keep(c.bsi_topk(bsi, found, 10**6))
        keep(c.bsi_topk(bsi, None, 3))
        n = len(cols)
        oc, ov = torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.zeros(n, dtype=torch.int64, device="cuda:0")
        assert c.bsi_values_device(bsi, oc.data_ptr(), ov.data_ptr(), n) == n
        hc, hv64, cnt = np.zeros(n, np.uint32), np.zeros(n, np.uint64), C.c_uint64()
        with pytest.raises(rb.InvalidArgument):  # cap one short: host, then device destination
            L.check(L.lib().rbgpu_bsi_values(c.h, bsi.h, None, 0, 65536, hc.ctypes.data, hv64.ctypes.data, n - 1,
                                             C.byref(cnt)))
        with pytest.raises(rb.InvalidArgument):
            c.bsi_values_device(bsi, oc.data_ptr(), ov.data_ptr(), n - 1)
        got, ex = c.bsi_get_values(bsi, [int(cols[0]), 400])
        assert ex.tolist() == [True, False] and int(got[0]) == int(bvals[0])
        torch.cuda.synchronize()

        # ---- every set freed, the derived tables with them: the pool is where it was
        assert _outstanding(c) > base
        keep.close()
        assert _outstanding(c) == base
    finally:
        keep.close()
        c.close()
