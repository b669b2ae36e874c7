"""The BSI value read-back on the MI355X (rbgpu_bsi_values / rbgpu_bsi_values_device / rbgpu_bsi_get_values and the
getValue / valueExist / toPairList / transpose mirror) against two independent expectations (tests/bsi_values_ref.py):
the numpy model of the input columns and values, and the restatement of getValue / toPairList over the oracle bitmaps
deserialized from the uploaded set.  Every comparison is exact."""
import numpy as np
import pytest

from bsi_values_ref import model_pairs, model_values, ref_pairs, ref_values

pytestmark = pytest.mark.gpu

M64 = 2**64 - 1
# (rows, value bits, universe): 3-4 high keys up to 64 keys; the last holds values >= 2^63
SHAPES = [(3000, 10, 1 << 18), (50000, 40, 1 << 22), (500, 63, 1 << 17), (2000, 64, 1 << 18)]
KEY_RANGES = [(0, 2), (2, 3), (3, 65536)]


def _case(seed, n, nbits, universe):
    """Columns and values whose distribution differs per high key (key k's values lose 2 * (k % 4) low bits)."""
    rng = np.random.default_rng(seed)
    cols = np.unique(rng.integers(0, universe, size=n)).astype(np.uint64)
    hi = 2**nbits if nbits < 64 else 2**64
    vals = rng.integers(0, hi, size=len(cols), dtype=np.uint64, endpoint=False)
    if nbits == 64:
        vals[:4] |= np.uint64(1 << 63)
    vals = vals >> (np.uint64(2) * ((cols >> np.uint64(16)) % np.uint64(4)))
    return rng, cols, vals


def _upload(ctx, oracle, bitmaps, run_optimize):
    """bitmaps = the slices' rows then ebM's -> (device set, oracle slices, oracle ebM): the exact containers uploaded."""
    d = ctx.upload_values([np.asarray(b, np.uint32) for b in bitmaps], run_optimize=run_optimize)
    refs = [oracle.RefBitmap.deserialize(b) for b in d.serialize()]
    return d, refs[:-1], refs[-1]


def _device_bsi(ctx, oracle, cols, vals, run_optimize, nbits=None):
    sl, ebm, _, _ = oracle.bsi_build(cols, vals)
    bitmaps = [s.to_array() for s in sl]
    if nbits is not None:  # exactly nbits slices: empty ones above the largest value, or the index cut there
        bitmaps = (bitmaps + [np.zeros(0, np.uint32)] * nbits)[:nbits]
    return _upload(ctx, oracle, bitmaps + [ebm.to_array()], run_optimize)


def _found_sets(ctx, oracle, rng, cols, universe):
    """name -> (device set, oracle bitmap, rows)."""
    third = np.unique(rng.choice(cols, size=max(1, len(cols) // 3)))
    out = {
        "third+outside": np.unique(np.concatenate([third, rng.integers(0, universe, size=50).astype(np.uint64)])),
        "empty": np.zeros(0, np.uint64),
        "one key": cols[cols < 65536],
        # a key past the universe: no slice (and not ebM) has a container there
        "absent key": np.unique(np.concatenate([third[::2], universe + 65536 + np.arange(0, 500, 5, dtype=np.uint64)])),
    }
    sets = {}
    for name, rows in out.items():
        ref = oracle.RefBitmap.of(rows.astype(np.uint32))
        sets[name] = (ctx.upload_serialized([ref.serialize()]), ref, rows)
    rows = np.arange(1000, min(universe, 150000), dtype=np.uint64)  # a row range, Run-typed
    dev = ctx.upload_values([rows.astype(np.uint32)], run_optimize=True)
    ref = oracle.RefBitmap.deserialize(dev.serialize()[0])
    assert all(c[1] == 2 for c in ref.containers())
    sets["run"] = (dev, ref, rows)
    return sets


def _check_export(ctx, oracle, d, rsl, rebm, f_dev, f_ref, cols, vals, rows, tag, key_ranges=False):
    gc, gv = ctx.bsi_values(d, f_dev)
    st = ctx.stats()
    assert gc.dtype == np.uint32 and gv.dtype == np.uint64, tag
    assert np.all(gc[1:] > gc[:-1]), tag
    wc, wv = model_pairs(cols, vals, rows)
    assert np.array_equal(gc, wc) and np.array_equal(gv, wv), tag
    rc, rv = ref_pairs(oracle, rsl, rebm, f_ref)
    assert np.array_equal(gc, rc) and np.array_equal(gv, rv), tag
    if len(gc):
        F = rebm if f_ref is None else f_ref
        lo, hi = int(gc[0]) >> 16, int(gc[-1]) >> 16
        assert st["main_kernel"] == "k_bsi_values" and st["output_bytes"] == 12 * len(gc), (tag, st)
        assert st["result_cardinality"] == len(gc) and st["input_bytes"] > 0, (tag, st)
        assert st["tasks"] == len(F.containers()), (tag, st)
        assert lo >= F.containers()[0][0] and hi <= F.containers()[-1][0]
    # the aggregates over the same rows
    assert sum(int(v) for v in gv) & M64 == ctx.bsi_sum(d, f_dev)[0], tag
    if key_ranges:
        parts = [ctx.bsi_values(d, f_dev, key_range=kr) for kr in KEY_RANGES]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), gc), tag
        assert np.array_equal(np.concatenate([p[1] for p in parts]), gv), tag
        F = rebm if f_ref is None else f_ref
        ctx.bsi_values(d, f_dev, key_range=(2, 3))
        if any(c[0] == 2 for c in F.containers()):
            assert ctx.stats()["tasks"] == 1, tag


def _check_lookups(ctx, oracle, d, rsl, rebm, cols, vals, columns, tag):
    gv, ge = ctx.bsi_get_values(d, columns)
    assert gv.dtype == np.uint64 and ge.dtype == bool and len(gv) == len(ge) == len(columns), tag
    wv, we = model_values(cols, vals, columns)
    assert np.array_equal(gv, wv) and np.array_equal(ge, we), tag
    rv, re_ = ref_values(rsl, rebm, columns)
    assert np.array_equal(gv, rv) and np.array_equal(ge, re_), tag


def _query_columns(rng, cols, universe, n):
    """n columns, unsorted, with duplicates: present ones, absent ones of present keys, columns of a key without
    any container and columns past the universe."""
    pool = np.concatenate([rng.choice(cols, max(4, n)), rng.integers(0, universe, max(4, n)).astype(np.uint64),
                           universe + 65536 + rng.integers(0, 65536, 3).astype(np.uint64),
                           np.array([2**32 - 1, 2**32 - 65536], np.uint64), cols[:2], cols[:2]])
    return rng.permutation(pool)[:n].astype(np.uint32)


@pytest.mark.parametrize("run_optimize", [False, True])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_export_and_lookups(ctx, oracle, shape, run_optimize):
    n, nbits, uni = SHAPES[shape]
    rng, cols, vals = _case(60 + shape, n, nbits, uni)
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, run_optimize)
    assert len(rsl) == nbits
    _check_export(ctx, oracle, d, rsl, rebm, None, None, cols, vals, None, ("ebM", shape, run_optimize), True)
    sets = _found_sets(ctx, oracle, rng, cols, uni)
    for name, (f_dev, f_ref, rows) in sets.items():
        _check_export(ctx, oracle, d, rsl, rebm, f_dev, f_ref, cols, vals, rows, (name, shape, run_optimize),
                      name == "third+outside")
    if nbits == 64:
        assert int(ctx.bsi_values(d)[1].max()) >= 2**63
    for k in (0, 1, 5, 1000):
        q = _query_columns(rng, cols, uni, k)
        assert len(q) == k
        _check_lookups(ctx, oracle, d, rsl, rebm, cols, vals, q, ("lookup", shape, run_optimize, k))
    assert ctx.stats()["main_kernel"] == "k_bsi_get" and ctx.stats()["tasks"] == 1000
    if nbits == 64:
        v, e = ctx.bsi_get_values(d, cols[:4].astype(np.uint32))
        assert e.all() and np.array_equal(v, vals[:4]) and (v >> np.uint64(63)).any()
    # the rows topK keeps all exist, and their values are the largest
    f_dev, f_ref, rows = sets["one key"]
    if len(rows) > 4:
        top = ctx.bsi_topk(d, f_dev, len(rows) // 2)
        trows = oracle.RefBitmap.deserialize(top.serialize()[0]).to_array()
        tv, te = ctx.bsi_get_values(d, trows)
        assert te.all() and len(tv) <= len(rows) // 2
        rest = np.setdiff1d(rows.astype(np.uint32), trows)
        if len(tv):
            assert int(tv.min()) > int(ctx.bsi_get_values(d, rest)[0].max())


TILE_ROWS = np.array([0, 31, 32, 2047, 2048, 4095, 4096, 65535], np.uint64)


@pytest.mark.parametrize("run_optimize", [False, True])
def test_full_key_at_the_tile_edges(ctx, oracle, run_optimize):
    """All 65536 rows of high key 1 with neighbours in keys 0 and 2: bit 0 alternates (a Bitmap slice), bit 5 is set
    on every row (a full Run once optimized), bit 9 on eight rows at the tile edges (an Array), bit 40 on a run that
    crosses a tile boundary and on one that ends the key."""
    import roaringbitmap_amd as rb
    low = np.arange(65536, dtype=np.uint64)
    v1 = (low & np.uint64(1)) | np.uint64(1 << 5)
    v1[TILE_ROWS.astype(np.int64)] |= np.uint64(1 << 9)
    v1[2000:2101] |= np.uint64(1 << 40)
    v1[65500:65536] |= np.uint64(1 << 40)
    n0 = np.array([3, 65535], np.uint64)
    n2 = 2 * 65536 + np.array([0, 77, 65535], np.uint64)
    cols = np.concatenate([n0, 65536 + low, n2])
    vals = np.concatenate([np.array([7, 1 << 40], np.uint64), v1, np.array([1 << 9, 0, (1 << 41) - 1], np.uint64)])
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, run_optimize)
    at1 = {i: [c[1] for c in s.containers() if c[0] == 1] for i, s in enumerate(rsl)}
    assert at1[0] == [rb.BITMAP] and at1[9] == [rb.ARRAY] and at1[5] == [rb.RUN if run_optimize else rb.BITMAP]
    assert at1[40] == [rb.RUN if run_optimize else rb.ARRAY] and at1[20] == []
    _check_export(ctx, oracle, d, rsl, rebm, None, None, cols, vals, None, ("full key", run_optimize), True)
    # exactly one row per 2048-row tile of key 1, at a different place in each
    rows = 65536 + 2048 * np.arange(32, dtype=np.uint64) + (np.arange(32, dtype=np.uint64) * 67) % 2048
    rows[0], rows[31] = 65536, 65536 + 65535
    f_ref = oracle.RefBitmap.of(rows.astype(np.uint32))
    f_dev = ctx.upload_serialized([f_ref.serialize()])
    _check_export(ctx, oracle, d, rsl, rebm, f_dev, f_ref, cols, vals, rows, ("one row per tile", run_optimize))
    q = np.concatenate([65536 + TILE_ROWS, 65536 + np.array([1999, 2000, 2100, 2101, 65499, 65500], np.uint64), n0, n2,
                        np.array([4, 3 * 65536], np.uint64)]).astype(np.uint32)
    _check_lookups(ctx, oracle, d, rsl, rebm, cols, vals, q, ("full key", run_optimize))


def test_big_run_slice(ctx, oracle):
    """A slice container that is a Run of more than 2047 runs (its payload exceeds 8 KiB), uploaded as SoA so that
    it stays a Run: the export and the lookups read it straight from global memory."""
    import roaringbitmap_amd as rb
    from roaringbitmap_amd.engine import soa_from_values
    low = (4 * np.arange(3000, dtype=np.uint32)[:, None] + np.array([0, 1], np.uint32)).ravel()  # 3000 runs of 2
    rng = np.random.default_rng(3)
    s1 = np.unique(rng.integers(0, 3 * 65536, 30000)).astype(np.uint32)
    ebm = np.unique(np.concatenate([low + 65536, s1, np.arange(0, 3 * 65536, 7, dtype=np.uint32)]))
    h = soa_from_values([low + 65536, s1, ebm])
    assert h.key[0] == 1 and h.type[0] == rb.BITMAP and int(h.begin[1]) == 1
    runs = np.stack([low[::2], np.ones(3000, np.uint32)], axis=1).astype(np.uint16).tobytes()
    h.offset[0] = len(h.payload)
    h.type[0], h.nruns[0] = rb.RUN, 3000
    h.payload = np.concatenate([h.payload, np.frombuffer(runs + b"\0" * ((-len(runs)) % 16), np.uint8)])
    d = ctx.upload_soa(h)
    refs = [oracle.RefBitmap.deserialize(b) for b in d.serialize()]
    assert refs[0].containers() == [(1, rb.RUN, 6000, 3000)]
    rsl, rebm = refs[:2], refs[2]
    cols = ebm.astype(np.uint64)
    vals = np.isin(ebm, low + 65536).astype(np.uint64) | (np.isin(ebm, s1).astype(np.uint64) << np.uint64(1))
    _check_export(ctx, oracle, d, rsl, rebm, None, None, cols, vals, None, "big run")
    rows = np.arange(60000, 140000, 3, dtype=np.uint64)
    f_ref = oracle.RefBitmap.of(rows.astype(np.uint32))
    _check_export(ctx, oracle, d, rsl, rebm, ctx.upload_serialized([f_ref.serialize()]), f_ref, cols, vals, rows,
                  "big run, found")
    q = np.concatenate([65536 + np.arange(0, 12050, dtype=np.uint32), rng.integers(0, 3 * 65536, 500).astype(np.uint32)])
    _check_lookups(ctx, oracle, d, rsl, rebm, cols, vals, q, "big run")


def test_no_slices(ctx, oracle):
    """nbits == 0, a set holding ebM only: every value is 0 and exists follows ebM."""
    rows = np.unique(np.concatenate([np.arange(100, 70000, 3), np.array([3 * 65536 + 5])])).astype(np.uint32)
    d, rsl, rebm = _upload(ctx, oracle, [rows], False)
    assert rsl == []
    cols, vals = rows.astype(np.uint64), np.zeros(len(rows), np.uint64)
    _check_export(ctx, oracle, d, rsl, rebm, None, None, cols, vals, None, "nbits 0")
    f = np.arange(0, 4 * 65536, 5, dtype=np.uint64)
    f_ref = oracle.RefBitmap.of(f.astype(np.uint32))
    _check_export(ctx, oracle, d, rsl, rebm, ctx.upload_serialized([f_ref.serialize()]), f_ref, cols, vals, f,
                  "nbits 0, found")
    q = np.array([100, 101, 103, 5, 3 * 65536 + 5, 3 * 65536 + 6, 100, 9 * 65536], np.uint32)
    _check_lookups(ctx, oracle, d, rsl, rebm, cols, vals, q, "nbits 0")
    assert list(ctx.bsi_get_values(d, q)[1]) == [True, False, True, False, True, False, True, False]


@pytest.mark.parametrize("nbits", [32, 33])
@pytest.mark.parametrize("run_optimize", [False, True])
def test_high_dword_edge(ctx, oracle, nbits, run_optimize):
    """32 slices (the high half of the transpose is skipped) and 33 (it is not): bits 31 and 32 both appear."""
    rng = np.random.default_rng(nbits)
    cols = np.unique(rng.integers(0, 1 << 18, size=4000)).astype(np.uint64)
    vals = rng.integers(0, 2**nbits, size=len(cols), dtype=np.uint64)
    vals[:8] = np.array([2**nbits - 1, 1 << (nbits - 1), 1 << 31, (1 << 31) - 1, 0, 1, 1 << 30,
                         (1 << (nbits - 1)) | 1], np.uint64)
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, run_optimize, nbits)
    assert len(rsl) == nbits and len(d) == nbits + 1
    _check_export(ctx, oracle, d, rsl, rebm, None, None, cols, vals, None, ("edge", nbits), True)
    rows = cols[::3]
    f_ref = oracle.RefBitmap.of(rows.astype(np.uint32))
    _check_export(ctx, oracle, d, rsl, rebm, ctx.upload_serialized([f_ref.serialize()]), f_ref, cols, vals, rows,
                  ("edge, found", nbits))
    _check_lookups(ctx, oracle, d, rsl, rebm, cols, vals, _query_columns(rng, cols, 1 << 18, 300), ("edge", nbits))


def test_arguments_capacity_and_device_outputs(ctx, oracle):
    import torch

    import roaringbitmap_amd as rb
    rng, cols, vals = _case(71, 3000, 10, 1 << 18)
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, True)
    for kr in ((5, 70000), (3, 2)):
        with pytest.raises(rb.InvalidArgument):
            ctx.bsi_values(d, key_range=kr)
        with pytest.raises(rb.InvalidArgument):
            ctx.bsi_values_device(d, 0, 0, 0, key_range=kr)
    with pytest.raises(rb.InvalidArgument):
        ctx.bsi_values(d, found=d)  # found must be a one-bitmap set
    with pytest.raises(rb.InvalidArgument):
        ctx.bsi_values_device(d, 0, 0, 0, found=d)
    rows = cols[::2]
    f_ref = oracle.RefBitmap.of(rows.astype(np.uint32))
    f_dev = ctx.upload_serialized([f_ref.serialize()])
    for f, r in ((None, None), (f_dev, rows)):
        wc, wv = model_pairs(cols, vals, r)
        n = len(wc)
        assert ctx.bsi_values_device(d, 0, 0, 0, found=f) == n  # the count-only call
        for kr in KEY_RANGES:
            m = (wc >> 16 >= kr[0]) & (wc >> 16 < kr[1])
            assert ctx.bsi_values_device(d, 0, 0, 0, found=f, key_range=kr) == int(m.sum())
        tc = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda:0")
        tv = torch.full((n + 8,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(rb.InvalidArgument):  # one short: refused, outputs untouched
            ctx.bsi_values_device(d, tc.data_ptr(), tv.data_ptr(), n - 1, found=f)
        assert bool((tc == -7).all()) and bool((tv == -7).all())
        assert ctx.bsi_values_device(d, tc.data_ptr(), tv.data_ptr(), n, found=f) == n
        st = ctx.stats()
        assert st["main_kernel"] == "k_bsi_values" and st["output_bytes"] == 12 * n and st["n_kernels"] == 2
        gc, gv = tc.cpu().numpy().view(np.uint32), tv.cpu().numpy().view(np.uint64)
        assert np.array_equal(gc[:n], wc) and np.array_equal(gv[:n], wv)
        assert np.all(gc[n:] == np.uint32(2**32 - 7)) and np.all(gv[n:] == np.uint64(2**64 - 7))  # nothing past count
        hc, hv = ctx.bsi_values(d, f)
        assert np.array_equal(hc, gc[:n]) and np.array_equal(hv, gv[:n])
    # the C entry point itself: count > cap leaves the host arrays untouched and still reports the count
    import ctypes as C

    from roaringbitmap_amd import _lib as L
    n = len(cols)
    hc, hv, cnt = np.full(n, 9, np.uint32), np.full(n, 9, np.uint64), C.c_uint64()
    rc = L.lib().rbgpu_bsi_values(ctx.h, d.h, None, 0, 65536, hc.ctypes.data, hv.ctypes.data, n - 1, C.byref(cnt))
    assert rc == L.RB_EINVAL and cnt.value == n and np.all(hc == 9) and np.all(hv == 9)
    rc = L.lib().rbgpu_bsi_values(ctx.h, d.h, None, 0, 65536, hc.ctypes.data, None, n, C.byref(cnt))
    assert rc == L.RB_EINVAL  # cols without vals
    rc = L.lib().rbgpu_bsi_values(ctx.h, d.h, None, 0, 65536, hc.ctypes.data, hv.ctypes.data, n, C.byref(cnt))
    assert rc == L.RB_OK and cnt.value == n and np.array_equal(hc, cols.astype(np.uint32)) and np.array_equal(hv, vals)


def test_lookup_container_types(ctx, oracle):
    """ebM an Array at key 0, a Bitmap at key 1 and a Run at key 2; at key 2 the probed slices are a Bitmap, a Run
    and an Array."""
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(9)
    cols = np.concatenate([np.unique(rng.integers(0, 65536, 3000)), 65536 + np.unique(rng.integers(0, 65536, 30000)),
                           2 * 65536 + np.arange(65536)]).astype(np.uint64)
    low = cols & np.uint64(0xFFFF)
    vals = (rng.integers(0, 2, len(cols)).astype(np.uint64) | (((low >> np.uint64(8)) & np.uint64(1)) << np.uint64(1))
            | ((low % np.uint64(50) == 0).astype(np.uint64) << np.uint64(2)))
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, True, 3)
    assert [c[1] for c in rebm.containers()] == [rb.ARRAY, rb.BITMAP, rb.RUN]
    assert [[c[1] for c in s.containers() if c[0] == 2] for s in rsl] == [[rb.BITMAP], [rb.RUN], [rb.ARRAY]]
    q = np.concatenate([rng.permutation(cols)[:3000], rng.integers(0, 3 * 65536, 3000).astype(np.uint64),
                        2 * 65536 + np.array([0, 255, 256, 511, 512, 65535, 50, 100], np.uint64)]).astype(np.uint32)
    _check_lookups(ctx, oracle, d, rsl, rebm, cols, vals, q, "types")
    _check_export(ctx, oracle, d, rsl, rebm, None, None, cols, vals, None, "types")


def test_python_mirror_known_answers(ctx, oracle):
    """R64BSITest style: setValue(x, x) for x in 1..99."""
    import roaringbitmap_amd as rb
    from oracle import rbref64
    bsi = rb.Roaring64BitmapSliceIndex()
    assert bsi.getValue(5) == (0, False) and not bsi.valueExist(5) and len(bsi.toPairList()[0]) == 0
    assert bsi.transpose(None).isEmpty()
    for x in range(1, 100):
        bsi.setValue(x, x)
    assert bsi.getValue(50) == (50, True) and bsi.getValue(1000) == (0, False)
    assert bsi.valueExist(50) is True and bsi.valueExist(1000) is False
    v, e = bsi.getValues([99, 1, 1, 0, 100])
    assert list(v) == [99, 1, 1, 0, 0] and list(e) == [True, True, True, False, False]
    c, v = bsi.toPairList()
    assert c.dtype == np.uint32 and v.dtype == np.uint64
    assert list(c) == list(range(1, 100)) and list(v) == list(range(1, 100))
    c, v = bsi.toPairList(rb.RoaringBitmap.bitmapOf(list(range(1, 51)) + [500]))
    assert list(c) == list(range(1, 51)) and list(v) == list(range(1, 51))
    assert list(bsi.transpose(None).toArray()) == list(range(1, 100))
    assert list(bsi.transpose(rb.RoaringBitmap.bitmapOf([3, 4, 500])).toArray()) == [3, 4]
    assert bsi.transpose(rb.RoaringBitmap()).isEmpty()
    bsi.setValue(50, 7)  # a further setValue shows in every answer
    bsi.setValue(1000, 1 << 40)
    assert bsi.getValue(50) == (7, True) and bsi.getValue(1000) == (1 << 40, True)
    c, v = bsi.toPairList()
    assert len(c) == 100 and int(v[49]) == 7 and (int(c[-1]), int(v[-1])) == (1000, 1 << 40)
    assert 50 not in bsi.transpose(None).toArray()
    # repeated values, and more than 4096 distinct values in one bucket of the 64-bit result
    big = rb.Roaring64BitmapSliceIndex()
    rng = np.random.default_rng(4)
    values = np.concatenate([np.arange(0, 15000, 3), (1 << 35) + rng.integers(0, 1000, 3000)]).astype(np.uint64)
    values = np.concatenate([values, values[:2000]])
    for col, val in zip(rng.permutation(200000)[:len(values)], values):
        big.setValue(int(col), int(val))
    assert len(np.unique(values)) < len(values) and np.sum(np.unique(values) < 2**32) > 4096
    assert big.transpose(None).serializePortable() == rbref64.Ref64.of(values).to_portable()
    assert rb.RoaringBitmapSliceIndex is rb.Roaring64BitmapSliceIndex
