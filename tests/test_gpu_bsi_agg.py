"""The BSI aggregates on the MI355X (rbgpu_bsi_slice_counts / rbgpu_bsi_sum / rbgpu_bsi_sum_sharded /
rbgpu_bsi_topk) against the oracle restatements of Roaring64BitmapSliceIndex.sum / topK (tests/bsi_agg_ref.py):
exact numbers for sum, identical serialized bytes (container types included) for topK."""
import numpy as np
import pytest

from bsi_agg_ref import bitmap_pin_case, found_values, model_sum, model_topk, ref_sum, ref_topk

pytestmark = pytest.mark.gpu

# (rows, value bits, universe): multi-key, the shapes of test_gpu_bsi.py, and 64-bit values (>= 2^63: the sum wraps)
SHAPES = [(3000, 10, 1 << 18), (50000, 40, 1 << 22), (500, 63, 1 << 17), (2000, 64, 1 << 18)]


def _case(seed, n, nbits, universe):
    """Columns and values whose distribution differs per high key (key k's values lose 2 * (k % 4) low bits), so
    a decision taken per key would differ from the global one."""
    rng = np.random.default_rng(seed)
    cols = np.unique(rng.integers(0, universe, size=n)).astype(np.uint64)
    hi = 2**nbits if nbits < 64 else 2**64
    vals = rng.integers(0, hi, size=len(cols), dtype=np.uint64, endpoint=False)
    if nbits == 64:
        vals[:4] |= np.uint64(1 << 63)
    vals = vals >> (np.uint64(2) * ((cols >> np.uint64(16)) % np.uint64(4)))
    return rng, cols, vals


def _device_bsi(ctx, oracle, cols, vals, run_optimize):
    sl, ebm, _, _ = oracle.bsi_build(cols, vals)
    d = ctx.upload_values([s.to_array() for s in sl] + [ebm.to_array()], run_optimize=run_optimize)
    refs = [oracle.RefBitmap.deserialize(b) for b in d.serialize()]  # the exact containers uploaded
    return d, refs[:-1], refs[-1]


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


def _check_counts(ctx, oracle, d, rsl, rebm, f_dev, f_ref, cols, vals, rows, tag):
    import roaringbitmap_amd as rb
    nbits = len(rsl)
    F = rebm if f_ref is None else f_ref
    want = [oracle.op_cardinality(oracle.AND, s, F) for s in rsl] + [F.cardinality()]
    got = ctx.bsi_slice_counts(d, f_dev)
    assert got.dtype == np.uint64 and [int(x) for x in got] == want, tag
    st = ctx.stats()
    if F.cardinality():
        assert st["main_kernel"] == "k_bsi_sum" and st["main_kernel_ms"] > 0.0 and st["input_bytes"] > 0, (tag, st)
        assert st["tasks"] == len(F.containers()), tag
    # the sum, against the restated Java method and the Python-int model
    s = ctx.bsi_sum(d, f_dev)
    frows = cols if f_ref is None else rows
    assert s == (ref_sum(oracle, rsl, F) if F.cardinality() else (0, 0)), tag
    assert s == model_sum(cols, vals, frows), tag
    # the composed path a caller had before: one batched AND-cardinality call over (slice_i, found)
    if nbits:
        if f_dev is None:
            comp = ctx.pairwise_cardinality(rb.AND, d, d, list(range(nbits)), [nbits] * nbits)
        else:
            comp = ctx.pairwise_cardinality(rb.AND, d, f_dev, list(range(nbits)), [0] * nbits)
        assert [int(x) for x in comp] == want[:nbits], tag
    # key ranges add up element-wise to the whole
    parts = [ctx.bsi_slice_counts(d, f_dev, key_range=kr) for kr in [(0, 2), (2, 3), (3, 65536)]]
    assert [int(x) for x in sum(parts)] == want, tag


@pytest.mark.parametrize("run_optimize", [False, True])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_slice_counts_and_sum(ctx, oracle, shape, run_optimize):
    n, nbits, uni = SHAPES[shape]
    rng, cols, vals = _case(10 + shape, n, nbits, uni)
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, run_optimize)
    assert len(rsl) == nbits
    _check_counts(ctx, oracle, d, rsl, rebm, None, None, cols, vals, None, ("ebM", shape, run_optimize))
    for name, (f_dev, f_ref, rows) in _found_sets(ctx, oracle, rng, cols, uni).items():
        _check_counts(ctx, oracle, d, rsl, rebm, f_dev, f_ref, cols, vals, rows, (name, shape, run_optimize))
    if nbits == 64:
        assert ctx.bsi_sum(d)[0] != sum(int(v) for v in vals)  # the 64-bit case wraps


def test_slice_counts_big_run_container(ctx, oracle):
    """A slice container that is a Run of more than 2047 runs (its payload exceeds 8 KiB: the from-global toggle
    branch), uploaded as SoA so that it stays a Run."""
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
    found_ref = oracle.RefBitmap.of(np.arange(60000, 140000, 3, dtype=np.uint32))
    found = ctx.upload_serialized([found_ref.serialize()])
    for f_dev, F in ((None, refs[2]), (found, found_ref)):
        want = [oracle.op_cardinality(oracle.AND, s, F) for s in refs[:2]] + [F.cardinality()]
        assert [int(x) for x in ctx.bsi_slice_counts(d, f_dev)] == want
    # topK walks the same container in both of its phases
    for k in (1, 1500, 2000, 20000):
        assert ctx.bsi_topk(d, found, k).serialize()[0] == ref_topk(oracle, refs[:2], found_ref, k).serialize(), k


def test_sum_arguments_and_known_answer(ctx, oracle):
    import roaringbitmap_amd as rb
    d = ctx.generate_bsi(12, 3 * 65536 + 99, seed=5)
    with pytest.raises(rb.InvalidArgument):
        ctx.bsi_slice_counts(d, key_range=(5, 70000))
    with pytest.raises(rb.InvalidArgument):
        ctx.bsi_slice_counts(d, key_range=(3, 2))
    with pytest.raises(rb.InvalidArgument):
        ctx.bsi_slice_counts(d, found=d)  # found must be a one-bitmap set
    with pytest.raises(rb.InvalidArgument):
        ctx.bsi_topk(d, d, 3)
    # R64BSITest.testSum through the Python mirror
    bsi = rb.Roaring64BitmapSliceIndex(1, 99)
    for x in range(1, 100):
        bsi.setValue(x, x)
    assert bsi.sum(rb.RoaringBitmap.bitmapOf(list(range(1, 51)))) == (1275, 50)
    assert bsi.sum(None) == (0, 0) and bsi.sum(rb.RoaringBitmap()) == (0, 0)


def test_sum_sharded_world_one(ctx, oracle):
    from roaringbitmap_amd.engine import Comm
    comm = Comm(ctx, Comm.unique_id(), 1, 0)
    try:
        d = ctx.generate_bsi(16, 3 * 65536 + 99, seed=5)
        found = ctx.upload_values([np.arange(0, 3 * 65536, 3, dtype=np.uint32)])
        for f in (None, found):
            assert ctx.bsi_sum_sharded(comm, d, (0, 65536), f) == ctx.bsi_sum(d, f)
            c = ctx.bsi_slice_counts(d, f, key_range=(1, 3))
            want = (sum(int(c[i]) << i for i in range(16)) & (2**64 - 1), int(c[16]))
            assert comm.bsi_sum_sharded(d, (1, 3), f) == want
    finally:
        comm.close()


def _ks_from_data(cols, vals, rows):
    """k values chosen from the data: 0, 1, 2, a k where the k-th and (k+1)-th largest values differ, a k inside a
    tie, |found| - 1, |found| and |found| + 5."""
    v = np.sort(found_values(cols, vals, rows))[::-1]
    n = len(v)
    ks = {0, 1, 2, n - 1, n, n + 5}
    diff = [k for k in range(3, n - 1) if v[k - 1] != v[k]]
    tie = [k for k in range(3, n - 1) if v[k - 1] == v[k]]
    if diff:
        ks.add(diff[len(diff) // 2])
    if tie:
        ks.add(tie[len(tie) // 2])
    return sorted(k for k in ks if k >= 0), (diff[len(diff) // 2] if diff else None), (tie[len(tie) // 2] if tie else None)


def _check_topk(ctx, oracle, d, rsl, f_dev, f_ref, cols, vals, rows, tag):
    ks, k_diff, k_tie = _ks_from_data(cols, vals, rows)
    found_bytes = f_ref.serialize()
    for k in ks:
        got = ctx.bsi_topk(d, f_dev, k)
        want = ref_topk(oracle, rsl, f_ref, k)
        assert got.serialize()[0] == want.serialize(), (tag, k)
        card = int(got.cardinalities()[0])
        assert card == len(model_topk(cols, vals, rows, k)), (tag, k)
        if k >= len(rows):
            assert got.serialize()[0] == found_bytes, (tag, k)
        if k == k_diff:
            assert card == k, (tag, k)
        if k == k_tie:
            assert card < k, (tag, k)


@pytest.mark.parametrize("run_optimize", [False, True])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_topk_bytes(ctx, oracle, shape, run_optimize):
    n, nbits, uni = SHAPES[shape]
    rng, cols, vals = _case(20 + shape, n, nbits, uni)
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, run_optimize)
    sets = _found_sets(ctx, oracle, rng, cols, uni)
    for name in ("third+outside", "absent key", "run"):
        f_dev, f_ref, rows = sets[name]
        _check_topk(ctx, oracle, d, rsl, f_dev, f_ref, cols, vals, rows, (name, shape, run_optimize))
    f_dev, f_ref, _ = sets["empty"]
    assert ctx.bsi_topk(d, f_dev, 3).serialize()[0] == f_ref.serialize()
    assert ctx.bsi_topk(d, None, 3).serialize()[0] == f_ref.serialize()
    st_dev, st_ref, st_rows = sets["third+outside"]
    ctx.bsi_topk(d, st_dev, max(1, len(st_rows) // 2))
    st = ctx.stats()
    assert st["n_kernels"] == 2 and st["main_kernel_ms"] > 0.0


@pytest.mark.parametrize("run_optimize", [False, True])
def test_topk_massive_ties(ctx, oracle, run_optimize):
    """A 3-bit index over 3000 rows of 4 keys: 8 distinct values."""
    rng, cols, vals = _case(31, 3000, 3, 1 << 18)
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, run_optimize)
    rows = np.unique(np.concatenate([cols[::2], rng.integers(0, 1 << 18, 40).astype(np.uint64)]))
    f_ref = oracle.RefBitmap.of(rows.astype(np.uint32))
    f_dev = ctx.upload_serialized([f_ref.serialize()])
    _check_topk(ctx, oracle, d, rsl, f_dev, f_ref, cols, vals, rows, ("ties", run_optimize))
    for k in range(3, len(rows), 211):
        assert ctx.bsi_topk(d, f_dev, k).serialize()[0] == ref_topk(oracle, rsl, f_ref, k).serialize(), k


def test_topk_run_found_on_run_index(ctx, oracle):
    """A run-optimized index of long runs with a Run-typed found: the Run AND Run -> toEfficientContainer rules."""
    cols = np.arange(0, 5 * 65536, dtype=np.uint64)
    vals = (cols >> np.uint64(9)) % np.uint64(37) >> ((cols >> np.uint64(16)) % np.uint64(3))  # runs of 512 rows
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, True)
    assert any(c[1] == 2 for s in rsl for c in s.containers())
    rows = np.arange(3000, 4 * 65536 + 777, dtype=np.uint64)
    f_dev = ctx.upload_values([rows.astype(np.uint32)], run_optimize=True)
    f_ref = oracle.RefBitmap.deserialize(f_dev.serialize()[0])
    assert all(c[1] == 2 for c in f_ref.containers())
    _check_topk(ctx, oracle, d, rsl, f_dev, f_ref, cols, vals, rows, "runs")
    assert ctx.bsi_sum(d, f_dev) == ref_sum(oracle, rsl, f_ref) == model_sum(cols, vals, rows)


def test_topk_bitmap_ior_pin(ctx, oracle):
    import roaringbitmap_amd as rb
    cols, vals, rows, k, key = bitmap_pin_case()
    d, rsl, rebm = _device_bsi(ctx, oracle, cols, vals, False)
    f_ref = oracle.RefBitmap.of(rows)
    got = ctx.bsi_topk(d, ctx.upload_serialized([f_ref.serialize()]), k)
    assert got.serialize()[0] == ref_topk(oracle, rsl, f_ref, k).serialize()
    h = got.download()
    assert (list(h.key), list(h.type), list(h.card)) == ([key], [rb.BITMAP], [65536])


def test_topk_python_mirror(ctx, oracle):
    """R64BSITest.testTopK through Roaring64BitmapSliceIndex.topK."""
    import roaringbitmap_amd as rb
    bsi = rb.Roaring64BitmapSliceIndex()
    for c, v in ((1, 3), (2, 6), (3, 4), (4, 10), (5, 7)):
        bsi.setValue(c, v)
    found = bsi.getExistenceBitmap()
    assert list(bsi.topK(found, 2).toArray()) == [4, 5]
    assert bsi.topK(None, 3).isEmpty() and bsi.topK(rb.RoaringBitmap(), 3).isEmpty()
    assert bsi.topK(found, 5) is found and bsi.topK(found, 9) is found
