"""rbgpu_bsi_add / rbgpu_bsi_merge / rbgpu_bsi_min_max on the device against the reference restated over the CPU oracle
(tests/bsi_arith_ref.py): every result bitmap's serialized bytes and the bitmap count equal the restatement's, min and
max too, and — independently of the restatement — the result reads back (toPairList) as numpy's addition.  The
restatement's inputs are the device sets' own serialized bitmaps, so both sides start from the same containers."""
import numpy as np
import pytest

import bsi_arith_ref as ref
import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L
from test_bsi_arith_oracle import random_pairs, run_pairs

pytestmark = pytest.mark.gpu

U64 = np.uint64


def _bsi(ctx, cols, vals, run_optimize=False):
    cols, vals = np.asarray(cols, np.uint32), np.asarray(vals, U64)
    return ctx.bsi_build(cols, vals, run_optimize)[0], (cols, vals)


def _np_sum(pa, pb):
    cols = np.union1d(pa[0], pb[0]).astype(np.uint32)
    vals = np.zeros(len(cols), U64)
    for c, v in (pa, pb):
        vals[np.searchsorted(cols, c)] += v  # columns are distinct within one index
    return cols, vals


def _check_add(ctx, oracle, A, pa, B, pb, path=None, both=True):
    """a.add(b) on the device (the path the planner takes, and the forced chain) against the restatement and numpy."""
    want = ref.add(ref.from_blobs(A.serialize()), ref.from_blobs(B.serialize()))
    res = None
    for chain in ((False, True) if both else (False,)):
        got, lo, hi = ctx.bsi_add(A, B, chain=chain)
        main = ctx.stats()["main_kernel"]
        if chain:
            assert not main.startswith("k_bsi_add"), main
        elif path is not None:
            assert main.startswith("k_bsi_add") == (path == "fused"), main
        assert len(got) == len(want[0]) + 1
        assert got.serialize() == ref.blobs(want), "chain" if chain else "planned"
        assert (lo, hi) == ref.min_max(want)
        assert ctx.bsi_min_max(got) == (lo, hi)
        cols, vals = ctx.bsi_values(got)
        wc, wv = _np_sum(pa, pb)
        assert np.array_equal(cols, wc) and np.array_equal(vals, wv)
        res = res or got
    return res, want


def _types(bm):
    return [(k, t, c) for k, t, c, _ in bm.containers()]


def test_one_plus_one(ctx, oracle):
    A, pa = _bsi(ctx, [7], [1])
    got, want = _check_add(ctx, oracle, A, pa, A, pa, path="fused")
    assert len(got) == 3 and got.cardinalities().tolist() == [0, 1, 1]  # slice 0 keeps no container, slice 1 appears


@pytest.mark.parametrize("k", [1, 31, 32, 63])
def test_full_ripple_in_one_key(ctx, oracle, k):
    A, pa = _bsi(ctx, [3, 64, 65535], [(1 << k) - 1] * 3)
    B, pb = _bsi(ctx, [3, 64, 65535], [1, 1, 1])
    got, _ = _check_add(ctx, oracle, A, pa, B, pb, path="fused")
    assert len(A) == k + 1 and len(got) == k + 2  # the result grows by one slice
    assert got.cardinalities().tolist() == [0] * k + [3, 3]


@pytest.mark.parametrize("va,vb", [((1 << 64) - 1, 1), (1 << 63, 1 << 63)])
@pytest.mark.parametrize("chain", [False, True])
def test_a_65th_slice_is_refused(ctx, va, vb, chain):
    A, _ = _bsi(ctx, [1, 9], [va, 2])
    B, _ = _bsi(ctx, [1, 70000], [vb, 5])
    with pytest.raises(rb.InvalidArgument):
        ctx.bsi_add(A, B, chain=chain)  # the first call also builds the sets' cached key tables
    import ctypes as C
    fn = L.lib().rbgpu_internal_pool_outstanding
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
    held, out = int(fn(ctx.h)), C.c_void_p()
    rc = L.lib().rbgpu_bsi_add(ctx.h, A.h, B.h, L.BSI_ADD_CHAIN if chain else 0, C.byref(out), None, None)
    assert rc == L.RB_EINVAL and not out.value and int(fn(ctx.h)) == held  # nothing created, nothing kept
    one, _ = _bsi(ctx, [9], [1])
    assert ctx.bsi_add(A, one, chain=chain)[1:] == (3, va)  # and the context still works


def test_carries_at_lane_and_word_edges(ctx, oracle):
    low = np.array([0, 63, 64, 1023, 1024, 65535], np.uint32)
    cols = np.concatenate([low, (65535 << 16) + low]).astype(np.uint32)
    A, pa = _bsi(ctx, cols, np.full(len(cols), 0b0111, U64))
    B, pb = _bsi(ctx, cols, np.tile(np.array([1, 2, 3, 4, 5, 9], U64), 2))
    _check_add(ctx, oracle, A, pa, B, pb, path="fused")


def test_type_boundary_of_a_touched_slice(ctx, oracle):
    A, pa = _bsi(ctx, np.arange(4097), np.ones(4097, U64))
    for col, val, want0 in ((0, 1, (ref.ARRAY, 4096)), (5000, 1, (ref.BITMAP, 4098)), (0, 2, (ref.BITMAP, 4097))):
        B, pb = _bsi(ctx, [col], [val])
        got, want = _check_add(ctx, oracle, A, pa, B, pb, path="fused")
        assert _types(want[0][0]) == [(0,) + want0]
        assert _types(ref.from_blobs(got.serialize())[0][0]) == [(0,) + want0]


def test_key_classes_in_one_call(ctx, oracle):
    rng = np.random.default_rng(5)
    # key 1 only a, key 9 only b, key 4 shared; at key 4 a holds slices 0..2 and b slices 3..5 only on some columns,
    # and a run of columns holds 1 + 1 everywhere, so slice 0 ends with no container there
    ca = np.concatenate([(1 << 16) + np.arange(0, 3000, 3), (4 << 16) + np.arange(0, 2000)]).astype(np.uint32)
    va = np.concatenate([rng.integers(0, 64, 1000), rng.integers(0, 8, 2000)]).astype(U64)
    cb = np.concatenate([(4 << 16) + np.arange(1000, 2500), (9 << 16) + np.arange(50, 5000)]).astype(np.uint32)
    vb = np.concatenate([rng.integers(0, 8, 1500) << 3, rng.integers(0, 300, 4950)]).astype(U64)
    A, pa = _bsi(ctx, ca, va)
    B, pb = _bsi(ctx, cb, vb)
    _check_add(ctx, oracle, A, pa, B, pb, path="fused")
    ones = (np.arange(100, 900, dtype=np.uint32) + (2 << 16), np.ones(800, U64))
    hi = (np.array([5, (2 << 16) + 950], np.uint32), np.array([4, 4], U64))
    A, pa = _bsi(ctx, np.concatenate([hi[0][:1], ones[0], hi[0][1:]]), np.concatenate([hi[1][:1], ones[1], hi[1][1:]]))
    B, pb = _bsi(ctx, ones[0], ones[1])
    got, _ = _check_add(ctx, oracle, A, pa, B, pb, path="fused")
    assert got.cardinalities().tolist() == [0, 800, 2, 802]  # slice 0 has no container left in the middle of the index


def test_bit_counts_and_empties(ctx, oracle):
    rng = np.random.default_rng(6)
    small = random_pairs(rng, (0, 3), 700, 3)
    big = random_pairs(rng, (3, 4), 900, 21)
    S, ps = _bsi(ctx, *small)
    G, pg = _bsi(ctx, *big)
    _check_add(ctx, oracle, S, ps, G, pg, path="fused")  # na < nb
    _check_add(ctx, oracle, G, pg, S, ps, path="fused")  # na > nb
    # na = 0: only an ebM of zero-valued columns
    zc = np.arange(10, 5000, 7, dtype=np.uint32)
    Z = ctx.upload_values([zc])
    pz = (zc, np.zeros(len(zc), U64))
    assert len(Z) == 1
    _check_add(ctx, oracle, Z, pz, S, ps, path="fused")
    _check_add(ctx, oracle, S, ps, Z, pz, path="fused")
    # b's ebM empty: a clone of a, its bitmap count kept; a empty: b's containers
    E, pe = _bsi(ctx, [], [])
    got, lo, hi = ctx.bsi_add(G, E)
    assert got.serialize() == G.serialize() and (lo, hi) == (int(big[1].min()), int(big[1].max()))
    got, _ = _check_add(ctx, oracle, E, pe, G, pg, path="fused")
    assert got.serialize() == G.serialize()


def _with_runs(rng, run_key, value, shared_key=3):
    c1, v1 = random_pairs(rng, (shared_key,), 3000, 9)
    c2, v2 = run_pairs(run_key, 100, 40000, value)
    o = np.argsort(np.concatenate([c1, c2]), kind="stable")
    return np.concatenate([c1, c2])[o], np.concatenate([v1, v2])[o]


def test_runs_at_unshared_keys_are_copied_by_the_fused_kernel(ctx, oracle):
    rng = np.random.default_rng(8)
    A, pa = _bsi(ctx, *_with_runs(rng, 1, 0b101101), run_optimize=True)
    B, pb = _bsi(ctx, *_with_runs(rng, 9, 0b110), run_optimize=True)
    assert A.type_stats()["run"] > 0 and B.type_stats()["run"] > 0
    got, want = _check_add(ctx, oracle, A, pa, B, pb, path="fused")
    assert any(t == ref.RUN for s in want[0] for _, t, _ in _types(s))


def test_runs_at_a_shared_key_take_the_chain(ctx, oracle):
    rng = np.random.default_rng(9)
    A, pa = _bsi(ctx, *_with_runs(rng, 3, 0b101101, shared_key=5), run_optimize=True)  # a Run at key 3 ...
    B, pb = _bsi(ctx, *random_pairs(rng, (3, 5), 2500, 7))                             # ... where b holds slices too
    _check_add(ctx, oracle, A, pa, B, pb, path="chain", both=False)
    # Run against Run at one key
    B2, pb2 = _bsi(ctx, *run_pairs(3, 20000, 30000, 0b111), run_optimize=True)
    _check_add(ctx, oracle, A, pa, B2, pb2, path="chain", both=False)


@pytest.mark.parametrize("bits", [1, 13, 40])
@pytest.mark.parametrize("members", [300, 5000, 40000])
def test_random_fused_equals_restatement_and_chain(ctx, oracle, members, bits):
    rng = np.random.default_rng(members * 100 + bits)
    A, pa = _bsi(ctx, *random_pairs(rng, (0, 7, 65535), members, bits))
    B, pb = _bsi(ctx, *random_pairs(rng, (0, 7, 65535), members, bits))
    _check_add(ctx, oracle, A, pa, B, pb, path="fused")


def test_fused_stats_contract(ctx):
    rng = np.random.default_rng(11)
    A, _ = _bsi(ctx, *random_pairs(rng, (2, 3), 5000, 6))
    B, _ = _bsi(ctx, *random_pairs(rng, (3, 4), 5000, 6))
    got, _, _ = ctx.bsi_add(A, B)
    st = ctx.stats()
    assert [k["name"] for k in st["kernels"]] == ["k_bsi_add<measure>", "k_bsi_add<emit>"]
    assert st["tasks"] == 3  # the keys walked
    nslice = int(got.n_containers) - 3  # ebM holds three containers
    # payload + 16 B per container (a summary's Run payload counts the serialized form's 2-byte run count)
    per = lambda s, nb: sum(x["payload_bytes"] - 2 * x["n_run_containers"] + 16 * x["n_containers"]
                            for x in s.summaries()[:nb])
    assert st["result_containers"] == nslice
    assert st["output_bytes"] == per(got, len(got) - 1)
    assert st["input_bytes"] == per(A, len(A) - 1) + per(B, len(B) - 1)


def test_calls_that_name_no_kernel(ctx):
    """rb_stats of the clone for an empty b, and of a fused call without any slice container, is the call's own (no
    kernel span, nothing counted), not the previous call's."""
    A, _ = _bsi(ctx, [1, 2], [3, 4])
    E, _ = _bsi(ctx, [], [])
    Z1 = ctx.upload_values([np.array([1, 2], np.uint32)])       # ebM only: every value 0
    Z2 = ctx.upload_values([np.array([2, 70000], np.uint32)])
    for call in (lambda: ctx.bsi_add(A, E)[0], lambda: ctx.bsi_merge(A, E), lambda: ctx.bsi_add(Z1, Z2)[0]):
        ctx.bsi_add(A, A)
        assert ctx.stats()["main_kernel"].startswith("k_bsi_add")
        got = call()
        st = ctx.stats()
        assert st["main_kernel"] == "" and st["kernels"] == [] and st["input_bytes"] == st["output_bytes"] == 0
    assert len(got) == 1 and got.cardinalities().tolist() == [3] and ctx.bsi_min_max(got) == (0, 0)
    got = ctx.bsi_add(A, E)[0]
    assert ctx.stats()["result_containers"] == got.n_containers and got.serialize() == A.serialize()


# ---- merge ------------------------------------------------------------------------------------------------------
def _disjoint(rng, bits_a, bits_b):
    ca, va = random_pairs(rng, (0, 2), 3000, bits_a)
    cb, vb = random_pairs(rng, (2, 5), 2000, bits_b)
    keep = ~np.isin(cb, ca)
    ra, va_r = run_pairs(8, 10, 30000, (1 << bits_a) - 1)  # long equal-valued ranges: Runs once run-optimised
    rb_, vb_r = run_pairs(8, 40000, 20000, 1)
    return (np.concatenate([ca, ra]), np.concatenate([va, va_r])), (np.concatenate([cb[keep], rb_]),
                                                                    np.concatenate([vb[keep], vb_r]))


@pytest.mark.parametrize("run_optimize", [False, True])
@pytest.mark.parametrize("bits", [(9, 9), (5, 14), (14, 5)])
def test_merge(ctx, oracle, bits, run_optimize):
    pa, pb = _disjoint(np.random.default_rng(12), *bits)
    A, _ = _bsi(ctx, *pa, run_optimize=run_optimize)
    B, _ = _bsi(ctx, *pb, run_optimize=run_optimize)
    want = ref.merge(ref.from_blobs(A.serialize()), ref.from_blobs(B.serialize()), run_optimize)
    got = ctx.bsi_merge(A, B, run_optimize=run_optimize)
    assert len(got) == max(bits) + 1 and got.serialize() == ref.blobs(want)
    if run_optimize:  # slices run-optimised, ebM not: the in-place or of two Runs at key 8 is no Run-optimised form
        assert any(t == ref.RUN for s in want[0] for _, t, _ in _types(s))
    cols, vals = ctx.bsi_values(got)
    wc, wv = _np_sum(pa, pb)
    assert np.array_equal(cols, wc) and np.array_equal(vals, wv)
    assert ctx.bsi_min_max(got) == (int(wv.min()), int(wv.max()))


def test_merge_refusals_and_empty(ctx, oracle):
    pa, pb = _disjoint(np.random.default_rng(13), 6, 6)
    A, _ = _bsi(ctx, *pa)
    B, _ = _bsi(ctx, *pb)
    for X, col in ((A, pa[0][:1]), (B, pb[0][-1:])):  # intersecting ebMs, on either side
        Y, _ = _bsi(ctx, col, [3])
        with pytest.raises(rb.InvalidArgument):
            ctx.bsi_merge(X, Y)
        with pytest.raises(rb.InvalidArgument):
            ctx.bsi_merge(Y, X)
    E, _ = _bsi(ctx, [], [])
    assert ctx.bsi_merge(A, E).serialize() == A.serialize()  # empty b: a clone of a
    got = ctx.bsi_merge(E, A)
    want = ref.merge(ref.from_blobs(E.serialize()), ref.from_blobs(A.serialize()))
    assert got.serialize() == ref.blobs(want) == A.serialize()


# ---- minValue / maxValue ----------------------------------------------------------------------------------------
def test_min_max(ctx, oracle):
    rng = np.random.default_rng(14)
    cols, vals = random_pairs(rng, (0, 7, 65535), 20000, 40)
    vals[::97] = 0
    S, lo, hi = ctx.bsi_build(cols, vals + U64(5))
    assert ctx.bsi_min_max(S) == (lo, hi) == (5, int(vals.max()) + 5)
    assert ctx.stats()["main_kernel"] == "k_bsi_minmax" and ctx.stats()["tasks"] == 3
    T, _, _ = ctx.bsi_build([3, 1 << 20, (1 << 32) - 1], [1 << 63, (1 << 64) - 1, (1 << 63) + 1])
    assert ctx.bsi_min_max(T) == (1 << 63, (1 << 64) - 1)
    G = ctx.generate_bsi(12, 300000, seed=3)
    _, gv = ctx.bsi_values(G)
    assert ctx.bsi_min_max(G) == (int(gv.min()), int(gv.max())) == ref.min_max(ref.from_blobs(G.serialize()))
    assert ctx.bsi_min_max(ctx.bsi_build([], [])[0]) == (0, 0)
    assert ctx.bsi_min_max(ctx.upload_values([np.arange(5, dtype=np.uint32)])) == (0, 0)  # no slices: every value 0


# ---- arguments --------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_on_the_host(ctx):
    import ctypes as C
    A, _ = _bsi(ctx, [1, 2], [3, 4])
    lib, out, lo, hi = L.lib(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    wide = ctx.build_values([np.arange(3, dtype=np.uint32)] * 66)  # more than 64 slices and ebM
    none = ctx.build_values([])                                     # no bitmap at all
    assert len(wide) == 66 and len(none) == 0
    other = rb.Context(0)
    try:
        foreign = other.bsi_build([1], [1])[0]
        for bad in (None, wide.h, none.h, foreign.h):
            for a, b in ((bad, A.h), (A.h, bad)):
                assert lib.rbgpu_bsi_add(ctx.h, a, b, 0, C.byref(out), C.byref(lo), C.byref(hi)) == L.RB_EINVAL
                assert lib.rbgpu_bsi_merge(ctx.h, a, b, 0, C.byref(out)) == L.RB_EINVAL
                assert not out.value
            assert lib.rbgpu_bsi_min_max(ctx.h, bad, C.byref(lo), C.byref(hi)) == L.RB_EINVAL
        foreign.close()
    finally:
        other.close()
    assert lib.rbgpu_bsi_add(ctx.h, A.h, A.h, 2, C.byref(out), None, None) == L.RB_EINVAL
    assert lib.rbgpu_bsi_merge(ctx.h, A.h, A.h, 2, C.byref(out)) == L.RB_EINVAL
    assert lib.rbgpu_bsi_add(ctx.h, A.h, A.h, 0, None, None, None) == L.RB_EINVAL
    assert lib.rbgpu_bsi_min_max(ctx.h, A.h, None, C.byref(hi)) == L.RB_EINVAL
    # min / max may be left out
    assert lib.rbgpu_bsi_add(ctx.h, A.h, A.h, 0, C.byref(out), None, None) == L.RB_OK
    rb.DeviceSet(ctx, out.value).close()


# ---- the Python class -------------------------------------------------------------------------------------------
def test_class_add_and_merge(oracle):
    rng = np.random.default_rng(15)
    pa = random_pairs(rng, (0, 1), 4000, 11)
    pb = random_pairs(rng, (1, 2), 4000, 11)
    x = rb.Roaring64BitmapSliceIndex.from_pairs(*pa)
    x.add(rb.Roaring64BitmapSliceIndex.from_pairs(*pb))
    wc, wv = _np_sum(pa, pb)
    y = rb.Roaring64BitmapSliceIndex.from_pairs(wc, wv)
    assert (x.minValue, x.maxValue, x.bitCount()) == (y.minValue, y.maxValue, y.bitCount())
    for v in (0, int(np.median(wv)), int(wv.max()), int(wv.max()) + 1):
        assert x.compare(rb.BSI_GE, v).serialize() == y.compare(rb.BSI_GE, v).serialize()
    every = x.getExistenceBitmap()
    assert x.sum(every) == y.sum(every) == (int(wv.sum()), len(wc))
    x.add(None)
    x.add(rb.Roaring64BitmapSliceIndex())
    assert x.sum(every) == y.sum(every)

    keep = ~np.isin(pb[0], pa[0])
    pb = (pb[0][keep], pb[1][keep] + U64(5000))
    m = rb.Roaring64BitmapSliceIndex.from_pairs(*pa)
    other = rb.Roaring64BitmapSliceIndex.from_pairs(*pb)
    m.merge(other)
    wc, wv = _np_sum(pa, pb)
    vals, ex = m.getValues(wc)
    assert ex.all() and np.array_equal(vals, wv)
    assert (m.minValue, m.maxValue, m.bitCount()) == (int(wv.min()), int(wv.max()), int(wv.max()).bit_length())
    with pytest.raises(ValueError):
        m.merge(other)
    d = rb.Roaring64BitmapSliceIndex.from_device(m._device())  # min and max left out: computed on the device
    assert (d.minValue, d.maxValue) == (m.minValue, m.maxValue)
