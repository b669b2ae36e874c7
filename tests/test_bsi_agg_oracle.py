"""The BSI aggregates on the CPU: the oracle restatements of Roaring64BitmapSliceIndex.sum / topK
(tests/bsi_agg_ref.py) against the reference's own known answers (R64BSITest.java testSum / testTopK) and against
independent value models, the container-type pin that separates Container.ior from the static or, and
ShardedBsi.sum's exchange over 2 gloo ranks.  The MI355X kernels are held to the same restatements in
tests/test_gpu_bsi_agg.py."""
import os

import numpy as np

from bsi_agg_ref import bitmap_pin_case, model_sum, model_topk, ref_sum, ref_topk
from test_sharding import _bsi_case, _restrict, _spawn

BITMAP = 1


def test_ref_sum_known_answer(oracle):
    """R64BSITest.testSum: values x -> x for 1..99, found 1..50."""
    x = np.arange(1, 100, dtype=np.uint64)
    slices, _, _, _ = oracle.bsi_build(x, x)
    found = oracle.RefBitmap.of(np.arange(1, 51, dtype=np.uint32))
    assert ref_sum(oracle, slices, found) == (1275, 50)
    assert ref_sum(oracle, slices, None) == (0, 0)
    assert ref_sum(oracle, slices, oracle.RefBitmap.of(np.zeros(0, np.uint32))) == (0, 0)


def test_ref_topk_known_answer(oracle):
    """R64BSITest.testTopK: {1: 3, 2: 6, 3: 4, 4: 10, 5: 7}, k = 2 -> {4, 5}."""
    cols = np.array([1, 2, 3, 4, 5], np.uint64)
    vals = np.array([3, 6, 4, 10, 7], np.uint64)
    slices, ebm, _, _ = oracle.bsi_build(cols, vals)
    assert list(ref_topk(oracle, slices, ebm, 2).to_array()) == [4, 5]
    assert ref_topk(oracle, slices, None, 2).cardinality() == 0
    assert ref_topk(oracle, slices, ebm, 0).cardinality() == 0
    assert ref_topk(oracle, slices, ebm, 5).serialize() == ebm.serialize()


def _tied_case(seed, nvalues):
    """~6 high keys, few distinct values (heavy ties), a distribution that differs per key, found = a part of
    the columns plus rows outside ebM."""
    rng = np.random.default_rng(seed)
    cols = np.unique(rng.integers(0, 6 * 65536, 20000)).astype(np.uint64)
    vals = rng.integers(0, nvalues, len(cols)).astype(np.uint64) >> ((cols >> np.uint64(16)) % np.uint64(3))
    rows = np.unique(np.concatenate([cols[rng.random(len(cols)) < 0.5], rng.integers(0, 7 * 65536, 300)]))
    return cols, vals, rows.astype(np.uint32)


def test_ref_topk_equals_value_model(oracle):
    for seed, nvalues in ((1, 8), (2, 50), (3, 1000)):
        cols, vals, rows = _tied_case(seed, nvalues)
        slices, _, _, _ = oracle.bsi_build(cols, vals)
        found = oracle.RefBitmap.of(rows)
        for k in (0, 1, 2, 7, 100, 3333, len(rows) // 2, len(rows) - 1, len(rows), len(rows) + 5):
            got = ref_topk(oracle, slices, found, k).to_array()
            assert np.array_equal(got, model_topk(cols, vals, rows, k)), (seed, k)


def test_ref_sum_equals_python_ints(oracle):
    rng = np.random.default_rng(7)
    cols, _, rows = _tied_case(4, 1000)
    for hi in (1 << 20, 1 << 63, 1 << 64):  # 64-bit values: the sum wraps
        vals = rng.integers(0, hi, len(cols), dtype=np.uint64)
        slices, _, _, _ = oracle.bsi_build(cols, vals)
        assert ref_sum(oracle, slices, oracle.RefBitmap.of(rows)) == model_sum(cols, vals, rows)


def test_ref_topk_bitmap_ior_pin(oracle):
    cols, vals, rows, k, key = bitmap_pin_case()
    slices, _, _, _ = oracle.bsi_build(cols, vals)
    got = ref_topk(oracle, slices, oracle.RefBitmap.of(rows), k)
    assert np.array_equal(got.to_array(), model_topk(cols, vals, rows, k))
    at_key = [c for c in got.containers() if c[0] == key]
    assert at_key == [(key, BITMAP, 65536, 0)], at_key  # not the full Run the static or returns
    assert [c[0] for c in got.containers()] == [key]


def _rank_bsi_sum(rank, world, port, q):
    import torch.distributed as dist

    from oracle import rbref as R
    from roaringbitmap_amd.sharding import ShardedBsi, partition_keys
    from roaringbitmap_amd.engine import soa_from_serialized
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        slices, ebm, _, _, found = _bsi_case(R)
        kb = np.zeros(65536, np.uint64)
        np.add.at(kb, soa_from_serialized([ebm.serialize()]).key.astype(np.int64), 1)
        lo, hi = partition_keys(kb, world)[rank]
        sb = ShardedBsi(dist, rank, world)
        for name, f in (("found", found), ("ebm", ebm)):
            s_f = _restrict(R, f, lo, hi)
            counts = [R.op_cardinality(R.AND, _restrict(R, s, lo, hi), s_f) for s in slices] + [s_f.cardinality()]
            got = sb.sum(None, None, (lo, hi), local_counts=np.array(counts, np.uint64))
            out[name] = (got, ref_sum(R, slices, f))
    except Exception as e:  # reported (every rank fails alike), so the parent does not wait for a rank that died
        out = {"error": (repr(e), None)}
    try:
        every = [None] * world
        dist.all_gather_object(every, out)
        if rank == 0:
            q.put(every)
    finally:
        dist.destroy_process_group()


def test_gloo_two_rank_sharded_bsi_sum():
    """Each rank computes its key range's slice counts with the oracle and passes them as local_counts; both get
    the whole index's ref_sum."""
    every = _spawn(_rank_bsi_sum)
    assert len(every) == 2
    for res in every:
        assert set(res) == {"found", "ebm"}, res
        for name, (got, want) in res.items():
            assert tuple(got) == tuple(want), (name, got, want)
