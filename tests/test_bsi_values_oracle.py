"""The BSI value read-back on the CPU: the restatement of getValue / toPairList over oracle bitmaps
(tests/bsi_values_ref.py) against the numpy model of the inputs and against the reference's known answers
(R64BSITest: setValue(x, x) for x in 1..99).  The MI355X kernels are held to both in tests/test_gpu_bsi_values.py."""
import numpy as np
import pytest

from bsi_values_ref import model_pairs, model_values, ref_pairs, ref_values

# (rows, value bits, universe): the shapes of tests/test_gpu_bsi_values.py
SHAPES = [(3000, 10, 1 << 18), (50000, 40, 1 << 22), (500, 63, 1 << 17), (2000, 64, 1 << 18)]


def _case(seed, n, nbits, universe):
    rng = np.random.default_rng(seed)
    cols = np.unique(rng.integers(0, universe, size=n)).astype(np.uint64)
    hi = 2**nbits if nbits < 64 else 2**64
    vals = rng.integers(0, hi, size=len(cols), dtype=np.uint64, endpoint=False)
    if nbits == 64:
        vals[:4] |= np.uint64(1 << 63)
    return rng, cols, vals


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_restatement_equals_model(oracle, shape):
    n, nbits, uni = SHAPES[shape]
    rng, cols, vals = _case(40 + shape, n, nbits, uni)
    slices, ebm, _, _ = oracle.bsi_build(cols, vals)
    gc, gv = ref_pairs(oracle, slices, ebm)
    wc, wv = model_pairs(cols, vals)
    assert np.array_equal(gc, wc) and np.array_equal(gv, wv)
    if nbits == 64:
        assert int(gv.max()) >= 2**63
    rows = np.unique(np.concatenate([rng.choice(cols, len(cols) // 3), rng.integers(0, uni, 50).astype(np.uint64)]))
    for r in (rows, np.zeros(0, np.uint64), cols[cols < 65536], uni + 65536 + np.arange(5, dtype=np.uint64)):
        gc, gv = ref_pairs(oracle, slices, ebm, oracle.RefBitmap.of(r.astype(np.uint32)))
        wc, wv = model_pairs(cols, vals, r)
        assert gc.dtype == np.uint32 and gv.dtype == np.uint64
        assert np.array_equal(gc, wc) and np.array_equal(gv, wv)
    q = np.concatenate([rng.choice(cols, 200), rng.integers(0, uni, 200).astype(np.uint64), [uni + 70000, 2**32 - 1]])
    gv, ge = ref_values(slices, ebm, q)
    wv, we = model_values(cols, vals, q)
    assert np.array_equal(gv, wv) and np.array_equal(ge, we)
    assert ge.any() and not ge.all()


def test_known_answers(oracle):
    x = np.arange(1, 100, dtype=np.uint64)
    slices, ebm, _, _ = oracle.bsi_build(x, x)
    v, e = ref_values(slices, ebm, [50, 1000, 99, 0])
    assert list(v) == [50, 0, 99, 0] and list(e) == [True, False, True, False]
    c, v = ref_pairs(oracle, slices, ebm)
    assert list(c) == list(range(1, 100)) and list(v) == list(range(1, 100))
    found = oracle.RefBitmap.of(np.array(list(range(1, 51)) + [500], np.uint32))
    c, v = ref_pairs(oracle, slices, ebm, found)
    assert list(c) == list(range(1, 51)) and list(v) == list(range(1, 51))
