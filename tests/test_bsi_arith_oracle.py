"""The restated BSI arithmetic (tests/bsi_arith_ref.py) checked on the CPU, before any device code is trusted against
it: the restated add is integer addition, the one-pass rule the fused kernel implements gives the restated chain's
containers (types, cardinalities, values) wherever no Run container is touched, and merge reads back as the union."""
import numpy as np
import pytest

import bsi_arith_ref as ref

KEYS = (0, 7, 65535)


def random_pairs(rng, keys, members, bits):
    """`members` distinct columns in each high key of `keys`, values below 2^bits: (cols uint32 ascending, vals uint64)."""
    cols = np.concatenate([(k << 16) + np.sort(rng.choice(65536, size=members, replace=False)) for k in sorted(keys)])
    vals = rng.integers(0, 1 << bits, size=len(cols), dtype=np.uint64, endpoint=False)
    return cols.astype(np.uint32), vals


def run_pairs(key, start, length, value):
    """One value over a column range of one high key: a Run container in every set slice once run-optimised."""
    cols = (key << 16) + np.arange(start, start + length, dtype=np.uint32)
    return cols.astype(np.uint32), np.full(length, value, np.uint64)


def summed(pa, pb):
    d = {}
    for cols, vals in (pa, pb):
        for c, v in zip(cols.tolist(), [int(x) for x in vals]):
            d[c] = d.get(c, 0) + v
    cols = sorted(d)
    return cols, [d[c] for c in cols]


@pytest.fixture(scope="module")
def built(oracle):
    return oracle


@pytest.mark.parametrize("seed", range(6))
def test_restated_add_is_integer_addition(built, seed):
    rng = np.random.default_rng(100 + seed)
    pa = random_pairs(rng, KEYS[:2], int(rng.integers(1, 3000)), int(rng.integers(1, 20)))
    pb = random_pairs(rng, KEYS[1:], int(rng.integers(1, 3000)), int(rng.integers(1, 20)))
    r = ref.add(ref.build(*pa), ref.build(*pb))
    cols, vals = ref.pairs(r)
    wc, wv = summed(pa, pb)
    assert cols.tolist() == wc and vals == wv
    assert ref.min_max(r) == (min(wv), max(wv))
    assert len(r[0]) == max(1, max(wv).bit_length(), int(pa[1].max()).bit_length(), int(pb[1].max()).bit_length())


def test_restated_add_edges(built):
    one = ref.build([5], [1])
    r = ref.add(one, one)
    assert [s.cardinality() for s in r[0]] == [0, 1]  # slice 0 stays in the count with no container left
    assert ref.pairs(ref.add(one, ([], ref.empty())))[1] == [1]
    top = ref.build([1, 2], [(1 << 64) - 1, 3])
    with pytest.raises(OverflowError):
        ref.add(top, ref.build([1], [1]))
    assert ref.min_max(([], ref.empty())) == (0, 0)
    assert ref.min_max(ref.build([1, 9, 70000], [1 << 63, 5, (1 << 63) + 1])) == (5, (1 << 63) + 1)


def _model_matches(a, b):
    got = ref.add_model(a, b)
    want = ref.add(a, b)[0]
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert ref.same_containers(g, ref.describe(w)), j


@pytest.mark.parametrize("seed", range(30))
def test_rule_model_equals_the_chain_without_runs(built, seed):
    rng = np.random.default_rng(seed)
    dens = rng.choice([0.01, 0.05, 0.2, 0.5], size=2)
    ka = [k for k in KEYS if rng.random() < 0.8] or [KEYS[0]]
    kb = [k for k in KEYS if rng.random() < 0.8] or [KEYS[2]]
    a = ref.build(*random_pairs(rng, ka, int(65536 * dens[0]), int(rng.integers(1, 20))))
    b = ref.build(*random_pairs(rng, kb, int(65536 * dens[1]), int(rng.integers(1, 20))))
    _model_matches(a, b)


@pytest.mark.parametrize("seed", range(12))
def test_rule_model_equals_the_chain_with_runs_at_unshared_keys(built, seed):
    rng = np.random.default_rng(1000 + seed)

    def side(run_key, value):
        c1, v1 = random_pairs(rng, (3,), int(rng.integers(100, 30000)), int(rng.integers(1, 16)))
        c2, v2 = run_pairs(run_key, int(rng.integers(0, 1000)), int(rng.integers(5000, 60000)), value)
        o = np.argsort(np.concatenate([c1, c2]), kind="stable")
        return np.concatenate([c1, c2])[o], np.concatenate([v1, v2])[o]

    a = ref.build(*side(1, int(rng.integers(1, 1 << 12))), run_optimize=True)
    b = ref.build(*side(9, int(rng.integers(1, 1 << 12))), run_optimize=True)
    assert any(t == ref.RUN for s in a[0] for _, t, _, _ in s.containers())
    _model_matches(a, b)
    _model_matches(b, a)


def test_merge_reads_back_as_the_union(built):
    rng = np.random.default_rng(7)
    ca, va = random_pairs(rng, (0, 2), 3000, 9)
    cb, vb = random_pairs(rng, (2, 5), 2000, 14)
    keep = ~np.isin(cb, ca)
    cb, vb = cb[keep], vb[keep]
    for ro in (False, True):
        r = ref.merge(ref.build(ca, va, ro), ref.build(cb, vb, ro), ro)
        cols, vals = ref.pairs(r)
        wc, wv = summed((ca, va), (cb, vb))
        assert cols.tolist() == wc and vals == wv and len(r[0]) == 14
    with pytest.raises(ValueError):
        ref.merge(ref.build(ca, va), ref.build(ca[:1], va[:1]))
