"""The restatement of the range mutations (range_ops_ref.py) against the oracle and a plain numpy model, on the CPU:
value-wise it must agree with the oracle's op(OR | ANDNOT | XOR, x, range bitmap) — the route that gives the right set
and the wrong container types — and with set arithmetic on the values; type-wise it must reproduce the reference's own
30 Container.not / inot pins (range_pins.py).  test_gpu_range_ops.py then holds the device to its bytes."""
import numpy as np
import pytest

import range_ops_ref as ref
from range_ops_ref import ADD, ARRAY, BITMAP, FLIP, REMOVE, RUN
from range_pins import PINS, n_pins

OR, XOR, ANDNOT = 1, 2, 3  # oracle op codes (rb_op)
ORACLE_OP = {ADD: OR, REMOVE: ANDNOT, FLIP: XOR}
FUZZ_SEED, FUZZ_N = 20251021, 360


def test_inventory_accounts_for_all_30_pins():
    assert n_pins() == 30
    assert sum(p.npins for p in PINS if p.cite.startswith("TestContainer.java")) == 27
    assert sum(p.npins for p in PINS if p.cite.startswith("TestRunContainer.java")) == 3


@pytest.mark.parametrize("pin", PINS, ids=[p.name for p in PINS])
def test_restatement_reproduces_the_pin(pin):
    t, vals = pin.input
    vals = np.asarray(vals, dtype=np.uint32)
    got_t, got_v = ref.container_op(pin.op, t, vals, *pin.rng)
    model = np.zeros(65536, bool)
    model[vals] = True
    if pin.op == ADD:
        model[pin.rng[0]:pin.rng[1]] = True
    elif pin.op == REMOVE:
        model[pin.rng[0]:pin.rng[1]] = False
    else:
        model[pin.rng[0]:pin.rng[1]] ^= True
    assert np.array_equal(got_v, np.nonzero(model)[0])
    if pin.expect is not None:
        assert got_t == pin.expect, (pin.name, got_t)
    if pin.card is not None:
        assert len(got_v) == pin.card, (pin.name, len(got_v))
    # the bitmap-level loops give the same container at any key, static and in place
    for key in (0, 7, 65535):
        for inplace in (False, True):
            res = ref.range_op(pin.op, [(key, t, vals)], (key << 16) + pin.rng[0], (key << 16) + pin.rng[1], inplace)
            assert [(k, ty) for k, ty, _ in res] == ([(key, got_t)] if len(got_v) else [])
            assert not res or np.array_equal(res[0][2], got_v)


def _model(conts, op, s, e):
    v = ref.values_of(conts)
    rng = np.arange(s, e, dtype=np.uint64) if s < e else np.zeros(0, np.uint64)
    if op == ADD:
        return np.union1d(v, rng)
    if op == REMOVE:
        return np.setdiff1d(v, rng)
    return np.setxor1d(v, rng)


def test_fuzz_agrees_with_the_oracle_pairwise_route_and_a_value_model(oracle):
    cases = ref.fuzz_cases(FUZZ_SEED, FUZZ_N)
    for conts, op, s, e, inplace in cases:
        if e - s > 4 << 16:  # the value model materialises the range
            continue
        res = ref.range_op(op, conts, s, e, inplace)
        want = _model(conts, op, s, e)
        assert np.array_equal(ref.values_of(res), want), (op, s, e, inplace)
        assert [k for k, _, _ in res] == sorted(k for k, _, _ in res) and all(len(v) for _, _, v in res)
        x = ref.to_oracle(oracle, conts)
        got = ref.to_oracle(oracle, res) if res else oracle.RefBitmap.of(np.zeros(0, np.uint32))
        # the oracle keeps the restatement's container types and cardinalities: its serializer writes these bytes
        assert [(k, t, c) for k, t, c, _ in got.containers()] == [(k, t, len(v)) for k, t, v in res]
        if s < e:
            rb = ref.to_oracle(oracle, ref.bitmap_of_range(s, e))
            assert np.array_equal(oracle.op(ORACLE_OP[op], x, rb).to_array().astype(np.uint64), want)
        else:
            assert got.serialize() == x.serialize()  # an empty range: the bitmap as it is


def test_fuzz_generator_covers_every_transition_of_the_table():
    census = ref.fuzz_census(ref.fuzz_cases(FUZZ_SEED, FUZZ_N))
    assert census <= ref.ALLOWED | {(t, op, t) for t in (ARRAY, BITMAP, RUN) for op in (ADD, REMOVE, FLIP)}, \
        census - ref.ALLOWED
    assert ref.ALLOWED <= census, sorted(ref.ALLOWED - census, key=str)


def test_static_and_inplace_differ_only_inside_an_add_span():
    a = np.array([3, 9], np.uint32)
    b = np.arange(0, 65536, 3, dtype=np.uint32)
    conts = [(1, ARRAY, a), (2, ARRAY, a), (3, BITMAP, b), (4, RUN, np.arange(10, 20, dtype=np.uint32)), (6, ARRAY, a)]
    s, e = (1 << 16) + 5, (6 << 16) + 4
    st, ip = ref.range_op(ADD, conts, s, e), ref.range_op(ADD, conts, s, e, inplace=True)
    assert np.array_equal(ref.values_of(st), ref.values_of(ip))
    assert [(k, t) for k, t, _ in st] == [(1, BITMAP), (2, RUN), (3, RUN), (4, RUN), (5, RUN), (6, ARRAY)]
    assert [(k, t) for k, t, _ in ip] == [(1, BITMAP), (2, BITMAP), (3, BITMAP), (4, RUN), (5, RUN), (6, ARRAY)]
    for op in (REMOVE, FLIP):
        st, ip = ref.range_op(op, conts, s, e), ref.range_op(op, conts, s, e, inplace=True)
        assert [(k, t) for k, t, _ in st] == [(k, t) for k, t, _ in ip]
        assert np.array_equal(ref.values_of(st), ref.values_of(ip))


def test_bitmap_of_range_is_add_on_the_empty_bitmap():
    for lo, hi in [(5, 6), (5, 7), (5, 8), (0, 65536), (65535, 65538), (3, 5 << 16), ((1 << 32) - 2, 1 << 32), (9, 9)]:
        a, b = ref.bitmap_of_range(lo, hi), ref.range_op(ADD, [], lo, hi)
        assert [(k, t) for k, t, _ in a] == [(k, t) for k, t, _ in b]
        assert all(np.array_equal(x[2], y[2]) for x, y in zip(a, b))
    assert [t for _, t, _ in ref.bitmap_of_range(5, 7)] == [ARRAY] and [t for _, t, _ in ref.bitmap_of_range(5, 8)] == [RUN]


def test_range_sanity_check():
    for s, e in [(-1, 5), (1 << 32, (1 << 32) + 1), (0, (1 << 32) + 1), (0, -1)]:
        for op in (ADD, REMOVE, FLIP):
            with pytest.raises(ValueError):
                ref.range_op(op, [], s, e)
