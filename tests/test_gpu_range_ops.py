"""Range mutations on the MI355X: rbgpu_set_range_op / rbgpu_set_range_op_inplace, Context.range_op and
RoaringBitmap.add / remove / flip / bitmapOfRange.  Every case compares the serialized bytes and the cardinality of the
device result with the restatement of the reference (range_ops_ref.py), whose own agreement with the oracle and with
the reference's 30 type pins test_range_ops_oracle.py checks on the CPU.  Shapes are the smallest that reach each
decision: every (source type, op) over the word, lane and container boundaries of the register image, the 4096 / 4097
and toEfficientContainer thresholds from both sides, results of 0 and of 65536 values, and the bitmap-level loop over
present and absent keys."""
import numpy as np
import pytest

import range_ops_ref as ref
from datasets import ornot_fuzz_bitmaps
from range_ops_ref import ADD, ARRAY, BITMAP, FLIP, FULL, REMOVE, RUN
from range_pins import PINS
from test_range_ops_oracle import FUZZ_N, FUZZ_SEED
from type_boundary_cases import keyed_soa

pytestmark = pytest.mark.gpu
OPS = [ADD, REMOVE, FLIP]
OP_NAME = {ADD: "add", REMOVE: "remove", FLIP: "flip"}


def r(a, b, step=1):
    return np.arange(a, b, step, dtype=np.uint32)


def u(*parts):
    return np.unique(np.concatenate([np.asarray(p, dtype=np.uint32) for p in parts]))


def want_bytes(oracle, conts) -> bytes:
    return (ref.to_oracle(oracle, conts) if conts else oracle.RefBitmap.of(np.zeros(0, np.uint32))).serialize()


def check(ctx, oracle, bitmaps, op, starts, ends, members=None, inplace=False, dset=None):
    """One device call over `bitmaps` (lists of (key, type, values)); every result against the restatement."""
    s = dset if dset is not None else ctx.upload_soa(keyed_soa(bitmaps))
    before = s.serialize()
    out = ctx.range_op(op, s, starts, ends, members=members, inplace=inplace)
    idx = list(range(len(bitmaps))) if members is None else list(members)
    assert len(out) == len(idx)
    got, cards = out.serialize(), out.cardinalities()
    results = []
    for i, m in enumerate(idx):
        res = ref.range_op(op, bitmaps[m], int(starts[i]), int(ends[i]), inplace)
        assert got[i] == want_bytes(oracle, res), (OP_NAME[op], inplace, i, m, int(starts[i]), int(ends[i]),
                                                   [(k, t, len(v)) for k, t, v in res][:8])
        assert int(cards[i]) == ref.cardinality(res)
        results.append(res)
    assert s.serialize() == before  # the input set is unchanged
    return results


# ------------------------------------------------------------------------------------------- container matrix
SOURCES = {
    ARRAY: u(r(0, 65536, 37), [0, 1, 62, 63, 64, 65, 127, 128, 1022, 1023, 1024, 1025, 2047, 2048, 65534, 65535]),
    BITMAP: u(r(0, 65536, 3), r(60, 70), r(1020, 1030), r(2040, 2050), [0, 1, 65534, 65535]),
    RUN: u(r(0, 2), r(40, 70), r(100, 1024), r(1025, 3000), r(65000, 65536)),
}
POSITIONS = [(500, 500), (9000, 9001), (9000, 9002), (9000, 9003), (0, 1), (63, 65), (64, 128), (1023, 1025),
             (1024, 2048), (0, 65536), (65535, 65536), (1, 65535)]


@pytest.mark.parametrize("inplace", [False, True], ids=["static", "inplace"])
@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
def test_container_matrix(ctx, oracle, op, inplace):
    """Array / Bitmap / Run x every range position inside one key, with a copied container on either side."""
    side = (ARRAY, np.array([7, 65535], np.uint32))
    bitmaps = [[(3,) + side, (5, t, v), (9,) + side] for t, v in SOURCES.items()]
    members, starts, ends = [], [], []
    for m in range(len(bitmaps)):
        for b, e in POSITIONS:
            members.append(m)
            starts.append((5 << 16) + b)
            ends.append((5 << 16) + e)
    res = check(ctx, oracle, bitmaps, op, starts, ends, members, inplace)
    # an absent key under the same positions: Container.rangeOfOnes
    lone = [[(3,) + side, (9,) + side]]
    res += check(ctx, oracle, lone, op, starts[:len(POSITIONS)], ends[:len(POSITIONS)], [0] * len(POSITIONS), inplace)
    if op != REMOVE:
        fresh = {len(x[1][2]): x[1][1] for x in res[-len(POSITIONS):] if len(x) == 3}
        assert fresh[1] == ARRAY and fresh[2] == ARRAY and fresh[3] == RUN and fresh[65536] == RUN


# ------------------------------------------------------------------------------------------- thresholds
A4000 = r(0, 8000, 2)
B5000 = r(0, 5000)
PAIRS = lambda n: u(5 * r(0, n), 5 * r(0, n) + 1)          # n runs of 2: 2 + 4 r against 2 + 2 c is a tie
TRIPLES = lambda n: u(8 * r(0, n), 8 * r(0, n) + 1, 8 * r(0, n) + 2)
# (name, source (type, values), op, [b, e), expected type or None = dropped, expected cardinality)
THRESHOLDS = [
    ("array.add->4096", (ARRAY, A4000), ADD, (9000, 9096), ARRAY, 4096),
    ("array.add->4097", (ARRAY, A4000), ADD, (9000, 9097), BITMAP, 4097),
    ("array.flip->4096", (ARRAY, A4000), FLIP, (9000, 9096), ARRAY, 4096),
    ("array.flip->4097", (ARRAY, A4000), FLIP, (9000, 9097), BITMAP, 4097),
    ("bitmap.remove->4096", (BITMAP, B5000), REMOVE, (4096, 5000), ARRAY, 4096),
    ("bitmap.remove->4097", (BITMAP, B5000), REMOVE, (4097, 5000), BITMAP, 4097),
    ("bitmap.flip->4096", (BITMAP, B5000), FLIP, (4096, 5000), ARRAY, 4096),
    ("bitmap.flip->4097", (BITMAP, B5000), FLIP, (4097, 5000), BITMAP, 4097),
    ("array.remove->0", (ARRAY, r(5, 8)), REMOVE, (5, 8), None, 0),
    ("array.flip->0", (ARRAY, r(5, 8)), FLIP, (5, 8), None, 0),
    ("bitmap.remove->0", (BITMAP, r(100, 5000)), REMOVE, (64, 5001), None, 0),
    ("bitmap.flip->0", (BITMAP, r(100, 5000)), FLIP, (100, 5000), None, 0),
    ("run.remove->0", (RUN, u(r(10, 20), r(30, 40))), REMOVE, (10, 40), None, 0),
    ("run.flip->0", (RUN, r(1024, 4096)), FLIP, (1024, 4096), None, 0),
    ("array.add->65536", (ARRAY, r(5, 8)), ADD, (0, 65536), BITMAP, 65536),
    ("bitmap.add->65536", (BITMAP, B5000), ADD, (4000, 65536), BITMAP, 65536),
    ("bitmap.flip->65536", (BITMAP, r(0, 60000)), FLIP, (60000, 65536), BITMAP, 65536),
    ("run.add->65536", (RUN, r(0, 60000)), ADD, (59990, 65536), RUN, 65536),
    ("run.flip->65536", (RUN, r(0, 60000)), FLIP, (60000, 65536), RUN, 65536),
    # toEfficientContainer through Run.flip.  The Array bound, 2 + 4 r against 2 + 2 c: below, at, above
    ("eff.array/run-side", (RUN, PAIRS(40)), FLIP, (1002, 1005), RUN, 83),
    ("eff.array/tie", (RUN, PAIRS(40)), FLIP, (1002, 1004), RUN, 82),
    ("eff.array/array-side", (RUN, PAIRS(40)), FLIP, (1002, 1003), ARRAY, 81),
    # the Bitmap bound, 2 + 4 r against 8192 (no r meets it exactly: 2047 runs are 8190 bytes, 2048 are 8194)
    ("eff.bitmap/2047", (RUN, TRIPLES(2046)), FLIP, (30000, 30003), RUN, 3 * 2047),
    ("eff.bitmap/2048", (RUN, TRIPLES(2047)), FLIP, (30000, 30003), BITMAP, 3 * 2048),
    ("eff.bitmap/2048-split", (RUN, TRIPLES(2047)), FLIP, (9, 10), BITMAP, 3 * 2047 - 1),
    # a Run larger than the Bitmap of its set stays a Run under add / remove
    ("run.add/3001-runs", (RUN, PAIRS(3000)), ADD, (30000, 30002), RUN, 6002),
    ("run.remove/3001-runs", (RUN, PAIRS(3000)), REMOVE, (10000, 10001), RUN, 5999),
]


def test_thresholds(ctx, oracle):
    for inplace in (False, True):
        for op in OPS:
            rows = [t for t in THRESHOLDS if t[2] == op]
            # alone in its bitmap (an emptied container leaves an empty bitmap), and between two other keys
            bitmaps = [[(7,) + src] for _, src, _, _, _, _ in rows] + \
                      [[(2, ARRAY, r(1, 3)), (7,) + src, (8, RUN, r(0, 9))] for _, src, _, _, _, _ in rows]
            starts = [(7 << 16) + rg[0] for _, _, _, rg, _, _ in rows] * 2
            ends = [(7 << 16) + rg[1] for _, _, _, rg, _, _ in rows] * 2
            res = check(ctx, oracle, bitmaps, op, starts, ends, inplace=inplace)
            for i, (name, _, _, _, ty, card) in enumerate(rows):
                for got in (res[i], res[len(rows) + i]):
                    at7 = [(t, len(v)) for k, t, v in got if k == 7]
                    assert at7 == ([(ty, card)] if ty is not None else []), (name, at7)
                assert len(res[i]) == (ty is not None) and len(res[len(rows) + i]) == 2 + (ty is not None)


# ------------------------------------------------------------------------------------------- run adjacency
def test_run_adjacency(ctx, oracle):
    """Run.add / remove keep the reference's maximal run list: (range, op, runs afterwards)."""
    src = (RUN, u(r(100, 200), r(300, 400)))
    rows = [((50, 100), ADD, 2), ((200, 250), ADD, 2), ((200, 300), ADD, 1), ((120, 150), ADD, 2), ((99, 100), ADD, 2),
            ((200, 201), ADD, 2), ((98, 99), ADD, 3), ((150, 160), REMOVE, 3), ((100, 120), REMOVE, 2),
            ((180, 200), REMOVE, 2), ((300, 400), REMOVE, 1), ((350, 65536), REMOVE, 2), ((0, 301), REMOVE, 1),
            ((150, 151), REMOVE, 3), ((100, 101), REMOVE, 2)]
    for inplace in (False, True):
        for op in (ADD, REMOVE):
            sel = [x for x in rows if x[1] == op]
            res = check(ctx, oracle, [[(1,) + src]], op, [(1 << 16) + x[0][0] for x in sel],
                        [(1 << 16) + x[0][1] for x in sel], [0] * len(sel), inplace)
            for x, got in zip(sel, res):
                assert [(t, ref.n_runs(v)) for _, t, v in got] == [(RUN, x[2])], x


# ------------------------------------------------------------------------------------------- bitmap level
def _mixed(keys):
    shapes = [(ARRAY, u(r(0, 65536, 41), [0, 65535])), (BITMAP, u(r(0, 65536, 2), [65535])), (RUN, u(r(0, 300), r(65000, 65536))),
              (RUN, FULL), (BITMAP, r(0, 65535)), (ARRAY, r(65530, 65536))]
    return [(k,) + shapes[i % len(shapes)] for i, k in enumerate(keys)]


@pytest.mark.parametrize("inplace", [False, True], ids=["static", "inplace"])
@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
def test_bitmap_level(ctx, oracle, op, inplace):
    K = 1 << 16
    mixed = _mixed([2, 3, 5, 6, 7, 11, 12, 20, 21, 40])
    top = _mixed([65533, 65535])
    no_top = _mixed([65533, 65534])
    full = [(4, RUN, FULL), (5, BITMAP, FULL), (6, RUN, FULL)]
    edges = [(4, ARRAY, r(65000, 65536)), (5, BITMAP, r(0, 65536, 2)), (6, RUN, r(0, 100)), (9, ARRAY, r(1, 3))]
    cases = [
        (mixed, 5 * K + 100, 5 * K + 40000),           # inside one key
        (mixed, 5 * K + 100, 6 * K + 40000),           # across two keys
        (mixed, 1 * K + 7, 30 * K + 9),                # many keys, present and absent in the middle
        (mixed, 0, 50 * K),                            # before the first key to past the last
        (mixed, 3 * K, 12 * K),                        # lbStart == 0 and lbLast == 0xFFFF
        (mixed, 3 * K, 4 * K),                         # exactly one whole container
        (mixed, 4 * K, 5 * K),                         # exactly one absent key
        (mixed, 8 * K + 5, 10 * K + 5),                # absent keys only
        (top, 65534 * K + 9, 1 << 32),                 # to 2^32, key 65535 present
        (no_top, 65534 * K + 9, 1 << 32),              # to 2^32, key 65535 absent
        (top, (1 << 32) - 1, 1 << 32),                 # the last value alone
        (full, 4 * K, 7 * K),                          # exactly its own full containers: flip and remove empty it
        (full, 4 * K + 1, 7 * K - 1),
        (edges, 4 * K + 65000, 6 * K + 100),           # the edge containers empty out under remove
        (edges, 4 * K + 64000, 6 * K + 200),
        ([], 0, 1 << 32),                              # the empty bitmap over the whole universe
        ([], 70000, 70002),
        ([], 65534, 65537),
    ]
    bitmaps = [c[0] for c in cases]
    res = check(ctx, oracle, bitmaps, op, [c[1] for c in cases], [c[2] for c in cases], inplace=inplace)
    whole = res[15]
    if op == REMOVE:
        assert whole == [] and res[11] == [] and [k for k, _, _ in res[13]] == [9]
    else:
        assert len(whole) == 65536 and all(t == RUN for _, t, _ in whole) and ref.cardinality(whole) == 1 << 32
    if op == FLIP:
        assert res[11] == []


# ------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("inplace", [False, True], ids=["static", "inplace"])
@pytest.mark.parametrize("op", OPS, ids=[OP_NAME[o] for o in OPS])
def test_batch(ctx, oracle, op, inplace):
    """One call, 96 results: distinct ranges, repeated members, empty ranges mixed in, an empty input bitmap."""
    rng = np.random.default_rng(77 + op)
    bitmaps = [_mixed(sorted(rng.choice(40, size=int(rng.integers(1, 9)), replace=False).tolist())) for _ in range(11)]
    bitmaps.insert(4, [])
    members = rng.integers(0, len(bitmaps), size=96)
    members[:3] = 4
    starts = rng.integers(0, 42 << 16, size=96)
    ends = starts + rng.integers(1, 6 << 16, size=96)
    ends[::7] = starts[::7] - rng.integers(0, 3, size=len(ends[::7]))  # empty ranges: clones
    ends = np.maximum(ends, 0)
    check(ctx, oracle, bitmaps, op, starts, ends, members.tolist(), inplace)


# ------------------------------------------------------------------------------------------- pins, real data, fuzz
def test_reference_pins_through_the_device(ctx, oracle):
    for op in OPS:
        for inplace in (False, True):
            pins = [p for p in PINS if p.op == op and p.inplace == inplace]
            if not pins:
                continue
            bitmaps = [[(0, p.input[0], np.asarray(p.input[1], dtype=np.uint32))] for p in pins]
            res = check(ctx, oracle, bitmaps, op, [p.rng[0] for p in pins], [p.rng[1] for p in pins], inplace=inplace)
            for p, got in zip(pins, res):
                if p.expect is not None:
                    assert [t for _, t, _ in got] == [p.expect], p.name
                if p.card is not None:
                    assert ref.cardinality(got) == p.card, p.name


def test_real_mixed_bitmaps(ctx, oracle):
    """flip(0, limit), add and remove over the two bitmaps of ornot-fuzz-failure.json (181 and 374 containers of all
    three types)."""
    blobs = ornot_fuzz_bitmaps()
    refs = [oracle.RefBitmap.deserialize(b) for b in blobs]
    bitmaps = [ref.conts_of(x) for x in refs]
    assert {t for b in bitmaps for _, t, _ in b} == {ARRAY, BITMAP, RUN}
    dset = ctx.upload_serialized(list(blobs))
    last = max(int(x.to_array()[-1]) for x in refs)
    first = min(int(x.to_array()[0]) for x in refs)
    mid = (first + last) // 2
    ranges = [(0, last + 1), (0, mid), (mid, min(last + 70000, 1 << 32)), (first + 5, first + 3 * 65536 + 11)]
    for op in OPS:
        for inplace in (False, True):
            members = [m for m in (0, 1) for _ in ranges]
            check(ctx, oracle, bitmaps, op, [s for s, _ in ranges] * 2, [e for _, e in ranges] * 2, members, inplace,
                  dset=dset)


def test_seeded_fuzz(ctx, oracle):
    cases = ref.fuzz_cases(FUZZ_SEED, FUZZ_N)
    # a weaker generator cannot pass quietly: these inputs reach every transition the type table allows
    assert ref.ALLOWED <= ref.fuzz_census(cases)
    for op in OPS:
        for inplace in (False, True):
            sel = [c for c in cases if c[1] == op and c[4] == inplace]
            check(ctx, oracle, [c[0] for c in sel], op, [c[2] for c in sel], [c[3] for c in sel], inplace=inplace)


# ------------------------------------------------------------------------------------------- the Python surface
def test_roaring_bitmap_static_and_inplace_forms(ctx, oracle):
    import roaringbitmap_amd as rb
    vals = u(r(10, 5000, 3), r(70000, 140000), r(400000, 400003), [1 << 20, (1 << 32) - 1])
    want = {ADD: ref.static_add, REMOVE: ref.static_remove, FLIP: ref.static_flip}
    conts = ref.conts_of(oracle.RefBitmap.of(vals))
    for s, e in [(20, 66000), (69999, 140001), (0, 1 << 32), (500, 500), ((1 << 32) - 1, 1 << 32)]:
        for op, name in OP_NAME.items():
            x = rb.RoaringBitmap.bitmapOf(vals)
            before = x.serialize()
            y = getattr(rb.RoaringBitmap, name)(x, s, e)
            assert x.serialize() == before  # the operand of a static call is unchanged
            assert y.serialize() == want_bytes(oracle, want[op](conts, s, e))
            assert getattr(x, name)(s, e) is None
            assert x.serialize() == want_bytes(oracle, ref.range_op(op, conts, s, e, inplace=True))
            if op != ADD:
                assert x.serialize() == y.serialize()
            assert x.getCardinality() == y.getCardinality()
    z = rb.RoaringBitmap.bitmapOfRange(65530, 3 * 65536 + 2)
    assert z.serialize() == want_bytes(oracle, ref.bitmap_of_range(65530, 3 * 65536 + 2))
    assert rb.RoaringBitmap.bitmapOfRange(9, 9).isEmpty()
    assert z.contains(65530, 3 * 65536 + 2) and not z.contains(65529, 65540) and not z.contains(5, 5)
    assert z.intersects(0, 65531) and not z.intersects(0, 65530) and not z.intersects(70000, 70000)
    assert z.contains(65530) and not z.contains(65529)  # the single-value form as before
    with pytest.raises(TypeError):
        z.add(5)


def test_out_of_range_arguments_raise_and_leave_no_result(ctx):
    import ctypes as C

    import roaringbitmap_amd as rb
    from roaringbitmap_amd import _lib as L
    s = ctx.upload_values([np.array([1, 2, 3], np.uint32), np.array([9], np.uint32)])
    for start, end in [(-1, 5), (1 << 32, (1 << 32) + 1), (0, (1 << 32) + 1), (5, -1)]:
        for op in OPS:
            with pytest.raises(ValueError):
                ctx.range_op(op, s, [0, start], [10, end])
            for name in OP_NAME.values():
                x = rb.RoaringBitmap.bitmapOf(1, 2, 3)
                before = x.serialize()
                with pytest.raises(ValueError):
                    getattr(x, name)(start, end)
                with pytest.raises(ValueError):
                    getattr(rb.RoaringBitmap, name)(x, start, end)
                assert x.serialize() == before
    with pytest.raises(ValueError):
        rb.RoaringBitmap.bitmapOfRange(0, (1 << 32) + 1)
    with pytest.raises(ValueError):
        rb.RoaringBitmap.bitmapOf(1).contains(-1, 4)
    with pytest.raises(ValueError):
        ctx.range_op(ADD, s, 0, 5, members=[0, 2])  # a member the set does not hold
    with pytest.raises(ValueError):
        ctx.range_op(7, s, 0, 5)
    # the C entry itself: one bad range fails the whole call and creates nothing
    start = np.array([0, 1 << 32], np.uint64)
    end = np.array([10, (1 << 32) + 4], np.uint64)
    for fn in (L.lib().rbgpu_set_range_op, L.lib().rbgpu_set_range_op_inplace):
        out = C.c_void_p(12345)
        assert fn(ctx.h, FLIP, s.h, None, start.ctypes.data, end.ctypes.data, 2, C.byref(out)) == L.RB_EINVAL
        assert not out.value
    assert ctx.range_op(FLIP, s, [0, 0], [4, 0]).serialize()[1] == s.serialize()[1]  # the context still works
