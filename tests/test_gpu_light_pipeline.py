"""The copy + filter task kernel's software pipeline (k_pair_tasks<.., kRoleLight>) on the general pipeline:
the places where its prefetched payload rows, its row-by-row filter and its chunk queue can go wrong, all
byte-exact (RoaringFormatSpec) against the oracle, with rbgpu_pairwise_cardinality equal as well.

  1. the rows of F: an Array F of 1 .. 4096 values spans 1 .. 8 rows of 512 values (the eighth, above 3584,
     is the row the kernel once kept in scratch), filtered against every kind of X;
  2. copies of payloads up to and past the 7 KiB and 8 KiB marks;
  3. the queued, concurrent launch taken from 65,536 tasks up.
Each batch repeats its pairs in a seeded order so that a wave meets several tasks in a row (the kernel's grid
holds 4096 waves) and the next task's prefetch crosses every kind of task."""
import numpy as np
import pytest

from type_pins import ARRAY, RUN, one_container_soa, oracle_bitmap, r, u

pytestmark = pytest.mark.gpu

F_CARDS = [1, 8, 511, 512, 513, 3584, 3585, 4095, 4096]
WAVES = 4096  # 256 CUs x 4 blocks x 4 waves of the copy + filter kernel


@pytest.fixture
def general(monkeypatch):
    monkeypatch.setenv("RBGPU_NO_SMALL_PAIRS", "1")


def _ops():
    import roaringbitmap_amd as rb
    return {"AND": rb.AND, "OR": rb.OR, "XOR": rb.XOR, "ANDNOT": rb.ANDNOT}


def _runs(nruns, length, gap, first=3):
    """nruns runs of `length` values, `gap` apart."""
    return u(*[r(first + k * gap, first + k * gap + length) for k in range(nruns)])


def _repeat(n_unique, rng):
    """Each unique pair at least 3 x WAVES / n_unique times, shuffled."""
    rep = -(-3 * WAVES // n_unique)
    order = np.tile(np.arange(n_unique), rep)
    rng.shuffle(order)
    return order


def _check(ctx, oracle, op, sa, sb, ai, bi, refs_a, refs_b, order, what):
    """pairwise(op) of the unique pairs (ai[k], bi[k]) repeated in `order`: bytes and cardinality of every
    result against the oracle's, computed once per unique pair."""
    want = []
    for x, y in zip(ai.tolist(), bi.tolist()):
        w = oracle.op(op, refs_a[x], refs_b[y])
        want.append((w.serialize(), w.cardinality()))
    assert len(ai) == len(bi) > 0 and len(order) >= 3 * WAVES
    ai_r, bi_r = ai[order].astype(np.uint32), bi[order].astype(np.uint32)
    out = ctx.pairwise(op, sa, sb, ai_r, bi_r)
    got = out.serialize()
    cards = ctx.pairwise_cardinality(op, sa, sb, ai_r, bi_r)
    out.close()
    assert len(got) == len(order)
    for k, j in enumerate(order.tolist()):
        assert got[k] == want[j][0], (what, "pair", int(ai[j]), int(bi[j]), "at", k)
        assert int(cards[k]) == want[j][1], (what, "card", int(ai[j]), int(bi[j]), "at", k)


# ------------------------------------------------------------------ 1. row boundaries of F
def _x_zoo():
    """(name, values, canonical): the other operand X of the filter.  The last two are Runs of more than 2047 runs,
    which no runOptimize'd bitmap holds (a Bitmap is smaller): they are uploaded as that container type.  2049
    runs is the first size over 8 KiB (2048 runs are exactly 8192 B: still staged through the registers)."""
    rng = np.random.default_rng(11)
    return [
        ("bitmap", np.sort(rng.choice(65536, 30000, replace=False)).astype(np.uint32), True),
        ("array1", np.array([40000], np.uint32), True),
        ("array4096", np.sort(rng.choice(65536, 4096, replace=False)).astype(np.uint32), True),
        ("run1", r(9000, 39000), True),
        ("run2047", _runs(2047, 9, 32), True),     # 18423 values in 8190 B: a Run
        ("run2049", _runs(2049, 7, 31), False),    # 8196 B: the first size staged from global memory (bigq)
        ("run3000", _runs(3000, 7, 21), False),    # 12000 B
    ]


def _f_sets(xvals, rng):
    """Arrays F of every card in F_CARDS against one X: entirely inside X, entirely outside it, and a mix whose
    kept count is no multiple of 8 — where X has the members for it; else a random F over the whole range."""
    inside = xvals
    outside = np.setdiff1d(r(0, 65536), xvals).astype(np.uint32)
    out = []
    for c in F_CARDS:
        if len(inside) >= c:
            out.append(np.sort(rng.choice(inside, c, replace=False)))
            out.append(np.sort(rng.choice(outside, c, replace=False)))
            keep = c // 2 if (c // 2) % 8 else c // 2 + 1       # kept values of the mix: never 0 mod 8
            keep = min(keep, c)
            mix = np.concatenate([rng.choice(inside, keep, replace=False), rng.choice(outside, c - keep, replace=False)])
            out.append(np.sort(mix))
        else:
            out.append(np.sort(rng.choice(65536, c, replace=False)))
            if len(inside) == 1 and c > 1:  # the one member of X among the c values
                f = rng.choice(outside, c - 1, replace=False)
                out.append(np.sort(np.concatenate([f, inside])))
    return [f.astype(np.uint32) for f in out]


@pytest.fixture(scope="module")
def rows(ctx, oracle):
    """One set of canonical bitmaps (every F, every canonical X; one key each) and one holding the big Runs; the
    unique (F, X) pairs as indices; the oracle's bitmaps."""
    rng = np.random.default_rng(5)
    vals, pairs_canon, pairs_big, big = [], [], [], []
    for name, xv, canon in _x_zoo():
        fs = _f_sets(xv, rng)
        if canon:
            xi = len(vals)
            vals.append(xv)
        else:
            xi = len(big)
            big.append(xv)
        for f in fs:
            (pairs_canon if canon else pairs_big).append((len(vals), xi))
            vals.append(f)
    s = ctx.upload_values(vals, run_optimize=True)
    h = s.download()
    for fi, _ in pairs_canon + pairs_big:  # every F is one Array container
        assert int(h.begin[fi + 1] - h.begin[fi]) == 1 and int(h.type[int(h.begin[fi])]) == ARRAY
    sb = ctx.upload_soa(one_container_soa([(RUN, v) for v in big]))
    hb = sb.download()
    assert [int(t) for t in hb.type] == [RUN] * len(big) and [int(n) for n in hb.nruns] == [2049, 3000]
    refs = [oracle.RefBitmap.deserialize(x) for x in s.serialize()]
    refs_big = [oracle_bitmap(oracle, RUN, v) for v in big]
    yield {"s": s, "sb": sb, "refs": refs, "refs_big": refs_big,
           "canon": np.array(pairs_canon, np.int64), "big": np.array(pairs_big, np.int64)}
    s.close()
    sb.close()


@pytest.mark.parametrize("how", ["AND", "AND_swapped", "ANDNOT"])
def test_filter_row_boundaries(ctx, oracle, general, rows, how):
    ops = _ops()
    op = ops["ANDNOT" if how == "ANDNOT" else "AND"]
    rng = np.random.default_rng(17)
    for which, sx, refs_x in (("canon", rows["s"], rows["refs"]), ("big", rows["sb"], rows["refs_big"])):
        fi, xi = rows[which][:, 0], rows[which][:, 1]
        order = _repeat(len(fi), rng)
        if how == "AND_swapped":  # X on the left
            _check(ctx, oracle, op, sx, rows["s"], xi, fi, refs_x, rows["refs"], order, (how, which))
        else:
            _check(ctx, oracle, op, rows["s"], sx, fi, xi, rows["refs"], refs_x, order, (how, which))


# ------------------------------------------------------------------ 2. copies
@pytest.fixture(scope="module")
def copies(ctx, oracle):
    """Bitmaps whose one container sits at key 0, and partners at key 1, so that every pair's keys are
    unmatched and each container the op keeps is cloned: payloads of 8 KiB (Array 4096, Bitmap), of the 7-8 KiB
    row (Runs of 1792 .. 2047 runs) and, uploaded as that type, a Run above 2047 runs (the direct copy)."""
    rng = np.random.default_rng(23)
    pay = [np.sort(rng.choice(65536, 4096, replace=False)).astype(np.uint32),
           np.sort(rng.choice(65536, 20000, replace=False)).astype(np.uint32),
           _runs(1792, 3, 36), _runs(1793, 3, 36), _runs(1900, 3, 34), _runs(2047, 3, 32)]
    partners = [np.array([65536 + 7, 65536 + 900], np.uint32),
                (65536 + np.sort(rng.choice(65536, 3000, replace=False))).astype(np.uint32)]
    s = ctx.upload_values(pay + partners, run_optimize=True)
    h = s.download()
    for i in range(2, 6):
        assert int(h.type[int(h.begin[i])]) == RUN and 1792 <= int(h.nruns[int(h.begin[i])]) <= 2047
    # payloads of 8192 B (2048 runs: the last size copied through the registers), 8196 B, 20000 B and 131072 B
    big = [_runs(2048, 5, 31), _runs(2049, 5, 31), _runs(5000, 2, 13), r(0, 65536, 2)]
    sb = ctx.upload_soa(one_container_soa([(RUN, v) for v in big]))
    refs = [oracle.RefBitmap.deserialize(x) for x in s.serialize()]
    refs_big = [oracle_bitmap(oracle, RUN, v) for v in big]
    yield {"s": s, "sb": sb, "refs": refs, "refs_big": refs_big, "npay": len(pay), "npart": len(partners),
           "nbig": len(big)}
    s.close()
    sb.close()


@pytest.mark.parametrize("opname", ["OR", "XOR", "ANDNOT"])
def test_copies_of_unmatched_containers(ctx, oracle, general, copies, opname):
    op = _ops()[opname]
    c = copies
    rng = np.random.default_rng(29)
    pi = np.repeat(np.arange(c["npay"]), c["npart"])
    qi = c["npay"] + np.tile(np.arange(c["npart"]), c["npay"])
    order = _repeat(len(pi), rng)
    _check(ctx, oracle, op, c["s"], c["s"], pi, qi, c["refs"], c["refs"], order, (opname, "payload left"))
    _check(ctx, oracle, op, c["s"], c["s"], qi, pi, c["refs"], c["refs"], order, (opname, "payload right"))
    bi = np.repeat(np.arange(c["nbig"]), c["npart"])
    qb = c["npay"] + np.tile(np.arange(c["npart"]), c["nbig"])
    order = _repeat(len(bi), rng)
    _check(ctx, oracle, op, c["sb"], c["s"], bi, qb, c["refs_big"], c["refs"], order, (opname, "big left"))
    _check(ctx, oracle, op, c["s"], c["sb"], qb, bi, c["refs"], c["refs_big"], order, (opname, "big right"))


# ------------------------------------------------------------------ 3. the queue path
QUEUE_PAIRS, QUEUE_SEED = 40000, 1234


@pytest.fixture(scope="module")
def posting(ctx, oracle):
    import roaringbitmap_amd as rb
    a, b = ctx.generate(rb.WL_FILTER_POSTING, QUEUE_PAIRS, seed=QUEUE_SEED)
    ra = [oracle.RefBitmap.deserialize(x) for x in a.serialize()]
    rbs = [oracle.RefBitmap.deserialize(x) for x in b.serialize()]
    yield a, b, ra, rbs
    a.close()
    b.close()


@pytest.mark.parametrize("opname", ["AND", "OR", "XOR", "ANDNOT"])
def test_queued_concurrent_launch(ctx, oracle, general, posting, opname):
    """40,000 (filter, posting-list) pairs make about 82k tasks of both kinds: above the 65,536 tasks from
    which the light and heavy kernels run side by side and draw their tasks from the chunk queues."""
    op = _ops()[opname]
    a, b, ra, rbs = posting
    out = ctx.pairwise(op, a, b)
    st = ctx.stats()
    assert st["tasks"] >= 65536, st["tasks"]
    assert "||" in st["main_kernel"], st["main_kernel"]
    got_cards = out.cardinalities()
    cards = ctx.pairwise_cardinality(op, a, b)
    want_cards = np.array([oracle.op_cardinality(op, x, y) for x, y in zip(ra, rbs)], np.uint64)
    assert np.array_equal(got_cards.astype(np.uint64), want_cards)
    assert np.array_equal(cards[:QUEUE_PAIRS].astype(np.uint64), want_cards)
    rng = np.random.default_rng(QUEUE_SEED)
    checked = 0
    for first in np.sort(rng.choice(QUEUE_PAIRS - 50, 20, replace=False)).tolist():  # 20 windows of 50 pairs
        got = out.serialize(first, 50)
        for i in range(50):
            assert got[i] == oracle.op(op, ra[first + i], rbs[first + i]).serialize(), (opname, first + i)
            checked += 1
    assert checked == 1000
    out.close()
