"""How the task kernels stage an Array or Run operand X in the wave's LDS image and how the Array filter probes
it (wave.hpp: or_chunk_values, toggles_fold_carry_lds, filter_rows_linear's PARITY probe), on the general
pipeline, byte-exact (RoaringFormatSpec) against the oracle with rbgpu_pairwise_cardinality equal as well.

  1. an Array X of 1 .. 4096 values: the chunk edge (7, 8, 9), the row edge (511, 512, 513), all 8 rows;
  2. Array X shapes: all values in one 32-bit word, 0..4095 (adjacent lanes hit the same word), 31/32/63/64/65535;
  3. a Run X (the run lists of light_stage_cases.py) probed at start-1, start, end, end+1 of every run and at
     random positions: the filter reads the carry-folded toggle image by parity;
  4. a Run X of more than 2047 runs (2048 runs, exactly 8 KiB, are the last size staged through the registers;
     from 2049 on it is staged from global memory as membership words) with the same probes;
  5. paths that must still see membership words: OR of a Run or Array into a large Bitmap, and the register
     path's Run AND Bitmap, Run OR Array, Run XOR Run;
  6. all of 1-4 in one batch above the queued, concurrent launch threshold (65,536 tasks).
Every container is uploaded as exactly the type named (one container per bitmap, key 0).  Each batch repeats
its pairs in a seeded order and always holds Bitmap X, Array X and Run X filter tasks, so that one wave meets
all three in a row and the kind of image in its LDS scratch changes under it."""
import numpy as np
import pytest

from light_stage_cases import big_run_lists, edge_probe_values, run_lists, run_values
from type_pins import ARRAY, BITMAP, RUN, one_container_soa, oracle_bitmap, r

pytestmark = pytest.mark.gpu

WAVES = 4096  # 256 CUs x 4 blocks x 4 waves of the copy + filter kernel
X_CARDS = [1, 7, 8, 9, 511, 512, 513, 4096]


@pytest.fixture
def general(monkeypatch):
    monkeypatch.setenv("RBGPU_NO_SMALL_PAIRS", "1")


def _ops():
    import roaringbitmap_amd as rb
    return {"AND": rb.AND, "OR": rb.OR, "XOR": rb.XOR, "ANDNOT": rb.ANDNOT}


def _in_and_out(xvals, card, rng):
    """An Array of `card` values, about half of them members of xvals (where both sides have enough)."""
    outside = np.setdiff1d(r(0, 65536), xvals)
    k = min(len(xvals), (card + 1) // 2, card)
    k = max(k, card - len(outside))
    f = np.concatenate([rng.choice(xvals, k, replace=False), rng.choice(outside, card - k, replace=False)])
    return np.sort(f).astype(np.uint32)


class Zoo:
    """Containers of exact types in one device set, the oracle's copies, and named groups of unique pairs."""

    def __init__(self):
        self.cont, self.groups = [], {}

    def add(self, t, vals):
        self.cont.append((t, np.asarray(vals, np.uint32)))
        return len(self.cont) - 1

    def pair(self, group, a, b):
        self.groups.setdefault(group, []).append((a, b))


def _build_zoo():
    rng = np.random.default_rng(41)
    z = Zoo()
    # ---- 1. Array X cards.  AND of two Arrays stages the LARGER one (A is F on ties), so an F of at most |X|
    #      values keeps X the staged operand; ANDNOT always stages B, whatever F holds.
    for c in X_CARDS:
        x = np.sort(rng.choice(65536, c, replace=False)).astype(np.uint32)
        xi = z.add(ARRAY, x)
        z.pair("array_cards", z.add(ARRAY, _in_and_out(x, min(c, 300), rng)), xi)
        z.pair("array_cards", z.add(ARRAY, x[: max(1, c // 2)]), xi)               # F inside X
        z.pair("array_cards_wide", z.add(ARRAY, _in_and_out(x, 600, rng)), xi)    # two rows of F (X staged by ANDNOT)
    # ---- 2. Array X shapes
    for x in (r(64, 96), r(0, 4096), np.array([31, 32, 63, 64, 65535], np.uint32)):
        xi = z.add(ARRAY, x)
        probes = np.unique(np.clip(np.concatenate([x[:40].astype(np.int64) - 1, x[-40:].astype(np.int64) + 1,
                                                   x[:: max(1, len(x) // 16)].astype(np.int64)]), 0, 65535))
        z.pair("array_shapes", z.add(ARRAY, probes[: len(x)]), xi)
        z.pair("array_shapes", z.add(ARRAY, x[-3:]), xi)
        z.pair("array_shapes_wide", z.add(ARRAY, _in_and_out(x, 700, rng)), xi)
    # ---- 3. / 4. Run X, small and big
    frand = z.add(ARRAY, np.sort(rng.choice(65536, 1000, replace=False)))
    for group, lists in (("runs", run_lists()), ("big_runs", big_run_lists())):
        for _, runs in lists:
            xi = z.add(RUN, run_values(runs))
            z.pair(group, z.add(ARRAY, edge_probe_values(runs)), xi)
            z.pair(group, frand, xi)
    # ---- the three image kinds for every batch
    fmix = z.add(ARRAY, np.sort(rng.choice(65536, 700, replace=False)))
    bmp = z.add(BITMAP, np.sort(rng.choice(65536, 30000, replace=False)))
    arr = z.add(ARRAY, np.sort(rng.choice(65536, 4096, replace=False)))
    run = z.add(RUN, run_values(run_lists()[-3][1]))  # random256
    z.mixers = [(fmix, bmp), (fmix, arr), (fmix, run)]
    # ---- 5. membership-word readers
    full_minus = z.add(BITMAP, np.setdiff1d(r(0, 65536), run_values(run_lists()[-1][1])))  # OR with its Run: full
    run2047 = z.add(RUN, run_values(run_lists()[-1][1]))
    run5 = z.add(RUN, run_values(run_lists()[8][1]))  # random5
    bigrun = z.add(RUN, run_values(big_run_lists()[0][1]))
    for a, b in ((bmp, run), (run, bmp), (bmp, arr), (arr, bmp), (full_minus, run2047), (run2047, full_minus),
                 (bmp, bigrun), (run, arr), (arr, run), (run, run2047), (run5, run), (run2047, arr), (bigrun, run)):
        z.pair("words", a, b)
    return z


@pytest.fixture(scope="module")
def zoo(ctx, oracle):
    z = _build_zoo()
    z.s = ctx.upload_soa(one_container_soa(z.cont))
    h = z.s.download()
    assert [int(t) for t in h.type] == [t for t, _ in z.cont]
    z.refs = [oracle_bitmap(oracle, t, v) for t, v in z.cont]
    z.want = {}
    yield z
    z.s.close()


def _check(ctx, oracle, z, opname, pairs, rng, min_pairs=3 * WAVES):
    """pairwise(op) of the unique pairs repeated in a seeded order: bytes and cardinality of every result
    against the oracle's (computed once per op and unique pair, shared by the tests)."""
    op = _ops()[opname]
    pairs = list(dict.fromkeys(pairs))
    for p in pairs:
        if (opname, p) not in z.want:
            w = oracle.op(op, z.refs[p[0]], z.refs[p[1]])
            z.want[(opname, p)] = (w.serialize(), w.cardinality())
    order = np.tile(np.arange(len(pairs)), -(-min_pairs // len(pairs)))
    rng.shuffle(order)
    ai = np.array([p[0] for p in pairs], np.uint32)[order]
    bi = np.array([p[1] for p in pairs], np.uint32)[order]
    out = ctx.pairwise(op, z.s, z.s, ai, bi)
    st = ctx.stats()
    got = out.serialize()
    cards = ctx.pairwise_cardinality(op, z.s, z.s, ai, bi)
    out.close()
    assert len(got) == len(order)
    for k, j in enumerate(order.tolist()):
        want = z.want[(opname, pairs[j])]
        assert got[k] == want[0], (opname, "pair", pairs[j], "at", k)
        assert int(cards[k]) == want[1], (opname, "card", pairs[j], "at", k)
    return st


def _swapped(pairs):
    return [(b, a) for a, b in pairs]


@pytest.mark.parametrize("opname", ["AND", "ANDNOT"])
@pytest.mark.parametrize("group", ["array_cards", "array_shapes"])
def test_array_x_staging(ctx, oracle, general, zoo, group, opname):
    pairs = zoo.groups[group] + zoo.groups[group + "_wide"] + zoo.mixers
    if opname == "AND":
        pairs = pairs + _swapped(zoo.groups[group])  # X on the left
    _check(ctx, oracle, zoo, opname, pairs, np.random.default_rng(3))


@pytest.mark.parametrize("opname", ["AND", "ANDNOT"])
@pytest.mark.parametrize("group", ["runs", "big_runs"])
def test_run_x_parity_probe(ctx, oracle, general, zoo, group, opname):
    pairs = zoo.groups[group] + zoo.mixers
    if opname == "AND":
        pairs = pairs + _swapped(zoo.groups[group])
    _check(ctx, oracle, zoo, opname, pairs, np.random.default_rng(5))


@pytest.mark.parametrize("opname", ["AND", "OR", "XOR", "ANDNOT"])
def test_membership_word_readers(ctx, oracle, general, zoo, opname):
    """OR: the Bitmap pairs are the copy + filter kernel's OR-into-Bitmap tasks; the rest of the list runs on
    the register path.  The mixers keep Run X filter tasks (folded images) beside them for AND / ANDNOT."""
    _check(ctx, oracle, zoo, opname, zoo.groups["words"] + zoo.mixers, np.random.default_rng(7))


@pytest.mark.parametrize("opname", ["AND", "ANDNOT"])
def test_all_of_it_on_the_queue_path(ctx, oracle, general, zoo, opname):
    pairs = [p for g in ("array_cards", "array_cards_wide", "array_shapes", "array_shapes_wide", "runs", "big_runs",
                         "words") for p in zoo.groups[g]] + zoo.mixers
    st = _check(ctx, oracle, zoo, opname, pairs, np.random.default_rng(9), min_pairs=66000)
    assert st["tasks"] >= 65536, st["tasks"]
    assert "||" in st["main_kernel"], st["main_kernel"]
