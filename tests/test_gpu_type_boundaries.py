"""The container-type decision boundaries of type_boundary_cases.py through every device path that restates the
type rules, byte-exact (RoaringFormatSpec) against the oracle, with rbgpu_pairwise_cardinality equal as well:

  1. the small-batch kernel (k_pair_small): every case as one pair, tables in the kernel arguments (<= 200 pairs)
     and in device memory;
  2. the general pipeline's static schedule: the op's cases repeated in a seeded order to 3 x 4096 pairs, so that
     every wave of the register-path kernel (at most 2048) and of the copy + filter kernel (4096) runs several tasks
     in a row and prefetches across every kind of task; static, in place and cardinality-only;
  3. the queued, concurrent launch from 65,536 tasks up;
  4. one pair of bitmaps that hold case k's operands at key k, through both pair paths;
  5. the wide aggregations over those two bitmaps, with and without the Run-list fast path.
A one-container result's serialized size fixes its type and run count, so the queue test compares the sizes and
cardinalities of all results and the bytes of 20 windows only."""
import numpy as np
import pytest

import type_boundary_cases as tb
from type_pins import ARRAY, BITMAP

pytestmark = pytest.mark.gpu
OPS = tb.OPS
WAVES = 4096  # waves of the copy + filter kernel's grid; the register-path kernel's holds at most 2048
WIDE = {
    "OR": ["FAST_OR", "PAR_OR", "HORIZONTAL_OR", "PQ_OR", "BUFFER_NAIVE_OR", "BUFFER_PQ_OR", "BUFFER_PQ_OR_ITER"],
    "AND": ["FAST_AND", "WORKSHY_AND", "NAIVE_AND", "NAIVE_AND_ITER"],
    "XOR": ["FAST_XOR", "PAR_XOR", "HORIZONTAL_XOR", "PQ_XOR", "BUFFER_PQ_XOR"],
}


@pytest.fixture
def general(monkeypatch):
    monkeypatch.setenv("RBGPU_NO_SMALL_PAIRS", "1")


@pytest.fixture
def small(monkeypatch):
    monkeypatch.setenv("RBGPU_NO_SMALL_PAIRS", "0")
    monkeypatch.setenv("RBGPU_SMALL_KERNEL_TIMES", "1")  # the call's stats then name the kernel that ran


class OpZoo:
    """One op's cases on the device (bitmap 2k = case k's A, 2k + 1 = its B, one container at key 0 each), the
    oracle's copies and its results, computed once.  pairs[j] for j < len(cases) is case j's; after them come
    the mixers: an operand against a partner at key 1, so that the keys are unmatched and OR / XOR clone both
    containers (ANDNOT the left one).  A matched OR / XOR key is a register-path task whatever its types, and
    the concurrent launch needs tasks of both kernels: the queue test adds the mixers for that."""

    def __init__(self, ctx, oracle, opname):
        self.op = OPS[opname]
        self.cases = tb.cases_of(opname)
        n = len(self.cases)
        conts = [x for c in self.cases for x in ((0, c.ta, c.a), (0, c.tb, c.b))]
        rng = np.random.default_rng(4097)
        conts += [(1, ARRAY, np.array([7, 900], np.uint32)),
                  (1, BITMAP, np.sort(rng.choice(65536, 9000, replace=False)).astype(np.uint32))]
        self.s = ctx.upload_soa(tb.keyed_soa([[c] for c in conts]))
        h = self.s.download()
        assert [int(t) for t in h.type] == [t for _, t, _ in conts]
        assert [int(k) for k in h.key] == [k for k, _, _ in conts]
        self.refs = [tb.oracle_keyed(oracle, [c]) for c in conts]
        self.pairs = [(2 * k, 2 * k + 1) for k in range(n)]
        self.labels = [c.id for c in self.cases]
        for k in range(0, n, max(1, n // 16)):  # about 16 cases' operands, left and right of a partner
            self.pairs += [(2 * k, 2 * n), (2 * n + 1, 2 * k + 1)]
            self.labels += [self.cases[k].id + " A | partner", "partner | B " + self.cases[k].id]
        self.want = []
        for x, y in self.pairs:
            w = oracle.op(self.op, self.refs[x], self.refs[y])
            self.want.append((w.serialize(), w.cardinality()))
        self.want_inplace = None
        # the small-batch kernel refuses a SET that holds a Run of more than 2048 runs: its cases in a set of their own
        self.small = np.array([k for k, c in enumerate(self.cases) if c.max_operand_runs <= 2048], np.int64)
        self.s_small = ctx.upload_soa(tb.keyed_soa([[conts[2 * k + i]] for k in self.small.tolist() for i in (0, 1)]))
        self.oracle = oracle

    def inplace(self):
        if self.want_inplace is None:
            self.want_inplace = []
            for x, y in self.pairs[:len(self.cases)]:
                r = self.refs[x].clone()
                self.oracle.op_inplace(self.op, r, self.refs[y])
                self.want_inplace.append((r.serialize(), r.cardinality()))
        return self.want_inplace

    def repeated(self, min_pairs, seed, mixers=False):
        n = len(self.pairs) if mixers else len(self.cases)
        order = np.tile(np.arange(n), -(-min_pairs // len(self.cases)))
        np.random.default_rng(seed).shuffle(order)
        return order

    def idx(self, js):
        p = np.array(self.pairs, np.uint32)[np.asarray(js, np.int64)]
        return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])


@pytest.fixture(scope="module")
def zoo(ctx, oracle):
    made = {}

    def get(opname):
        if opname not in made:
            made[opname] = OpZoo(ctx, oracle, opname)
        return made[opname]
    yield get
    for z in made.values():
        z.s.close()
        z.s_small.close()


@pytest.fixture(scope="module")
def many_keys(ctx, oracle):
    """(device set of two bitmaps, the oracle's two, the number of keys): key k holds case k's operands."""
    made = {}

    def get(opname, small_path_only):
        if (opname, small_path_only) not in made:
            cases = tb.cases_of(opname, small_path_only)
            ca, cb = tb.many_key_bitmaps(cases)
            s = ctx.upload_soa(tb.keyed_soa([ca, cb]))
            refs = [tb.oracle_keyed(oracle, ca), tb.oracle_keyed(oracle, cb)]
            made[(opname, small_path_only)] = (s, refs, len(cases))
        return made[(opname, small_path_only)]
    yield get
    for s, _, _ in made.values():
        s.close()


def _compare(z, ks, got, cards, want, what):
    assert len(got) == len(ks) == len(cards)
    for i, k in enumerate(np.asarray(ks).tolist()):
        assert got[i] == want[k][0], (what, z.labels[k], "at", i)
        assert int(cards[i]) == want[k][1], (what, "card", z.labels[k], "at", i)


def _kernel_names(ctx):
    return [k["name"] for k in ctx.stats()["kernels"]]


# ------------------------------------------------------------------ 1. the small-batch kernel
@pytest.mark.parametrize("opname", list(OPS))
def test_small_batch_kernel(ctx, oracle, zoo, small, opname):
    z = zoo(opname)
    assert {c.id for c in z.cases} - {z.cases[k].id for k in z.small} == \
        {c.id for c in z.cases if c.max_operand_runs > 2048}   # refused by this path: general batches only
    where = np.arange(len(z.small))  # bitmaps 2i, 2i + 1 of s_small are case small[i]'s
    batches = [where[i:i + 200] for i in range(0, len(where), 200)] + [np.tile(where, 2)]
    assert 200 < len(batches[-1]) <= 4096
    for pos in batches:
        ks, ai, bi = z.small[pos], (2 * pos).astype(np.uint32), (2 * pos + 1).astype(np.uint32)
        out = ctx.pairwise(z.op, z.s_small, z.s_small, ai, bi)
        assert _kernel_names(ctx) == ["k_pair_small"]
        got = out.serialize()
        out.close()
        cards = ctx.pairwise_cardinality(z.op, z.s_small, z.s_small, ai, bi)
        assert _kernel_names(ctx) == ["k_pair_small"]
        _compare(z, ks, got, cards, z.want, (opname, "small", len(ks)))
        out = ctx.pairwise_inplace(z.op, z.s_small, z.s_small, ai, bi)
        assert _kernel_names(ctx) == ["k_pair_small"]
        got, cards = out.serialize(), out.cardinalities()
        out.close()
        _compare(z, ks, got, cards, z.inplace(), (opname, "small in place", len(ks)))


# ------------------------------------------------------------------ 2. general pipeline, static schedule
@pytest.mark.parametrize("how", ["static", "inplace", "cardinality"])
@pytest.mark.parametrize("opname", list(OPS))
def test_general_pipeline_static_schedule(ctx, oracle, zoo, general, opname, how):
    z = zoo(opname)
    order = z.repeated(3 * WAVES, seed=101)
    assert len(order) >= 3 * WAVES
    ai, bi = z.idx(order)
    if how == "cardinality":
        cards = ctx.pairwise_cardinality(z.op, z.s, z.s, ai, bi)
        st = ctx.stats()
        for i, k in enumerate(order.tolist()):
            assert int(cards[i]) == z.want[k][1], (opname, "card", z.labels[k], "at", i)
    else:
        want = z.want if how == "static" else z.inplace()
        out = (ctx.pairwise if how == "static" else ctx.pairwise_inplace)(z.op, z.s, z.s, ai, bi)
        st = ctx.stats()
        got = out.serialize()
        cards = out.cardinalities()
        out.close()
        _compare(z, order, got, cards, want, (opname, how))
    assert st["tasks"] == len(order), (st["tasks"], len(order))   # one matched key per pair: the general pipeline ran
    assert "||" not in st["main_kernel"], st["main_kernel"]


# ------------------------------------------------------------------ 3. general pipeline, queued concurrent launch
@pytest.mark.parametrize("opname", list(OPS))
def test_general_pipeline_queued_launch(ctx, oracle, zoo, general, opname):
    z = zoo(opname)
    order = z.repeated(66000, seed=103, mixers=True)
    assert (order < len(z.cases)).sum() >= 66000
    ai, bi = z.idx(order)
    out = ctx.pairwise(z.op, z.s, z.s, ai, bi)
    st = ctx.stats()
    assert st["tasks"] >= 65536, st["tasks"]
    assert "||" in st["main_kernel"], st["main_kernel"]
    want_cards = np.array([w[1] for w in z.want], np.uint64)[order]
    want_sizes = np.array([len(w[0]) for w in z.want], np.uint64)[order]
    assert np.array_equal(out.cardinalities().astype(np.uint64), want_cards)
    assert np.array_equal(out.serialized_sizes().astype(np.uint64), want_sizes)
    cards = ctx.pairwise_cardinality(z.op, z.s, z.s, ai, bi)
    assert np.array_equal(cards[:len(order)].astype(np.uint64), want_cards)
    rng = np.random.default_rng(107)
    checked = 0
    for first in np.sort(rng.choice(len(order) - 50, 20, replace=False)).tolist():
        got = out.serialize(first, 50)
        for i in range(50):
            k = int(order[first + i])
            assert got[i] == z.want[k][0], (opname, z.labels[k], "at", first + i)
            checked += 1
    assert checked == 1000
    out.close()


# ------------------------------------------------------------------ 4. many keys per bitmap
@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("opname", list(OPS))
def test_many_keys_per_bitmap(ctx, oracle, many_keys, monkeypatch, opname, path):
    monkeypatch.setenv("RBGPU_NO_SMALL_PAIRS", "1" if path == "general" else "0")
    monkeypatch.setenv("RBGPU_SMALL_KERNEL_TIMES", "1")
    s, refs, nkeys = many_keys(opname, path == "small")
    assert nkeys >= 100
    op = OPS[opname]
    for x, y in ((0, 1), (1, 0)):
        want = oracle.op(op, refs[x], refs[y])
        out = ctx.pairwise(op, s, s, [x], [y])
        st = ctx.stats()
        if path == "small":
            assert [k["name"] for k in st["kernels"]] == ["k_pair_small"]
        else:
            assert st["tasks"] == nkeys and "k_pair_small" not in [k["name"] for k in st["kernels"]], st
        assert out.serialize()[0] == want.serialize(), (opname, path, x, y)
        out.close()
        assert int(ctx.pairwise_cardinality(op, s, s, [x], [y])[0]) == want.cardinality(), (opname, path, x, y)


# ------------------------------------------------------------------ 5. wide aggregations
@pytest.mark.parametrize("run_fastpath", ["fastpath", "generic"])
@pytest.mark.parametrize("opname", list(WIDE))
def test_wide_aggregations(ctx, oracle, many_keys, monkeypatch, opname, run_fastpath):
    """(14, 7) / (13, 7) and (4096, 7) / (4097, 7) hold at most 8 runs per container: the Run-list fast paths
    (wide_runs.hip, wide_xor.hip) take them, and with RBGPU_NO_RUN_FASTPATH the generic reduce does."""
    import roaringbitmap_amd as rb
    if run_fastpath == "generic":
        monkeypatch.setenv("RBGPU_NO_RUN_FASTPATH", "1")
    else:
        monkeypatch.delenv("RBGPU_NO_RUN_FASTPATH", raising=False)
    s, refs, _ = many_keys(opname, False)
    for sem in WIDE[opname]:
        for members in ((0, 1), (1, 0)):
            want = oracle.wide(getattr(oracle, sem), [refs[m] for m in members]).serialize()
            out = ctx.wide(getattr(rb, sem), s, np.array(members, np.uint32))
            got = out.serialize()[0]
            out.close()
            assert got == want, (opname, sem, members, run_fastpath)
