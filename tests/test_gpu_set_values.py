"""The value read-out of plain sets on the MI355X: rbgpu_set_values / rbgpu_set_values_device / rbgpu_set_contains /
rbgpu_set_rank / rbgpu_set_select and the RoaringBitmap mirror (toArray, contains, rank, select, first, last,
rangeCardinality).  Every comparison is exact and is made against two expectations: the numpy arrays the bitmaps were
built from, and oracle.RefBitmap.deserialize(bytes).to_array() of the uploaded set's own serialization.  Rank is
np.searchsorted(v, x, "right"), select is v[j], contains is np.isin.

The containers of the "typed" set are built as host SoA with the type stated, and the type is asserted from the
downloaded metadata.  One container the list of cases names cannot exist: a Bitmap with bits only in word 0 and
word 1023 would hold at most 128 values, and the library refuses a Bitmap of cardinality <= 4096 as non-canonical
(as the reference never builds one).  "b_ends" stands in for it: word 0 and words 960..1023 full and nothing
between, so step 0 of the decode holds one word, steps 1..14 are empty and step 15 fills the whole 4096-value window;
"b_sparse_ends" holds bit 0 of word 0 and bit 63 of word 1023 around a dense middle."""
import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L
from roaringbitmap_amd.engine import HostSoA, _runs_of_sorted

pytestmark = pytest.mark.gpu

A, B, R = rb.ARRAY, rb.BITMAP, rb.RUN
U32 = 2**32 - 1
BATCHES = [0, 1, 63, 257, 1000]


def _rng(seed):
    return np.random.default_rng(seed)


def _pick(seed, n, lo=0, hi=65536):
    return np.sort(_rng(seed).choice(np.arange(lo, hi), size=n, replace=False))


def _runs(nruns, length, stride, start=0):
    return (start + stride * np.arange(nruns)[:, None] + np.arange(length)[None, :]).ravel()


# (name, key, type, low values): one container per key, gaps between the keys, keys 0 and 65535 at the ends
ZOO = [
    ("a1", 0, A, np.array([0])),
    ("a63", 3, A, _pick(1, 63)),
    ("a64", 5, A, _pick(2, 64)),
    ("a65", 6, A, _pick(3, 65)),
    ("a4096", 9, A, _pick(4, 4096)),
    ("b4097", 12, B, _pick(5, 4097)),
    ("b_ends", 13, B, np.concatenate([np.arange(64), np.arange(960 * 64, 65536)])),
    ("b_sparse_ends", 14, B, np.unique(np.concatenate([[0, 65535], _pick(6, 4200, 400 * 64, 600 * 64)]))),
    ("b_63_0", 20, B, np.unique(np.concatenate([64 * np.arange(1023) + 63, 64 * np.arange(1023) + 64,
                                                 64 * np.arange(1024) + 10, 64 * np.arange(1024) + 31,
                                                 64 * np.arange(1024) + 32]))),
    ("b_full", 21, B, np.arange(65536)),
    ("r_one", 30, R, np.array([777])),
    ("r_whole", 31, R, np.arange(65536)),
    ("r65", 40, R, _runs(65, 5, 900, 11)),
    ("r130", 41, R, _runs(130, 2, 500, 1)),
    ("r2047", 50, R, _runs(2047, 3, 32)),
    ("r3000", 51, R, _runs(3000, 2, 16, 7)),
    ("r_last", 65535, R, np.array([65535])),
]
SMALL = [("s_a", 2, A, np.array([5, 9, 65535])), ("s_r", 9, R, np.arange(100, 40000)), ("s_b", 10, B, _pick(7, 30000))]


def _typed_soa(bitmaps) -> HostSoA:
    """Host SoA of bitmaps given as lists of (name, key, type, low values): every container with the type stated."""
    begin, key, typ, card, nruns, off, chunks, pos = [0], [], [], [], [], [], [], 0
    for conts in bitmaps:
        for _, k, t, low in conts:
            low = np.unique(np.asarray(low)).astype(np.uint16)
            if t == A:
                data, r = low.tobytes(), 0
            elif t == B:
                bits = np.zeros(65536, np.uint8)
                bits[low] = 1
                data, r = np.packbits(bits, bitorder="little").tobytes(), 0
            else:
                runs = _runs_of_sorted(low)
                data, r = runs.tobytes(), len(runs)
            key.append(k), typ.append(t), card.append(len(low)), nruns.append(r), off.append(pos)
            data += b"\0" * ((-len(data)) % 16)
            chunks.append(data)
            pos += len(data)
        begin.append(len(key))
    return HostSoA(np.array(begin, np.uint64), np.array(key, np.uint16), np.array(typ, np.uint8),
                   np.array(card, np.uint32), np.array(nruns, np.uint16), np.array(off, np.uint64),
                   np.frombuffer(b"".join(chunks) or b"\0" * 16, np.uint8).copy())


def _cat(arrays) -> np.ndarray:
    return np.concatenate(arrays) if len(arrays) else np.zeros(0, np.uint32)


def _values_of(conts) -> np.ndarray:
    if not conts:
        return np.zeros(0, np.uint32)
    return np.concatenate([(np.unique(np.asarray(low)).astype(np.uint32) | np.uint32(k << 16))
                           for _, k, _, low in conts])


def _plain_bitmaps():
    """Six bitmaps with an empty one in the middle: the zoo's values, sparse keys with gaps, dense keys, long ranges
    and the single value 2^32 - 1."""
    rng = _rng(21)
    sparse = np.concatenate([(k << 16) + rng.integers(0, 65536, 80) for k in (1, 2, 7, 65534)])
    dense = np.concatenate([(k << 16) + _pick(30 + k, 30000) for k in (100, 101, 103)] + [np.arange(104 << 16, 6900000)])
    return [_values_of(ZOO), np.unique(sparse).astype(np.uint32), np.zeros(0, np.uint32),
            np.unique(dense).astype(np.uint32), np.arange(70000, 300000, dtype=np.uint32), np.array([U32], np.uint32)]


class Case:
    """A device set, the numpy values of its bitmaps and the oracle's reading of its own serialization."""

    def __init__(self, ctx, oracle, dset, values):
        self.d, self.values = dset, [np.asarray(v, np.uint32) for v in values]
        self.ref = [oracle.RefBitmap.deserialize(b).to_array() for b in dset.serialize()]
        assert len(self.ref) == len(self.values) == len(dset)
        for v, r in zip(self.values, self.ref):
            assert np.array_equal(v, r)
        self.expectations = (self.values, self.ref)


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    out = {}
    typed = [ZOO, [], SMALL]
    out["typed"] = Case(ctx, oracle, ctx.upload_soa(_typed_soa(typed)), [_values_of(c) for c in typed])
    plain = _plain_bitmaps()
    for ro in (False, True):
        out[f"values-ro{int(ro)}"] = Case(ctx, oracle, ctx.upload_values(plain, run_optimize=ro), plain)
    return out


CASES = ["typed", "values-ro0", "values-ro1"]


def test_container_types_are_what_the_cases_name(cases):
    h = cases["typed"].d.download()
    want = ZOO + SMALL
    assert h.type.tolist() == [t for _, _, t, _ in want] and h.key.tolist() == [k for _, k, _, _ in want]
    assert h.card.tolist() == [len(np.unique(low)) for _, _, _, low in want]
    runs = {n: int(r) for (n, _, _, _), r in zip(want, h.nruns)}
    assert (runs["r_one"], runs["r_whole"], runs["r65"], runs["r130"], runs["r2047"], runs["r3000"]) == \
        (1, 1, 65, 130, 2047, 3000)
    assert h.begin.tolist() == [0, len(ZOO), len(ZOO), len(ZOO) + len(SMALL)]
    # the same values through bitmapOf + runOptimize: 2047 runs of 3 stay a Run (8190 B against 8192 B), the full
    # container is a Bitmap unoptimized and one run optimized, 3000 runs of 2 are no Run
    for ro, exp in ((False, {50: B, 21: B, 51: B, 9: A}), (True, {50: R, 21: R, 51: B, 31: R, 65535: A})):
        h = cases[f"values-ro{int(ro)}"].d.download(0, 1)
        got = dict(zip(h.key.tolist(), h.type.tolist()))
        assert {k: got[k] for k in exp} == exp, ro
    assert set(cases["values-ro1"].d.download().type.tolist()) == {A, B, R}


# ---- expectations
def _value_pool(rng, v):
    """Queries for a bitmap with members v: 0 and 2^32 - 1, both sides of every container's first and last member and
    of every present key's range, present values, absent values inside present keys, values in key gaps, values
    below the first key and above the last."""
    pool = [np.array([0, 1, U32 - 1, U32], np.int64), rng.integers(0, 2**32, 40)]
    if len(v):
        v64 = v.astype(np.int64)
        keys = np.unique(v64 >> 16)
        first = v64[np.searchsorted(v64, keys << 16)]
        last = v64[np.searchsorted(v64, (keys + 1) << 16) - 1]
        pool += [first, last, first - 1, first + 1, last - 1, last + 1, keys << 16, (keys << 16) + 65535,
                 (keys << 16) - 1, (keys + 1) << 16]
        pool += [rng.choice(v64, 200), (rng.choice(keys, 200) << 16) | rng.integers(0, 65536, 200)]
        gaps = np.setdiff1d(np.clip(np.concatenate([keys - 1, keys + 1, [0, 65535]]), 0, 65535), keys)
        if len(gaps):
            pool.append((rng.choice(gaps, 60) << 16) | rng.integers(0, 65536, 60))
    return np.clip(np.concatenate(pool), 0, U32).astype(np.uint32)


def _index_pool(rng, v):
    """Select indices: 0, card - 1, card, card + 5, both sides of every container boundary, far past the end."""
    card = len(v)
    pool = [np.array([0, card, card + 5, 2**40, 2**64 - 1], np.uint64)]
    if card:
        ends = np.cumsum(np.unique(v >> 16, return_counts=True)[1]).astype(np.int64)
        edges = np.concatenate([ends - 2, ends - 1, ends, ends + 1])
        pool += [np.array([card - 1], np.uint64), edges[edges >= 0].astype(np.uint64),
                 rng.integers(0, card, 200).astype(np.uint64)]
    return np.concatenate(pool)


def _mixed(rng, case, pool_fn, n=None):
    """(bitmap column, queries): every bitmap's pool, the empty bitmap's included, shuffled; n given: n of them, with
    duplicates."""
    bs, qs = [], []
    for b, v in enumerate(case.values):
        q = pool_fn(rng, v)
        bs.append(np.full(len(q), b, np.uint32))
        qs.append(q)
    bs, qs = np.concatenate(bs), np.concatenate(qs)
    perm = rng.permutation(len(qs))
    bs, qs = bs[perm], qs[perm]
    if n is not None:
        bs, qs = np.resize(bs, n), np.resize(qs, n)
        if n > 8:
            bs[::7], qs[::7] = bs[0], qs[0]
    return bs, qs


def _check_value_queries(case, bs, qs, tag):
    got_c, got_r = case.d.contains(qs, bitmap=bs), case.d.rank(qs, bitmap=bs)
    assert got_c.dtype == bool and got_r.dtype == np.uint64 and len(got_c) == len(got_r) == len(qs), tag
    for exp in case.expectations:
        want_c, want_r = np.zeros(len(qs), bool), np.zeros(len(qs), np.uint64)
        for b, v in enumerate(exp):
            m = bs == b
            want_c[m] = np.isin(qs[m], v)
            want_r[m] = np.searchsorted(v, qs[m], "right")
        assert np.array_equal(got_c, want_c), tag
        assert np.array_equal(got_r, want_r), tag


def _check_select(case, bs, js, tag):
    got_v, got_f = case.d.select(js, bitmap=bs)
    assert got_v.dtype == np.uint32 and got_f.dtype == bool and len(got_v) == len(got_f) == len(js), tag
    for exp in case.expectations:
        want_v, want_f = np.zeros(len(js), np.uint32), np.zeros(len(js), bool)
        for b, v in enumerate(exp):
            m = (bs == b) & (js < len(v))
            want_f[m] = True
            want_v[m] = v[js[m].astype(np.int64)]
        assert np.array_equal(got_f, want_f), tag
        assert np.array_equal(got_v, want_v), tag


# ---- toArray
@pytest.mark.parametrize("name", CASES)
def test_to_arrays(cases, name):
    case = cases[name]
    nb = len(case.values)
    got = case.d.to_arrays()
    assert len(got) == nb and all(g.dtype == np.uint32 for g in got)
    for exp in case.expectations:
        for b in range(nb):
            assert np.array_equal(got[b], exp[b]), (name, b)
    # first > 0, one bitmap, the empty bitmap alone, an empty range
    for first, count in ((1, nb - 1), (2, 1), (nb - 1, 1), (1, 0), (nb, 0)):
        part = case.d.to_arrays(first, count)
        assert len(part) == count
        for i, g in enumerate(part):
            assert np.array_equal(g, case.values[first + i]), (name, first, count)


@pytest.mark.parametrize("name", CASES)
def test_sizes_only_small_cap_and_device_buffer(ctx, cases, name):
    import torch
    case = cases[name]
    nb = len(case.values)
    lens = np.array([len(v) for v in case.values], np.uint64)
    want_offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(want_offs[-1])
    # dst == NULL: the sizes only, and nothing decoded
    assert np.array_equal(case.d.values_device(0, 0), want_offs)
    assert ctx.stats()["tasks"] == 0
    assert np.array_equal(case.d.values_device(0, 0, first=1, count=2), want_offs[1:4] - want_offs[1])
    # cap too small: RB_EINVAL, the offsets still filled, nothing written (host and device destinations)
    offs = np.zeros(nb + 1, np.uint64)
    host = np.full(total, 0xA5A5A5A5, np.uint32)
    rc = L.lib().rbgpu_set_values(case.d.h, 0, nb, host.ctypes.data, total - 1, offs.ctypes.data_as(L._U64P))
    assert rc == L.RB_EINVAL and np.array_equal(offs, want_offs) and np.all(host == 0xA5A5A5A5)
    buf = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(rb.InvalidArgument):
        case.d.values_device(buf.data_ptr(), total - 1)
    torch.cuda.synchronize()
    assert bool((buf == -1).all())
    # into a torch buffer: the host call's values, and nothing past them
    offs = case.d.values_device(buf.data_ptr(), total)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert np.array_equal(offs, want_offs)
    assert np.array_equal(got[:total], np.concatenate(case.d.to_arrays()))
    assert np.array_equal(got[:total], np.concatenate(case.values)) and np.all(got[total:] == U32)
    # a sub-range lands at the start of the buffer
    buf.fill_(-1)
    offs = case.d.values_device(buf.data_ptr(), total, first=3, count=nb - 3)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    k = int(offs[-1])
    assert k == total - int(want_offs[3]) and np.array_equal(got[:k], _cat(case.values[3:]))
    assert np.all(got[k:] == U32)


def test_values_stats(ctx, cases):
    for name in CASES:
        case = cases[name]
        for first, count in ((0, len(case.values)), (1, 2), (2, 1)):
            h = case.d.download(first, count)
            got = case.d.to_arrays(first, count)
            st = ctx.stats()
            total = sum(len(g) for g in got)
            if h.n_containers == 0:  # the empty bitmap alone: nothing launched
                assert st["tasks"] == 0 and st["n_kernels"] == 0, (name, st)
                continue
            pay = sum(len(h.container_payload(i)) for i in range(h.n_containers))
            assert st["main_kernel"] == "k_set_values" and st["tasks"] == h.n_containers, (name, st)
            assert st["output_bytes"] == 4 * total and st["result_cardinality"] == total, (name, st)
            assert st["input_bytes"] == pay + 16 * h.n_containers, (name, st)
            assert st["main_kernel_bytes"] == st["input_bytes"] + st["output_bytes"], (name, st)


# ---- contains / rank / select
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("name", CASES)
def test_query_batches(ctx, cases, name, n):
    case = cases[name]
    rng = _rng(100 + n)
    bs, qs = _mixed(rng, case, _value_pool, n)
    _check_value_queries(case, bs, qs, (name, n))
    assert ctx.stats()["tasks"] == n and (n == 0 or ctx.stats()["main_kernel"] == "k_set_rank")
    bs, js = _mixed(rng, case, _index_pool, n)
    _check_select(case, bs, js, (name, n))
    assert ctx.stats()["tasks"] == n and (n == 0 or ctx.stats()["main_kernel"] == "k_set_select")
    case.d.contains(qs, bitmap=bs)
    assert ctx.stats()["tasks"] == n and (n == 0 or ctx.stats()["main_kernel"] == "k_set_contains")
    if n:  # bitmap == NULL: bitmap 0 for all
        zero = np.zeros(n, np.uint32)
        assert np.array_equal(case.d.rank(qs), case.d.rank(qs, bitmap=zero))
        assert np.array_equal(case.d.contains(qs), np.isin(qs, case.values[0]))
        v, f = case.d.select(js)
        assert np.array_equal(f, js < len(case.values[0]))


@pytest.mark.parametrize("name", CASES)
def test_every_boundary(cases, name):
    """The whole pools of every bitmap in one call each: both sides of every container boundary are asked."""
    case = cases[name]
    rng = _rng(7)
    bs, qs = _mixed(rng, case, _value_pool)
    _check_value_queries(case, bs, qs, name)
    bs, js = _mixed(rng, case, _index_pool)
    _check_select(case, bs, js, name)
    # select(rank(x) - 1) == x for members, per bitmap
    for b, v in enumerate(case.values):
        if len(v):
            x = rng.choice(v, 300)
            col = np.full(len(x), b, np.uint32)
            got, found = case.d.select(case.d.rank(x, bitmap=col) - np.uint64(1), bitmap=col)
            assert found.all() and np.array_equal(got, x), (name, b)


def test_bad_arguments_are_refused(cases):
    d = cases["typed"].d
    nb = len(d)
    q = np.array([1, 2, 3], np.uint32)
    for fn, arg in ((d.contains, q), (d.rank, q), (d.select, q.astype(np.uint64))):
        with pytest.raises(rb.InvalidArgument):
            fn(arg, bitmap=np.array([0, nb, 0], np.uint32))
        with pytest.raises(rb.InvalidArgument):
            fn(arg, bitmap=np.array([0, 0, U32], np.uint32))
    for first, count in ((0, nb + 1), (nb, 1), (nb + 1, 0), (U32, 2)):
        with pytest.raises(rb.InvalidArgument):
            d.to_arrays(first, count)
        with pytest.raises(rb.InvalidArgument):
            d.values_device(0, 0, first, count)
    lib = L.lib()
    out8, out64, out32 = np.zeros(3, np.uint8), np.zeros(3, np.uint64), np.zeros(3, np.uint32)
    j = q.astype(np.uint64)
    assert lib.rbgpu_set_contains(d.h, None, None, 3, out8.ctypes.data) == L.RB_EINVAL
    assert lib.rbgpu_set_contains(d.h, None, q.ctypes.data, 3, None) == L.RB_EINVAL
    assert lib.rbgpu_set_rank(d.h, None, None, 3, out64.ctypes.data) == L.RB_EINVAL
    assert lib.rbgpu_set_rank(d.h, None, q.ctypes.data, 3, None) == L.RB_EINVAL
    assert lib.rbgpu_set_select(d.h, None, None, 3, out32.ctypes.data, out8.ctypes.data) == L.RB_EINVAL
    assert lib.rbgpu_set_select(d.h, None, j.ctypes.data, 3, None, out8.ctypes.data) == L.RB_EINVAL
    assert lib.rbgpu_set_select(d.h, None, j.ctypes.data, 3, out32.ctypes.data, None) == L.RB_EINVAL
    assert lib.rbgpu_set_values(d.h, 0, nb, None, 0, None) == L.RB_EINVAL
    # n == 0 with null arrays is legal
    assert lib.rbgpu_set_contains(d.h, None, None, 0, None) == L.RB_OK
    assert lib.rbgpu_set_select(d.h, None, None, 0, None, None) == L.RB_OK


# ---- results of the algebra fed straight in (their arenas carry slot padding)
def _check_result(ctx, oracle, dset, want, tag):
    case = Case(ctx, oracle, dset, want)
    got = dset.to_arrays()
    for b, v in enumerate(want):
        assert np.array_equal(got[b], v), (tag, b)
    rng = _rng(3)
    bs, qs = _mixed(rng, case, _value_pool)
    _check_value_queries(case, bs, qs, tag)
    bs, js = _mixed(rng, case, _index_pool)
    _check_select(case, bs, js, tag)


def test_pairwise_and_wide_results(ctx, oracle, cases):
    case = cases["values-ro1"]
    v = case.values
    idx_a = np.array([0, 0, 3, 4, 2, 1], np.uint32)
    idx_b = np.array([3, 4, 4, 0, 0, 5], np.uint32)
    out = ctx.pairwise(rb.AND, case.d, case.d, idx_a, idx_b)
    _check_result(ctx, oracle, out, [np.intersect1d(v[a], v[b]) for a, b in zip(idx_a, idx_b)], "pairwise and")
    plain = cases["values-ro0"]
    out = ctx.pairwise(rb.XOR, plain.d, plain.d, np.array([0, 4], np.uint32), np.array([3, 2], np.uint32))
    _check_result(ctx, oracle, out, [np.setxor1d(v[0], v[3]), v[4]], "pairwise xor")
    out = ctx.wide(rb.FAST_OR, case.d)
    union = np.unique(np.concatenate(v))
    _check_result(ctx, oracle, out, [union], "wide or")


def test_async_result_is_waited_for(ctx, cases):
    case = cases["values-ro0"]
    n = 5000  # past the small-batch path, so the result is pending when the read-out starts
    idx_a = np.resize(np.array([0, 4, 1, 2, 5], np.uint32), n)
    idx_b = np.resize(np.array([4, 0, 1, 3, 5], np.uint32), n)
    out = ctx.pairwise_async(rb.AND, case.d, case.d, idx_a, idx_b)
    got = out.to_arrays()
    memo = {}
    for i in range(0, n, 97):
        key = (int(idx_a[i]), int(idx_b[i]))
        if key not in memo:
            memo[key] = np.intersect1d(case.values[key[0]], case.values[key[1]])
        assert np.array_equal(got[i], memo[key]), i


# ---- real data
def test_census1881_in_one_call(ctx, oracle):
    from datasets import load_realdata
    bms = [np.unique(b) for b in load_realdata("census1881")]
    d = ctx.upload_values(bms, run_optimize=True)
    got = d.to_arrays()
    assert ctx.stats()["tasks"] == d.n_containers
    refs = [oracle.RefBitmap.deserialize(b).to_array() for b in d.serialize()]
    for b, v in enumerate(bms):
        assert np.array_equal(got[b], v) and np.array_equal(refs[b], v), b
    rng = _rng(1881)
    col = rng.integers(0, len(bms), 4000).astype(np.uint32)
    col = col[np.array([len(bms[b]) > 0 for b in col])]
    x = np.array([rng.choice(bms[b]) for b in col], np.uint32)
    r = d.rank(x, bitmap=col)
    assert np.array_equal(r, np.array([np.searchsorted(bms[b], xi, "right") for b, xi in zip(col, x)], np.uint64))
    back, found = d.select(r - np.uint64(1), bitmap=col)
    assert found.all() and np.array_equal(back, x)
    assert d.contains(x, bitmap=col).all()


# ---- the Python mirror
def test_roaring_bitmap_mirror(oracle):
    v = np.unique(np.concatenate([_values_of(SMALL), np.array([0, 70000, 70001, U32], np.uint32),
                                  np.arange(20 << 16, (22 << 16) + 17, dtype=np.uint32)]))
    x = rb.RoaringBitmap.bitmapOf(v)
    x.runOptimize()
    ref = oracle.RefBitmap.deserialize(x.serialize()).to_array()
    for exp in (v, ref):
        assert np.array_equal(x.toArray(), exp)
        assert x.contains(70000) is True and x.contains(69999) is False and x.contains(-1) is True
        q = np.array([0, 5, 6, 70001, U32, 12345678, 70000, 70000], np.uint32)
        assert np.array_equal(x.contains(q), np.isin(q, exp))
        assert np.array_equal(x.rankLong(q), np.searchsorted(exp, q, "right").astype(np.uint64))
        assert x.rank(70000) == x.rankLong(70000) == int(np.searchsorted(exp, 70000, "right"))
        assert x.rank(-1) == len(exp)
        assert x.select(0) == int(exp[0]) and x.select(len(exp) - 1) == int(exp[-1])
        j = np.array([3, 0, len(exp) - 1, 3], np.uint64)
        assert np.array_equal(x.select(j), exp[j.astype(np.int64)])
        assert x.first() == int(exp[0]) and x.last() == int(exp[-1])
        # ranges that start or end inside, between and past containers; start == 0; start >= end; past 2^32
        e64 = exp.astype(np.int64)
        for s, e in ((0, 1), (0, 2**32), (0, 2**33), (1, 2**32), (5, 6), (6, 10), (2 << 16, 3 << 16), (3 << 16, 9 << 16),
                     ((9 << 16) + 150, (10 << 16) + 40000), ((2 << 16) + 9, (21 << 16) + 5), (70001, 70001),
                     (70002, 70001), (11 << 16, 20 << 16), ((22 << 16) + 16, 2**32 - 1), (2**32 - 1, 2**32),
                     (2**32, 2**32 + 5), (1 << 40, 5), (65536, 65537), ((10 << 16) + 65535, 11 << 16)):
            want = int(np.count_nonzero((e64 >= s) & (e64 < e))) if s < e else 0
            assert x.rangeCardinality(s, e) == want, (s, e)
    with pytest.raises(ValueError):
        x.select(len(v))
    with pytest.raises(ValueError):
        x.select(np.array([0, len(v) + 5], np.uint64))
    empty = rb.RoaringBitmap()
    assert len(empty.toArray()) == 0 and empty.contains(0) is False and empty.rank(U32) == 0
    assert empty.rangeCardinality(0, 2**32) == 0
    for fn in (empty.first, empty.last, lambda: empty.select(0)):
        with pytest.raises(ValueError):
            fn()
