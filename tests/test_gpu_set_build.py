"""Sets built from member values on the MI355X: rbgpu_set_from_values / rbgpu_set_from_values_device, Context.build_values
/ build_values_device and the RoaringBitmapWriter mirror.  Every comparison is exact, and every case has three
expectations: the serialized bytes equal oracle.RefBitmap.of(v).serialize() (after run_optimize() when the flag is set),
they equal the bytes of ctx.upload_values(..., run_optimize) — the host-built containers — and the downloaded
(key, type, cardinality, run count) of every container equals the oracle's, with the types the case is about asserted
by name as well."""
import ctypes as C

import numpy as np
import pytest

import roaringbitmap_amd as rb
from roaringbitmap_amd import _lib as L
from type_boundary_cases import target_set

pytestmark = pytest.mark.gpu

A, B, R = rb.ARRAY, rb.BITMAP, rb.RUN
U32 = 2**32 - 1
TILE = L.BUILD_TILE


def _rng(seed):
    return np.random.default_rng(seed)


def _pick(seed, n):
    return np.sort(_rng(seed).choice(65536, size=n, replace=False)).astype(np.uint32)


def _at(key, low):
    return (np.asarray(low, np.uint32) | np.uint32(key << 16)).astype(np.uint32)


def _payload_bytes(t, c, r):
    return 8192 if t == B else 2 * c if t == A else 4 * r


def check(ctx, oracle, bitmaps, ro, built=None):
    """The three expectations for one batch; returns (the built set, its downloaded SoA)."""
    bitmaps = [np.asarray(v, np.uint32) for v in bitmaps]
    if built is None:
        built = ctx.build_values(bitmaps, run_optimize=ro)
    assert len(built) == len(bitmaps)
    got = built.serialize()
    host = ctx.upload_values(bitmaps, run_optimize=ro).serialize()
    conts, begin = [], [0]
    for i, v in enumerate(bitmaps):
        ref = oracle.RefBitmap.of(v)
        if ro:
            ref.run_optimize()
        assert got[i] == ref.serialize(), (i, ro)
        assert got[i] == host[i], (i, ro)
        conts += ref.containers()
        begin.append(len(conts))
    h = built.download()
    assert list(zip(h.key.tolist(), h.type.tolist(), h.card.tolist(), h.nruns.tolist())) == conts
    assert h.begin.tolist() == begin
    # the arena is tight: the payloads, each rounded up to 16 B, and nothing else
    sizes = [_payload_bytes(t, c, r) for _, t, c, r in conts]
    assert built.payload_capacity == sum((b + 15) & ~15 for b in sizes)
    return built, h


# ---- the zoo: one bitmap, containers of 1 .. 65536 members, keys 0 and 65535, values 0 and 2^32 - 1
ZOO_CARDS = [(0, 1), (2, 63), (3, 64), (4, 65), (7, 4095), (8, 4096), (9, 4097), (20, 65535), (21, 65536), (65535, 1)]


def _zoo():
    parts = []
    for key, n in ZOO_CARDS:
        low = np.array([0]) if key == 0 else np.array([65535]) if key == 65535 else \
            np.arange(65536) if n == 65536 else np.arange(1, 65536) if n == 65535 else _pick(key, n)
        parts.append(_at(key, low))
    return np.concatenate(parts)


@pytest.mark.parametrize("ro", [False, True])
def test_zoo(ctx, oracle, ro):
    v = _zoo()
    assert v[0] == 0 and v[-1] == U32
    built, h = check(ctx, oracle, [v], ro)
    types = dict(zip(h.key.tolist(), h.type.tolist()))
    if not ro:  # bitmapOf: an Array up to 4096 members, a Bitmap above, never a Run
        assert [types[k] for k, _ in ZOO_CARDS] == [A, A, A, A, A, A, B, B, B, A]
    else:       # the two long runs become Runs; scattered values stay as they are
        assert [types[k] for k, _ in ZOO_CARDS] == [A, A, A, A, A, A, B, R, R, A]
    s = ctx.stats()
    nc = built.n_containers
    assert s["main_kernel"] == "k_set_build" and s["tasks"] == nc == s["result_containers"] == len(ZOO_CARDS)
    assert s["result_cardinality"] == len(v) and s["input_bytes"] == 4 * len(v)
    sizes = [_payload_bytes(t, c, r) for t, c, r in zip(h.type.tolist(), h.card.tolist(), h.nruns.tolist())]
    assert s["output_bytes"] == sum(sizes) + 16 * nc


# ---- run-optimize boundaries, each on both sides (type_runopt: Array -> Run iff 2c > 2 + 4r, Bitmap -> Run iff
# 8192 > 2 + 4r)
RUNOPT_EDGES = [((15, 7), A), ((15, 6), R), ((4095, 2047), A), ((4095, 2046), R),
                ((4097, 2047), R), ((4097, 2048), B), ((20000, 2047), R), ((20000, 2048), B)]


def test_run_optimize_boundaries(ctx, oracle):
    assert all(2 * c == 2 + 4 * r for c, r in ((15, 7), (4095, 2047)))  # the ties: an Array stays an Array
    v = np.concatenate([_at(k, target_set(c, r)) for k, ((c, r), _) in enumerate(RUNOPT_EDGES)])
    _, h = check(ctx, oracle, [v], True)
    assert h.type.tolist() == [t for _, t in RUNOPT_EDGES]
    assert h.nruns.tolist() == [r if t == R else 0 for (_, r), t in RUNOPT_EDGES]
    _, h = check(ctx, oracle, [v], False)
    assert h.type.tolist() == [A if c <= 4096 else B for (c, _), _ in RUNOPT_EDGES]


# ---- batches
def _heads(bitmaps):
    """Positions, in the grouped element stream, at which a container starts (duplicates stay in the stream)."""
    out, pos = [], 0
    for v in bitmaps:
        hi = np.sort(np.asarray(v, np.uint32)) >> 16
        if len(hi):
            out.append(pos + np.concatenate([[0], np.nonzero(np.diff(hi.astype(np.int64)))[0] + 1]))
        pos += len(hi)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


@pytest.mark.parametrize("ro", [False, True])
def test_batch_of_1000_lengths(ctx, oracle, ro):
    """Bitmap i holds i values (with repeats) over eight high keys: its start and its key changes fall anywhere in a
    discovery tile, and over the batch on every residue of it."""
    rng = _rng(1000)
    bitmaps = [((rng.integers(0, 8, i) << 16) | rng.integers(0, 300, i)).astype(np.uint32) for i in range(1000)]
    assert set((_heads(bitmaps) % TILE).tolist()) == set(range(TILE))
    assert sum(len(b) for b in bitmaps) > 400 * TILE
    check(ctx, oracle, bitmaps, ro)


def test_bitmap_starts_on_every_tile_residue(ctx, oracle):
    """Empty bitmaps first, in the middle and last; between them 1100 one-value bitmaps and two longer ones, so a
    bitmap starts at every residue of the discovery tile."""
    e = np.zeros(0, np.uint32)
    ones = [np.array([(i * 2654435761) & U32], np.uint32) for i in range(1100)]
    bitmaps = [e, e] + ones[:500] + [e, np.arange(70000, 73000, dtype=np.uint32), e, e] + ones[500:] + \
        [np.array([5, 5, 5], np.uint32), e, e, e]
    offs = np.cumsum([0] + [len(b) for b in bitmaps])[:-1]
    starts = {int(o) % TILE for o, b in zip(offs, bitmaps) if len(b)}
    assert starts == set(range(TILE))
    check(ctx, oracle, bitmaps, True)


def test_empty_batches(ctx, oracle):
    e = np.zeros(0, np.uint32)
    built, h = check(ctx, oracle, [e, e, e], False)
    assert built.n_containers == 0 and ctx.stats()["tasks"] == 0
    none = ctx.build_values([])
    assert len(none) == 0 and none.n_containers == 0 and none.serialize() == []


# ---- unsorted input and duplicates
def _spread(seed, keys, n):
    rng = _rng(seed)
    return ((rng.choice(keys, n).astype(np.uint32) << 16) | rng.integers(0, 65536, n).astype(np.uint32)).astype(np.uint32)


UNSORTED = {
    "shuffled-doubled": lambda: _rng(1).permutation(np.repeat(_spread(2, [0, 1, 5, 900, 65535], 60000), 2)),
    "descending": lambda: np.sort(_spread(3, [0, 3, 4, 65535], 40000))[::-1].copy(),
    "keys-ascending-lows-shuffled": lambda: np.concatenate(
        [_at(k, _rng(k).permutation(_pick(40 + k, n))) for k, n in ((1, 100), (2, 5000), (9, 30000), (65535, 4097))]),
    "70000-over-5000": lambda: _at(77, _rng(4).choice(_pick(5, 5000), 70000)),
    "200000-copies": lambda: np.full(200000, (123 << 16) | 4567, np.uint32),
}


@pytest.mark.parametrize("name", list(UNSORTED))
@pytest.mark.parametrize("ro", [False, True])
def test_unsorted_and_duplicates(ctx, oracle, name, ro):
    v = UNSORTED[name]().astype(np.uint32)
    built, h = check(ctx, oracle, [v], ro)
    assert ctx is built.ctx
    if name == "70000-over-5000":
        assert h.card.tolist() == [len(np.unique(v))] and h.card[0] <= 5000 and h.type.tolist() == [B if h.card[0] > 4096 else A]
    if name == "200000-copies":
        assert (h.type.tolist(), h.card.tolist()) == ([A], [1])


def test_unsorted_batch_keeps_bitmaps_apart(ctx, oracle):
    """Several unsorted bitmaps that share values: the sort key carries the bitmap index."""
    base = _spread(6, [0, 1, 2], 30000)
    bitmaps = [_rng(i).permutation(base[i * 3000:(i + 4) * 3000]) for i in range(8)] + [np.zeros(0, np.uint32)]
    check(ctx, oracle, bitmaps, True)


# ---- the device form
def _to_gpu(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, np.uint32).view(np.int32).copy()).to("cuda:0")


@pytest.mark.parametrize("ro", [False, True])
def test_device_form_gives_the_same_bytes_and_leaves_the_input(ctx, oracle, ro):
    import torch
    bitmaps = [UNSORTED["shuffled-doubled"]().astype(np.uint32), np.zeros(0, np.uint32), _zoo()]
    offs = np.cumsum([0] + [len(b) for b in bitmaps]).astype(np.uint64)
    t = _to_gpu(np.concatenate(bitmaps))
    before = t.clone()
    torch.cuda.synchronize()
    built = ctx.build_values_device(t.data_ptr(), offs, run_optimize=ro)
    check(ctx, oracle, bitmaps, ro, built=built)
    assert torch.equal(t, before)
    # a range that does not start at the tensor's first element
    part = ctx.build_values_device(t.data_ptr(), offs[2:], run_optimize=ro)
    check(ctx, oracle, bitmaps[2:], ro, built=part)


def test_values_device_round_trip_of_the_typed_zoo(ctx):
    """values_device -> build_values_device gives back the members of every container type."""
    import torch
    from test_gpu_set_values import SMALL, ZOO, _typed_soa
    d = ctx.upload_soa(_typed_soa([ZOO, [], SMALL]))
    want = d.to_arrays()
    total = sum(len(v) for v in want)
    t = torch.zeros(total, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    offs = d.values_device(t.data_ptr(), total)
    for ro in (False, True):
        back = ctx.build_values_device(t.data_ptr(), offs, run_optimize=ro)
        got = back.to_arrays()
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- a built set is a set like any other
def test_built_set_in_pairwise_and(ctx, oracle):
    a = [_spread(10 + i, [0, 1, 2, 7], 50000) for i in range(4)]
    b = [np.unique(_spread(20 + i, [0, 1, 2, 9], 50000)) for i in range(4)]
    built = ctx.build_values(a, run_optimize=True)
    up = ctx.upload_values(b, run_optimize=True)
    got = ctx.pairwise(rb.AND, built, up).serialize()
    for i in range(4):
        ra, rb_ = oracle.RefBitmap.of(a[i]), oracle.RefBitmap.of(b[i])
        ra.run_optimize(), rb_.run_optimize()
        assert got[i] == oracle.op(rb.AND, ra, rb_).serialize()


def test_writer_mirror(ctx, oracle):
    for rc in (False, True):
        w = rb.RoaringBitmapWriter.writer().runCompress(rc).get()
        v = np.concatenate([np.arange(5 << 16, (5 << 16) + 40000), _at(9, _pick(1, 300))]).astype(np.uint32)
        w.add(7)
        w.addMany(v)
        w.add(U32)
        w.flush()
        ref = oracle.RefBitmap.of(np.concatenate([[7], v, [U32]]).astype(np.uint32))
        if rc:
            ref.run_optimize()
        assert w.get().serialize() == ref.serialize()
        w.reset()
        w.addMany(3, 2, 1, 2)
        assert w.get().toArray().tolist() == [1, 2, 3]


# ---- RB_EINVAL, before any launch
def _raw(fn, ctx, ptr, offs, n, flags, out):
    offs = np.ascontiguousarray(offs, np.uint64)
    return fn(ctx.h, C.c_void_p(ptr or None), offs.ctypes.data_as(L._U64P) if len(offs) else None, n, flags, out)


@pytest.mark.parametrize("form", ["rbgpu_set_from_values", "rbgpu_set_from_values_device"])
def test_bad_arguments(ctx, form):
    fn = getattr(L.lib(), form)
    vals = np.arange(10, dtype=np.uint32)
    ptr = _to_gpu(vals).data_ptr() if form.endswith("device") else vals.ctypes.data
    out = C.c_void_p()
    assert _raw(fn, ctx, ptr, [0, 6, 4, 10], 3, 0, C.byref(out)) == L.RB_EINVAL       # offsets descend
    assert _raw(fn, ctx, 0, [0, 5], 1, 0, C.byref(out)) == L.RB_EINVAL                # null values, 5 to read
    assert _raw(fn, ctx, ptr, [0, 5], 1, 0, None) == L.RB_EINVAL                      # null out
    assert _raw(fn, ctx, ptr, [0, 5], 1, 2, C.byref(out)) == L.RB_EINVAL              # unknown flag bit
    assert _raw(fn, ctx, ptr, [], 1, 0, C.byref(out)) == L.RB_EINVAL                  # null offsets, one bitmap
    assert not out.value
    with pytest.raises(rb.InvalidArgument):
        ctx.build_values_device(0, [0, 3])
    # legal: null values with nothing to read
    assert _raw(fn, ctx, 0, [0, 0, 0], 2, 1, C.byref(out)) == L.RB_OK
    d = rb.DeviceSet(ctx, out.value)
    assert len(d) == 2 and d.n_containers == 0
