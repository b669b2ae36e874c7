"""Reference restatement of the range mutations (a helper, not a test): RoaringBitmap.add / remove / flip over
[rangeStart, rangeEnd), static and in place, and bitmapOfRange, with the container classes' add / remove / not under
them.  Paths are relative to /root/reference/RoaringBitmap/src/main/java/org/roaringbitmap/.

A bitmap is a list of (key, type, values): `values` the sorted low 16-bit members of one container as a uint32 array,
`type` the container class that holds them.  The bitmap-level loops below follow the reference's line by line; each
container method decides its result TYPE the way its class does (ArrayContainer counts the new cardinality from two
binary searches and converts above DEFAULT_MAX_SIZE, BitmapContainer.add never converts, RunContainer.add / remove stay
RunContainers, RunContainer.not ends in toEfficientContainer) — not "the smallest encoding of the result set", which is
a different table (a full Bitmap stays a Bitmap, a Run of 3000 runs stays a Run).  A RunContainer's run list is kept
maximal by iadd / iremove (RunContainer.java:1087-1130: valueLengthContains(begin - 1, ..), canPrependValueLength,
mergeValuesLength) and by smartAppendExclusive, so a Run result is its value set re-encoded.  Bytes come out of the
oracle's serializer (to_oracle -> rbref.from_soa)."""
import numpy as np

ARRAY, BITMAP, RUN = 0, 1, 2
ADD, REMOVE, FLIP = 0, 1, 2
MAX_ARRAY = 4096  # ArrayContainer.DEFAULT_MAX_SIZE (ArrayContainer.java:27)
FULL = np.arange(65536, dtype=np.uint32)
FULL.setflags(write=False)
NONE = np.zeros(0, np.uint32)


def n_runs(vals) -> int:
    v = np.asarray(vals, dtype=np.int64)
    return 0 if len(v) == 0 else 1 + int(np.count_nonzero(np.diff(v) != 1))


def _span(b: int, e: int) -> np.ndarray:
    return FULL if (b, e) == (0, 65536) else np.arange(b, e, dtype=np.uint32)


def _bits(vals) -> np.ndarray:
    x = np.zeros(65536, bool)
    x[np.asarray(vals, dtype=np.int64)] = True
    return x


def _vals(bits) -> np.ndarray:
    return np.nonzero(bits)[0].astype(np.uint32)


# ------------------------------------------------------------------------------------------- Container.java
def range_of_ones(b: int, e: int):
    """Container.rangeOfOnes (Container.java:29-37): arrayContainerOverRunThreshold = 2."""
    return (ARRAY if e - b <= 2 else RUN), _span(b, e)


# ------------------------------------------------------------------------------------------- ArrayContainer.java
def _array_indices(v, b, e):
    """indexstart / indexend of add, iadd, remove, iremove (ArrayContainer.java:111-120): the first index with a
    value >= begin and the first with a value > end - 1."""
    return int(np.searchsorted(v, b, "left")), int(np.searchsorted(v, e - 1, "right"))


def array_add(v, b, e):
    """ArrayContainer.add / iadd(begin, end) (:103-135, :464-): the same decisions in both."""
    if b == e:
        return ARRAY, v                                   # :104-106 clone / :466-468 this
    i0, i1 = _array_indices(v, b, e)
    newcard = i0 + (len(v) - i1) + (e - b)                # :121-122
    if newcard > MAX_ARRAY:                               # :123-126 toBitmapContainer().iadd: stays a Bitmap
        return bitmap_add(v, b, e)
    return ARRAY, np.concatenate([v[:i0], _span(b, e), v[i1:]]).astype(np.uint32)


def array_remove(v, b, e):
    """ArrayContainer.remove / iremove(begin, end) (:1039-1062, :759-): always an ArrayContainer."""
    if b == e:
        return ARRAY, v
    i0, i1 = _array_indices(v, b, e)
    return ARRAY, np.concatenate([v[:i0], v[i1:]]).astype(np.uint32)


def array_not(v, b, e):
    """ArrayContainer.not / inot(firstOfRange, lastOfRange) (:876-929, :652-694)."""
    if b >= e:
        return ARRAY, v                                   # :878-880
    i0, i1 = _array_indices(v, b, e)                      # startIndex, lastIndex + 1
    in_range = i1 - i0                                    # currentValuesInRange (:892)
    new_in_range = (e - b) - in_range                     # :893-894
    newcard = len(v) + new_in_range - in_range            # :895-896
    if newcard > MAX_ARRAY:                               # :898-900 toBitmapContainer().not(...)
        return bitmap_not(v, b, e)
    flipped = np.setdiff1d(_span(b, e), v[i0:i1], assume_unique=True)
    return ARRAY, np.concatenate([v[:i0], flipped, v[i1:]]).astype(np.uint32)


# ------------------------------------------------------------------------------------------- BitmapContainer.java
def bitmap_add(v, b, e):
    """BitmapContainer.add / iadd(begin, end) (:131-144, :517-529): setBitmapRange and updateCardinality, no
    conversion — a full container is a BitmapContainer of 65536 values."""
    x = _bits(v)
    x[b:e] = True
    return BITMAP, (FULL if x.all() else _vals(x))


def bitmap_remove(v, b, e):
    """BitmapContainer.remove / iremove(begin, end) (:1175-1190, :797-811): toArrayContainer at <= 4096."""
    if b == e:
        return BITMAP, v                                  # :1176-1178 clone
    x = _bits(v)
    x[b:e] = False
    out = _vals(x)
    return (ARRAY if len(out) <= MAX_ARRAY else BITMAP), out


def bitmap_not(v, b, e):
    """BitmapContainer.not -> clone().inot (:1003-1006, :688-696): toArrayContainer at <= 4096, else this."""
    x = _bits(v)
    x[b:e] ^= True
    out = FULL if x.all() else _vals(x)
    return (ARRAY if len(out) <= MAX_ARRAY else BITMAP), out


# ------------------------------------------------------------------------------------------- RunContainer.java
def to_efficient(vals):
    """RunContainer.toEfficientContainer (:2326-2335): this while serializedSizeInBytes(nbrruns) = 2 + 4 r is at
    most min(8192, 2 + 2 card); else toBitmapOrArrayContainer(card) (:2300-2323)."""
    c, r = len(vals), n_runs(vals)
    if 2 + 4 * r <= min(8192, 2 + 2 * c):
        return RUN, vals
    return (ARRAY if c <= MAX_ARRAY else BITMAP), vals


def run_add(v, b, e):
    """RunContainer.add -> clone().iadd (:242-245, :1068-): every branch returns this, the RunContainer, with
    [begin, end) merged into the run list (a span of one through add(char), :1078-1081, :248-)."""
    if b == e:
        return RUN, v
    x = _bits(v)
    x[b:e] = True
    return RUN, (FULL if x.all() else _vals(x))


def run_remove(v, b, e):
    """RunContainer.remove -> clone().iremove (:2032-2035, :1553-): returns this (a span of one calls remove(char)
    and drops the container IT returns, :1562-1565); the list may end with no runs."""
    if b == e:
        return RUN, v
    x = _bits(v)
    x[b:e] = False
    return RUN, _vals(x)


def run_not(v, b, e):
    """RunContainer.not / inot (:1900-1918, :1267-1364): the runs below rangeStart, then smartAppendExclusive of
    the range and of every later run, then toEfficientContainer; inot's in-place branch ends the same way."""
    if e <= b:
        return RUN, v                                     # :1901-1903
    x = _bits(v)
    x[b:e] ^= True
    return to_efficient(FULL if x.all() else _vals(x))


_CONTAINER_OPS = {
    (ARRAY, ADD): array_add, (ARRAY, REMOVE): array_remove, (ARRAY, FLIP): array_not,
    (BITMAP, ADD): bitmap_add, (BITMAP, REMOVE): bitmap_remove, (BITMAP, FLIP): bitmap_not,
    (RUN, ADD): run_add, (RUN, REMOVE): run_remove, (RUN, FLIP): run_not,
}


def container_op(op: int, t: int, v, b: int, e: int):
    """Container.add / remove / not(b, e) of a container of class t -> (type, values); values may be empty."""
    assert 0 <= b <= e <= 65536
    return _CONTAINER_OPS[(t, op)](np.asarray(v, dtype=np.uint32), b, e)


# ------------------------------------------------------------------------------------------- RoaringBitmap.java
def range_sanity_check(start: int, end: int) -> None:
    """rangeSanityCheck (:204-213)."""
    if start < 0 or start > (1 << 32) - 1:
        raise ValueError(f"rangeStart={start} should be in [0, 0xffffffff]")
    if end > (1 << 32) or end < 0:
        raise ValueError(f"rangeEnd={end} should be in [0, 0xffffffff + 1]")


def _split(start, end):
    return start >> 16, start & 0xFFFF, (end - 1) >> 16, (end - 1) & 0xFFFF


def _index(conts):
    return {k: i for i, (k, _, _) in enumerate(conts)}


def static_add(conts, start, end):
    """RoaringBitmap.add(rb, rangeStart, rangeEnd) (:298-344)."""
    range_sanity_check(start, end)
    if start >= end:
        return list(conts)                                                      # :300-302
    hb_s, lb_s, hb_l, lb_l = _split(start, end)
    at = _index(conts)
    out = [c for c in conts if c[0] < hb_s]                                     # :311 appendCopiesUntil
    if hb_s == hb_l:                                                            # :313-321
        i = at.get(hb_s)
        t, v = container_op(ADD, conts[i][1], conts[i][2], lb_s, lb_l + 1) if i is not None \
            else range_of_ones(lb_s, lb_l + 1)
        out.append((hb_s, t, v))
    else:
        i, j = at.get(hb_s), at.get(hb_l)
        t, v = container_op(ADD, conts[i][1], conts[i][2], lb_s, 65536) if i is not None \
            else range_of_ones(lb_s, 65536)                                     # :325-331
        out.append((hb_s, t, v))
        for hb in range(hb_s + 1, hb_l):                                        # :332-335 whatever rb held there
            out.append((hb,) + range_of_ones(0, 65536))
        t, v = container_op(ADD, conts[j][1], conts[j][2], 0, lb_l + 1) if j is not None \
            else range_of_ones(0, lb_l + 1)                                     # :336-341
        out.append((hb_l, t, v))
    return out + [c for c in conts if c[0] > hb_l]                              # appendCopiesAfter


def static_remove(conts, start, end):
    """RoaringBitmap.remove(rb, rangeStart, rangeEnd) (:995-1037)."""
    range_sanity_check(start, end)
    if start >= end:
        return list(conts)
    hb_s, lb_s, hb_l, lb_l = _split(start, end)
    at = _index(conts)
    out = [c for c in conts if c[0] < hb_s]

    def removed(i, b, e):
        t, v = container_op(REMOVE, conts[i][1], conts[i][2], b, e)
        if len(v):                                                              # !c.isEmpty()
            out.append((conts[i][0], t, v))
    if hb_s == hb_l:                                                            # :1009-1019
        if hb_s in at:
            removed(at[hb_s], lb_s, lb_l + 1)
    else:
        if hb_s in at and lb_s != 0:                                            # :1022-1028
            removed(at[hb_s], lb_s, 65536)
        if hb_l in at and lb_l != 0xFFFF:                                       # :1029-1034
            removed(at[hb_l], 0, lb_l + 1)
    return out + [c for c in conts if c[0] > hb_l]


def static_flip(conts, start, end):
    """RoaringBitmap.flip(bm, rangeStart, rangeEnd) (:626-664); x.flip(rangeStart, rangeEnd) (:1893-1925) walks the
    same keys with inot and removeAtIndex / insertNewKeyValueAt: the same containers."""
    range_sanity_check(start, end)
    if start >= end:
        return list(conts)
    hb_s, lb_s, hb_l, lb_l = _split(start, end)
    at = _index(conts)
    out = [c for c in conts if c[0] < hb_s]
    for hb in range(hb_s, hb_l + 1):                                            # :640-660
        b = lb_s if hb == hb_s else 0
        e = (lb_l if hb == hb_l else 0xFFFF) + 1
        i = at.get(hb)
        if i is not None:
            t, v = container_op(FLIP, conts[i][1], conts[i][2], b, e)
            if len(v):
                out.append((hb, t, v))
        else:
            out.append((hb,) + range_of_ones(b, e))
    return out + [c for c in conts if c[0] > hb_l]


def inplace_add(conts, start, end):
    """x.add(rangeStart, rangeEnd) (:1181-1208): iadd on every container found in the span — the keys strictly
    inside it included, where the static add writes rangeOfOnes(0, 65536) instead."""
    range_sanity_check(start, end)
    if start >= end:
        return list(conts)
    hb_s, lb_s, hb_l, lb_l = _split(start, end)
    at = _index(conts)
    out = [c for c in conts if c[0] < hb_s]
    for hb in range(hb_s, hb_l + 1):                                            # :1191-1207
        b = lb_s if hb == hb_s else 0
        e = (lb_l if hb == hb_l else 0xFFFF) + 1
        i = at.get(hb)
        out.append((hb,) + (container_op(ADD, conts[i][1], conts[i][2], b, e) if i is not None
                            else range_of_ones(b, e)))
    return out + [c for c in conts if c[0] > hb_l]


def inplace_remove(conts, start, end):
    """x.remove(rangeStart, rangeEnd) (:2656-2711): iremove on the two edge containers (skipped when the edge is a
    whole container), then removeIndexRange over what lies between and the edges left empty."""
    range_sanity_check(start, end)
    if start >= end:
        return list(conts)
    hb_s, lb_s, hb_l, lb_l = _split(start, end)
    work = list(conts)
    at = _index(work)
    if hb_s == hb_l:                                                            # :2669-2681
        i = at.get(hb_s)
        if i is None:
            return work
        t, v = container_op(REMOVE, work[i][1], work[i][2], lb_s, lb_l + 1)
        if len(v):
            work[i] = (hb_s, t, v)
        else:
            del work[i]
        return work
    keys = [c[0] for c in work]
    ifirst = at.get(hb_s, -int(np.searchsorted(keys, hb_s)) - 1)                # getIndex
    ilast = at.get(hb_l, -int(np.searchsorted(keys, hb_l)) - 1)
    if ifirst >= 0:                                                             # :2684-2695
        if lb_s != 0:
            t, v = container_op(REMOVE, work[ifirst][1], work[ifirst][2], lb_s, 65536)
            if len(v):
                work[ifirst] = (hb_s, t, v)
                ifirst += 1
    else:
        ifirst = -ifirst - 1
    if ilast >= 0:                                                              # :2696-2709
        if lb_l != 0xFFFF:
            t, v = container_op(REMOVE, work[ilast][1], work[ilast][2], 0, lb_l + 1)
            if len(v):
                work[ilast] = (hb_l, t, v)
            else:
                ilast += 1
        else:
            ilast += 1
    else:
        ilast = -ilast - 1
    del work[ifirst:ilast]                                                      # :2710 removeIndexRange
    return work


def bitmap_of_range(lo, hi):
    """RoaringBitmap.bitmapOfRange(min, max) (:588-615).  `RunContainer.rangeOfOnes` there is Container's static
    method reached through the subclass (RunContainer declares none): the threshold of 2 applies."""
    range_sanity_check(lo, hi)
    if lo >= hi:
        return []
    hb_s, lb_s, hb_l, lb_l = _split(lo, hi)
    out = [(hb_s,) + range_of_ones(lb_s, 65536 if hb_s < hb_l else lb_l + 1)]   # :601-603
    if hb_s < hb_l:
        out += [(hb,) + range_of_ones(0, 65536) for hb in range(hb_s + 1, hb_l)]
        out.append((hb_l,) + range_of_ones(0, lb_l + 1))
    return out


_STATIC = {ADD: static_add, REMOVE: static_remove, FLIP: static_flip}
_INPLACE = {ADD: inplace_add, REMOVE: inplace_remove, FLIP: static_flip}


def range_op(op: int, conts, start: int, end: int, inplace: bool = False):
    return (_INPLACE if inplace else _STATIC)[op](conts, int(start), int(end))


# ------------------------------------------------------------------------------------------- forms
def cardinality(conts) -> int:
    return sum(len(v) for _, _, v in conts)


def values_of(conts) -> np.ndarray:
    """The members as uint64 (a whole-universe result does not fit a test's memory: callers keep those to counts)."""
    if not conts:
        return np.zeros(0, np.uint64)
    return np.concatenate([(np.uint64(k) << np.uint64(16)) | v.astype(np.uint64) for k, _, v in conts])


def conts_of(ref) -> list:
    """An oracle bitmap (rbref.RefBitmap) as [(key, type, values)]."""
    vals = ref.to_array()
    hi = vals >> 16
    out = []
    for key, t, card, _ in ref.containers():
        k = hi.dtype.type(key)  # a Python int would make numpy convert the whole array on every call
        a, b = np.searchsorted(hi, k, "left"), np.searchsorted(hi, k, "right")
        assert b - a == card
        out.append((key, t, (vals[a:b] & 0xFFFF).astype(np.uint32)))
    return out


def _payload(t, v) -> bytes:
    if t == ARRAY:
        return v.astype(np.uint16).tobytes()
    if t == BITMAP:
        return np.packbits(_bits(v), bitorder="little").tobytes()
    x = v.astype(np.int64)
    brk = np.nonzero(np.diff(x) != 1)[0]
    starts, ends = np.concatenate([[0], brk + 1]), np.concatenate([brk, [len(x) - 1]])
    return np.stack([x[starts], x[ends] - x[starts]], axis=1).astype(np.uint16).tobytes()


def to_oracle(R, conts):
    """The oracle's bitmap of [(key, type, values)], container types as given: the bytes are its serializer's.  The
    payload of a (type, array object) seen before is shared (65536 full Runs are one payload)."""
    seen, chunks, offs, nruns, pos = {}, [], [], [], 0
    for _, t, v in conts:
        assert len(v), "the reference drops empty containers"
        tag = (t, id(v))
        if tag not in seen:
            p = _payload(t, v)
            seen[tag] = (pos, n_runs(v) if t == RUN else 0)
            chunks.append(p)
            pos += len(p)
        offs.append(seen[tag][0])
        nruns.append(seen[tag][1])
    return R.from_soa([k for k, _, _ in conts], [t for _, t, _ in conts], [len(v) for _, _, v in conts], nruns,
                      np.frombuffer(b"".join(chunks) or b"\0\0", np.uint8), offs)


def census(op: int, conts, start: int, end: int, inplace: bool = False) -> set:
    """The (source type or None, op, result type or None) transitions of the keys inside the span."""
    if start >= end:
        return set()
    hb_s, hb_l = start >> 16, (end - 1) >> 16
    src = {k: t for k, t, _ in conts}
    res = {k: t for k, t, _ in range_op(op, conts, start, end, inplace)}
    keys = [k for k in set(src) | set(res) if hb_s <= k <= hb_l]
    return {(src.get(k), op, res.get(k)) for k in keys}


# ------------------------------------------------------------------------------------------- seeded fuzz
# Every (source type, op, result type) the container table allows, None = no container.  The static add also writes
# a full Run over an Array or a Bitmap strictly inside its span (RoaringBitmap.java:332-335).
ALLOWED = {
    (None, ADD, ARRAY), (None, ADD, RUN), (ARRAY, ADD, ARRAY), (ARRAY, ADD, BITMAP), (BITMAP, ADD, BITMAP),
    (RUN, ADD, RUN), (ARRAY, ADD, RUN), (BITMAP, ADD, RUN),
    (ARRAY, REMOVE, ARRAY), (ARRAY, REMOVE, None), (BITMAP, REMOVE, BITMAP), (BITMAP, REMOVE, ARRAY),
    (BITMAP, REMOVE, None), (RUN, REMOVE, RUN), (RUN, REMOVE, None),
    (None, FLIP, ARRAY), (None, FLIP, RUN), (ARRAY, FLIP, ARRAY), (ARRAY, FLIP, BITMAP), (ARRAY, FLIP, None),
    (BITMAP, FLIP, BITMAP), (BITMAP, FLIP, ARRAY), (BITMAP, FLIP, None), (RUN, FLIP, RUN), (RUN, FLIP, ARRAY),
    (RUN, FLIP, BITMAP), (RUN, FLIP, None),
}


def _shape(rng, kind):
    """(type, values) of one container."""
    if kind == "a_block":      # a short block: a flip over exactly it empties the container
        b = int(rng.integers(0, 65000))
        return ARRAY, np.arange(b, b + int(rng.integers(1, 6)), dtype=np.uint32)
    if kind == "a_sparse":
        return ARRAY, np.unique(rng.integers(0, 65536, size=int(rng.integers(1, 3000)))).astype(np.uint32)
    if kind == "a_4096":
        return ARRAY, np.sort(rng.choice(65536, size=int(rng.integers(4090, 4097)), replace=False)).astype(np.uint32)
    if kind == "b_block":      # a contiguous Bitmap (legal: not every bitmap is run-optimized)
        b = int(rng.integers(0, 30000))
        return BITMAP, np.arange(b, b + int(rng.integers(4097, 30000)), dtype=np.uint32)
    if kind == "b_4097":
        return BITMAP, np.sort(rng.choice(65536, size=int(rng.integers(4097, 4104)), replace=False)).astype(np.uint32)
    if kind == "b_dense":
        return BITMAP, np.sort(rng.choice(65536, size=int(rng.integers(20000, 65000)), replace=False)).astype(np.uint32)
    if kind == "r_one":
        b = int(rng.integers(0, 60000))
        return RUN, np.arange(b, b + int(rng.integers(3, 5000)), dtype=np.uint32)
    if kind == "r_pairs":      # runs of length 2: 2 + 4 r against 2 + 2 c is a tie, one value less tips it to Array
        n = int(rng.integers(2, 400))
        s = 5 * np.arange(n, dtype=np.uint32) + int(rng.integers(0, 1000))
        return RUN, np.sort(np.concatenate([s, s + 1]))
    if kind == "r_2047":       # 2 + 4 * 2047 = 8190: one more run and the Bitmap is smaller
        s = 8 * np.arange(2047, dtype=np.uint32) + int(rng.integers(0, 100))
        return RUN, np.sort(np.concatenate([s, s + 1, s + 2]))
    if kind == "r_many":       # a Run larger than its Bitmap: add / remove keep it a Run
        s = 4 * np.arange(int(rng.integers(2100, 5000)), dtype=np.uint32)
        return RUN, np.sort(np.concatenate([s, s + 1]))
    assert kind == "r_full"
    return RUN, FULL


SHAPES = ["a_block", "a_sparse", "a_4096", "b_block", "b_4097", "b_dense", "r_one", "r_pairs", "r_2047", "r_many",
          "r_full"]


def fuzz_cases(seed: int, n: int):
    """n cases (conts, op, start, end, inplace): bitmaps of 1..6 containers drawn from SHAPES on scattered keys, and
    ranges aimed at what the type table distinguishes: a container's exact hull, a point on or off a member, the whole
    key, spans of two and of many keys, one or two values at a key not held, and plain random ranges."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        keys = np.sort(rng.choice(12, size=int(rng.integers(1, 7)), replace=False)) + int(rng.integers(0, 65524))
        conts = [(int(k),) + _shape(rng, SHAPES[int(rng.integers(0, len(SHAPES)))]) for k in keys]
        k, _, v = conts[int(rng.integers(0, len(conts)))]
        base = k << 16
        aim = ["hull", "member", "absent", "key", "two", "many", "random", "empty", "inside", "fresh"][i % 10]
        if aim == "fresh":  # one or two values at a key the bitmap does not hold: rangeOfOnes' Array
            kk = int(keys[-1]) + 1 if int(keys[-1]) < 65535 else int(keys[0]) - 1
            s = (kk << 16) + int(rng.integers(0, 65534))
            e = s + int(rng.integers(1, 3))
        elif aim == "hull":
            s, e = base + int(v[0]), base + int(v[-1]) + 1
        elif aim == "member":
            s = base + int(v[int(rng.integers(0, len(v)))])
            e = s + 1
        elif aim == "absent":
            s = base + int(rng.integers(0, 65536))
            e = s + int(rng.integers(1, 4))
        elif aim == "key":
            s, e = base, base + 65536
        elif aim == "two":
            s = base + int(rng.integers(0, 65536))
            e = s + int(rng.integers(1, 65536))
        elif aim == "many":
            s = (int(keys[0]) << 16) + int(rng.integers(0, 65536))
            e = (int(keys[-1]) << 16) + int(rng.integers(1, 65537))
        elif aim == "random":
            s = base + int(rng.integers(0, 65536))
            e = s + int(rng.integers(0, 3 << 16))
        elif aim == "empty":
            s = base + int(rng.integers(0, 65536))
            e = s - int(rng.integers(0, 5))
        else:
            s = base + int(v[0]) + 1
            e = max(s + 1, base + int(v[-1]))
        s, e = min(s, (1 << 32) - 1), min(max(e, 0), 1 << 32)
        cases.append((conts, int(rng.integers(0, 3)), s, e, bool(rng.integers(0, 2))))
    return cases


def fuzz_census(cases) -> set:
    out = set()
    for conts, op, s, e, inplace in cases:
        out |= census(op, conts, s, e, inplace)
    return out
