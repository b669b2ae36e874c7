"""Container-type decision boundaries as data: one-container operand pairs whose RESULT lands exactly
on an edge of a type rule, for test_type_boundaries.py (oracle against the rule) and test_gpu_type_boundaries.py
(device against the oracle).  Pure numpy; the oracle and the device are only touched by the helper functions at
the end, when a test calls them.

Group "target": a case is (op, ka, kb, target).  target = (c, r) is the cardinality and the number of maximal runs
of the result set T; ka, kb are operand kinds: "A" Array, "B" Bitmap, "R" Run and, for the pairs whose rule reads
the Array's cardinality (RunContainer.xor / andNot switch at |Array| < 32), "a" = an Array of at most 31 values
while "A" then holds at least 32.  build_operands() makes A and B of those kinds with A op B == T:
  AND     A = T u Ea, B = T u Eb, Ea and Eb disjoint and outside T
  OR      A = a prefix of T, B = a suffix of T, overlapping where the kinds leave room
  XOR     A = T1 u S, B = T2 u S, T = T1 + T2 (prefix, suffix), S outside T
  ANDNOT  A = T u S, B = S u E, S and E outside T
with the extras sized so that each operand fits its kind (Array 1..4096 values, Bitmap >= 4097, Run any set).
What cannot be built is listed in INFEASIBLE with its reason; built + listed is the whole product.

Group "array32": RunContainer.xor / andNot against an Array of 31 and of 32 values.
Group "operand": operand representations of the register path (Runs of 2047 / 2048 / 2049 / 5000 runs: the last
two are staged from global memory) and Run AND Run on both sides of the interval path's scratch fit."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from type_pins import ARRAY, BITMAP, RUN, payload_of, runs_of

OPS = {"AND": 0, "OR": 1, "XOR": 2, "ANDNOT": 3}
SPAN = 65536
KIND_TYPE = {"A": ARRAY, "a": ARRAY, "B": BITMAP, "R": RUN}

TARGETS: List[Tuple[int, int]] = [
    (4096, 1), (4097, 1), (4096, 7), (4097, 7),                                               # AB edge
    (100, 50), (99, 50), (14, 7), (13, 7), (4094, 2047), (4093, 2047),                        # EFF tie c = 2r | 2r - 1
    (4096, 2047), (4096, 2048), (4097, 2047), (4097, 2048), (8190, 2047), (20000, 2047), (20000, 2048),  # EFF 8 KiB
    (8192, 4096), (8194, 4097),                                                               # lazyorToRun's 4096 runs
    (1, 1), (65535, 2), (65536, 1), (0, 0),                                                   # ends, the empty result
]
# pairs of targets that differ only in the side of one edge they are on
EFF_EDGES = [((100, 50), (99, 50)), ((14, 7), (13, 7)), ((4094, 2047), (4093, 2047)),
             ((4096, 2047), (4096, 2048)), ((4097, 2047), (4097, 2048)), ((20000, 2047), (20000, 2048))]
AB_EDGES = [((4096, 1), (4097, 1)), ((4096, 7), (4097, 7))]


@dataclass(frozen=True, eq=False)
class Case:
    id: str
    group: str                         # target | array32 | operand
    op: str
    ta: int
    tb: int
    a: np.ndarray                      # sorted uint32 values (low 16 bits) of the left container
    b: np.ndarray
    kinds: Optional[Tuple[str, str]] = None
    target: Optional[Tuple[int, int]] = None

    @property
    def max_operand_runs(self) -> int:
        return max(len(runs_of(v)) if t == RUN else 0 for t, v in ((self.ta, self.a), (self.tb, self.b)))


# ------------------------------------------------------------------ sets
def _u(*parts) -> np.ndarray:
    parts = [np.asarray(p, np.uint32) for p in parts]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint32)


def card_runs(vals) -> Tuple[int, int]:
    v = np.asarray(vals, np.int64)
    return len(v), (int((np.diff(v) != 1).sum()) + 1 if len(v) else 0)


def result_set(op: str, a, b) -> np.ndarray:
    f = {"AND": np.intersect1d, "OR": np.union1d, "XOR": np.setxor1d, "ANDNOT": np.setdiff1d}[op]
    return f(a, b).astype(np.uint32)


def target_set(c: int, r: int) -> np.ndarray:
    """c values in r maximal runs of near-equal length, one value apart, starting at 3 where there is room."""
    if c == 0:
        return np.zeros(0, np.uint32)
    assert 1 <= r <= c and c + r - 1 <= SPAN
    lens = [c // r + (1 if i < c % r else 0) for i in range(r)]
    pos = min(3, SPAN - (c + r - 1))
    parts = []
    for n in lens:
        parts.append(np.arange(pos, pos + n, dtype=np.uint32))
        pos += n + 1
    return np.concatenate(parts)


def _pool(t: np.ndarray) -> np.ndarray:
    """The values outside T in the order the extras are drawn: the block above T (not touching it), then the rest."""
    free = np.setdiff1d(np.arange(SPAN, dtype=np.uint32), t)
    if len(t) == 0:
        return np.roll(free, -5)
    above = free > int(t[-1]) + 1
    return np.concatenate([free[above], free[~above]])


def _clamp(x, lo, hi):
    return max(lo, min(hi, x))


# ------------------------------------------------------------------ group "target"
def kind_pairs(op: str) -> List[Tuple[str, str]]:
    pairs = [(x, y) for x in "ABR" for y in "ABR"]
    if op == "XOR":
        pairs += [("a", "R"), ("R", "a")]
    if op == "ANDNOT":
        pairs += [("R", "a")]
    return pairs


def bounds(op: str, ka: str, kb: str):
    """((lo, hi) of |A|, (lo, hi) of |B|) for the kinds."""
    reads_array_card = (op == "XOR" and {ka, kb} == {"A", "R"}) or (op == "ANDNOT" and (ka, kb) == ("R", "A"))

    def one(k):
        if k == "a":
            return 1, 31
        if k == "A":
            return (32 if reads_array_card else 1), 4096
        return (4097, SPAN) if k == "B" else (1, SPAN)
    return one(ka), one(kb)


def product():
    return [(op, ka, kb, t) for op in OPS for ka, kb in kind_pairs(op) for t in TARGETS]


def case_id(op, ka, kb, target) -> str:
    return f"{op}-{ka}{kb}-{target[0]}x{target[1]}"


def infeasible_reason(op, ka, kb, target) -> Optional[str]:
    """Why no operands of these kinds give this result, from set arithmetic alone (not from the builder)."""
    c = target[0]
    (la, ha), (lb, hb) = bounds(op, ka, kb)
    outside = SPAN - c
    if op == "AND":
        if c > min(ha, hb):
            return "AND with an Array operand cannot exceed 4096 values"
        if max(la, c) + max(lb, c) - c > SPAN:
            return "two operands that share only the result do not fit 65536 values"
    elif op == "OR":
        if c == 0:
            return "OR of two containers is never empty"
        if max(la, lb) > c:
            return "OR with a Bitmap operand has at least 4097 values"
        if ha + hb < c:
            return "OR of two Arrays cannot exceed 8192 values"
    elif op == "XOR":
        if ha + hb < c:
            return "XOR of two Arrays cannot exceed 8192 values"
        if la - hb > c or lb - ha > c:
            return "the operands' cardinalities differ by at most the result's: equal sets are no Array and Bitmap"
    else:
        if c > ha:
            return "ANDNOT from an Array cannot exceed 4096 values"
        if lb > outside:
            return "the right operand lies outside the result: too few values are left for it"
        if max(0, la - c) > min(hb, outside):
            return "an empty result needs A inside B: a Bitmap is inside no Array"
    return None


INFEASIBLE: Dict[str, str] = {}
for _p in product():
    _why = infeasible_reason(*_p)
    if _why:
        INFEASIBLE[case_id(*_p)] = _why


def build_operands(op, ka, kb, target):
    """(A, B) value arrays of the kinds with A op B == target_set(*target), or None."""
    c, r = target
    t = target_set(c, r)
    pool = _pool(t)
    avail = len(pool)
    (la, ha), (lb, hb) = bounds(op, ka, kb)
    if op == "AND":
        ea_lo, eb_lo, ea_hi, eb_hi = max(0, la - c), max(0, lb - c), ha - c, hb - c
        if ea_hi < ea_lo or eb_hi < eb_lo or ea_lo + eb_lo > avail:
            return None
        spare = avail - ea_lo - eb_lo
        ea = min(ea_hi, ea_lo + min(40, spare // 2))
        eb = min(eb_hi, eb_lo + min(30, spare - (ea - ea_lo)))
        return _u(t, pool[:ea]), _u(t, pool[ea:ea + eb])
    if op == "OR":
        ha, hb = min(ha, c), min(hb, c)
        if c == 0 or la > ha or lb > hb or ha + hb < c:
            return None
        want = -(-3 * c // 5)
        na = _clamp(want, la, ha)
        nb = _clamp(max(want, c - na), lb, hb)
        if na + nb < c:
            na = _clamp(c - nb, la, ha)
        assert na + nb >= c
        return t[:na].copy(), t[c - nb:].copy()
    if op == "XOR":
        s_lo = max(0, la - c, lb - c, -((c - la - lb) // 2))
        s_hi = min(avail, ha, hb, (ha + hb - c) // 2)
        if s_lo > s_hi:
            return None
        s = _clamp(40, s_lo, s_hi)
        t_lo, t_hi = max(0, la - s, c + s - hb), min(c, ha - s, c + s - lb)
        assert t_lo <= t_hi
        t1 = _clamp(c // 2, t_lo, t_hi)
        return _u(t[:t1], pool[:s]), _u(t[t1:], pool[:s])
    s_lo, s_hi = max(0, la - c), min(ha - c, avail, hb)
    if s_lo > s_hi or avail < lb:
        return None
    s = _clamp(40, s_lo, s_hi)
    e_lo, e_hi = max(0, lb - s), min(hb - s, avail - s)
    assert e_lo <= e_hi
    e = _clamp(30, e_lo, e_hi)
    return _u(t, pool[:s]), _u(pool[:s + e])


def _target_cases() -> List[Case]:
    out = []
    for op, ka, kb, t in product():
        ab = build_operands(op, ka, kb, t)
        if ab is not None:
            out.append(Case(case_id(op, ka, kb, t), "target", op, KIND_TYPE[ka], KIND_TYPE[kb], ab[0], ab[1],
                            (ka, kb), t))
    return out


# ------------------------------------------------------------------ group "array32"
def _array32_cases() -> List[Case]:
    out = []
    for c in (1000, 30000):
        half = c // 2
        run = _u(np.arange(100, 100 + half), np.arange(40000 - half, 40000))
        second = 40000 - half + 2
        inner = np.concatenate([np.arange(102, 102 + 2 * 16, 2), np.arange(second, second + 2 * 16, 2)])
        for n in (31, 32):  # n isolated interior values of the two runs: 2 + n runs are left
            arr = np.sort(inner[:n]).astype(np.uint32)
            out.append(Case(f"XOR-R{c}^A{n}", "array32", "XOR", RUN, ARRAY, run, arr))
            out.append(Case(f"XOR-A{n}^R{c}", "array32", "XOR", ARRAY, RUN, arr, run))
            out.append(Case(f"ANDNOT-R{c}-A{n}", "array32", "ANDNOT", RUN, ARRAY, run, arr))
    return out


ARRAY32_PAIRS = [(f"XOR-R{c}^A31", f"XOR-R{c}^A32") for c in (1000, 30000)] + \
                [(f"XOR-A31^R{c}", f"XOR-A32^R{c}") for c in (1000, 30000)] + \
                [(f"ANDNOT-R{c}-A31", f"ANDNOT-R{c}-A32") for c in (1000, 30000)]


# ------------------------------------------------------------------ group "operand"
def _periodic(n, period, first, last):
    """n runs [k * period + first, k * period + last], k = 0 .. n - 1."""
    k = np.arange(n, dtype=np.int64)[:, None] * period
    v = (k + np.arange(first, last + 1, dtype=np.int64)[None, :]).ravel()
    assert v[-1] < SPAN
    return v.astype(np.uint32)


FIT_PAIRS = [(1021, 1024), (1022, 1025), (1, 2044), (1, 2045), (1024, 1024)]  # ((ra + 3) & ~3) + rb <= 2048 or not


def run_and_run_operands(ra: int, rb: int, kind: str):
    """Run lists of ra and rb runs whose intersection stays a Run ("run": 7-value overlaps), fails EFF and is an
    Array ("array": 1-value overlaps) or is empty.  A one-run list is the whole container (empty: a run below
    the other list).  No pair that fits the scratch gives a Bitmap: an intersection has at most ra + rb - 1 <= 2047
    runs and a Bitmap needs 2048 (2 + 4r > 8192); "bitmap" is (1500, 1500) with 2-value overlaps on the full path."""
    p = SPAN // max(ra, rb)
    assert p >= 32
    xs, ys = {"run": ((0, 12), (6, 20)), "array": ((0, 12), (12, 20)), "empty": ((0, 5), (10, 20))}[kind]
    if kind == "array" and ra == 1:
        ys = (12, 12)
    a = _periodic(ra, p, *xs)
    if ra == 1:
        a = np.arange(0, 6 if kind == "empty" else SPAN, dtype=np.uint32)
    return a, _periodic(rb, p, *ys)


def _operand_cases() -> List[Case]:
    rng = np.random.default_rng(2047)
    partners = {
        "B": (BITMAP, np.sort(rng.choice(SPAN, 30000, replace=False)).astype(np.uint32)),
        "A": (ARRAY, np.sort(rng.choice(SPAN, 3000, replace=False)).astype(np.uint32)),
        "R": (RUN, _u(*[np.arange(s, s + n) for s, n in zip(np.sort(rng.choice(SPAN - 200, 300, replace=False)),
                                                             rng.integers(1, 150, 300))])),
    }
    out = []
    for n in (2047, 2048, 2049, 5000):
        p = min(32, SPAN // n)
        big = _periodic(n, p, 1, p // 3)
        assert card_runs(big)[1] == n
        for op in OPS:
            for k, (t, v) in partners.items():
                out.append(Case(f"{op}-R{n}-{k}", "operand", op, RUN, t, big, v))
                out.append(Case(f"{op}-{k}-R{n}", "operand", op, t, RUN, v, big))
    for ra, rb in FIT_PAIRS:
        for kind in ("run", "array", "empty"):
            a, b = run_and_run_operands(ra, rb, kind)
            assert (card_runs(a)[1], card_runs(b)[1]) == (ra, rb)
            out.append(Case(f"AND-R{ra}&R{rb}-{kind}", "operand", "AND", RUN, RUN, a, b))
            if ra != rb:
                out.append(Case(f"AND-R{rb}&R{ra}-{kind}", "operand", "AND", RUN, RUN, b, a))
    a, b = _periodic(1500, 43, 0, 30), _periodic(1500, 43, 29, 44)
    out.append(Case("AND-R1500&R1500-bitmap", "operand", "AND", RUN, RUN, a, b))
    return out


_CASES: Optional[List[Case]] = None


def all_cases() -> List[Case]:
    global _CASES
    if _CASES is None:
        _CASES = _target_cases() + _array32_cases() + _operand_cases()
        assert len({c.id for c in _CASES}) == len(_CASES)
    return _CASES


def cases_of(op: str, small_path_only: bool = False) -> List[Case]:
    """The op's cases; small_path_only drops those with a Run operand of more than 2048 runs, which the
    small-batch kernel refuses (a copy of it would not fit an 8 KiB slot)."""
    return [c for c in all_cases() if c.op == op and not (small_path_only and c.max_operand_runs > 2048)]


# ------------------------------------------------------------------ device / oracle forms
def keyed_soa(bitmaps):
    """HostSoA of bitmaps given as lists of (key, type, values), keys ascending: containers of exactly those types."""
    from roaringbitmap_amd.engine import HostSoA
    begin, keys, types, cards, nruns, offs, chunks = [0], [], [], [], [], [], []
    pos = 0
    for conts in bitmaps:
        assert [k for k, _, _ in conts] == sorted({k for k, _, _ in conts})
        for k, t, v in conts:
            data = payload_of(t, v)
            keys.append(k)
            types.append(t)
            cards.append(len(v))
            nruns.append(len(runs_of(v)) if t == RUN else 0)
            offs.append(pos)
            pad = (-len(data)) % 16
            chunks.append(data + b"\0" * pad)
            pos += len(data) + pad
        begin.append(len(keys))
    return HostSoA(np.array(begin, np.uint64), np.array(keys, np.uint16), np.array(types, np.uint8),
                   np.array(cards, np.uint32), np.array(nruns, np.uint16), np.array(offs, np.uint64),
                   np.frombuffer(b"".join(chunks) or b"\0" * 16, np.uint8).copy())


def oracle_keyed(oracle, conts):
    """The oracle's bitmap of one list of (key, type, values)."""
    data, offs, pos = [], [], 0
    for _, t, v in conts:
        p = payload_of(t, v)
        offs.append(pos)
        data.append(p)
        pos += len(p)
    return oracle.from_soa([k for k, _, _ in conts], [t for _, t, _ in conts], [len(v) for _, _, v in conts],
                           [len(runs_of(v)) if t == RUN else 0 for _, t, v in conts],
                           np.frombuffer(b"".join(data) or b"\0\0", np.uint8), offs)


def many_key_bitmaps(cases):
    """Two bitmaps in which key k holds case k's operands."""
    return ([(k, c.ta, c.a) for k, c in enumerate(cases)], [(k, c.tb, c.b) for k, c in enumerate(cases)])
