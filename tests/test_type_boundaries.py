"""The oracle's procedural port (run_eff, run_xor_array, ...) against the declarative type rule of SURVEY §8a, on
the case set of type_boundary_cases.py: every result's values, its (cardinality, runs) and its container type.
The rule below is the one the device restates (wave.hpp type_eff / type_ab / type_lr, pairwise.hip eff_rule); if
it and the oracle disagree the reference's Java decides.  The coverage tests keep the case set on the edges."""
import numpy as np
import pytest

import type_boundary_cases as tb
from type_pins import ARRAY, BITMAP, RUN, TYPE_NAME, oracle_bitmap

OPS = tb.OPS
CASES = tb.all_cases()
BY_ID = {c.id: c for c in CASES}


def expected_type(op, ta, tb_, ca, cb, c, r):
    """Result container type of a matched pair, None when the (empty) result is dropped."""
    if c == 0:
        return None  # RoaringBitmap.java:389-391, 1084-1086, 455-471; an OR is never empty
    ab = ARRAY if c <= 4096 else BITMAP  # RunContainer.java:2300-2323, BitmapContainer.java:1393-1396
    eff = RUN if 2 + 4 * r <= min(8192, 2 * c + 2) else ab  # RunContainer.java:2326-2335: ties go to Run
    lr = RUN if c == 65536 else ab  # BitmapContainer.java:1214-1224, 1073-1110, 769-778
    runs = (ta == RUN) + (tb_ == RUN)
    if op == "AND":  # RunContainer.java:381-456; every other pair :305-378, BitmapContainer.java:162-188
        return eff if runs == 2 else ab
    if op == "OR":
        if BITMAP in (ta, tb_):
            return lr
        # ArrayContainer.java:949-973; RunContainer.java:1926-1986 (lazyorToRun :1769-1813 keeps at most 4096
        # runs, then :861-875 + repairAfterLazy: more than 4096 runs are more than 4096 values, a Bitmap as EFF says)
        return ab if runs == 0 else eff
    if runs == 2:  # RunContainer.java:2448-2482 (xor), :624-692 (andNot)
        return eff
    if op == "XOR" and runs == 1 and ARRAY in (ta, tb_):  # RunContainer.java:2410-2428: |Array| < 32 -> lazyxor + EFF
        return eff if (ca if ta == ARRAY else cb) < 32 else ab
    if op == "ANDNOT" and ta == RUN and tb_ == ARRAY:  # RunContainer.java:574-584: |Array| < 32 -> lazyandNot + EFF
        return eff if cb < 32 else ab
    return ab  # ArrayContainer.java:222-271, 1311-1336; BitmapContainer.java:221-274, 1381-1422


def oracle_result(oracle, case):
    res = oracle.op(OPS[case.op], oracle_bitmap(oracle, case.ta, case.a), oracle_bitmap(oracle, case.tb, case.b))
    cs = res.containers()
    assert len(cs) <= 1
    return res, (cs[0][1] if cs else None)


def rule_type(case):
    c, r = tb.card_runs(tb.result_set(case.op, case.a, case.b))
    return expected_type(case.op, case.ta, case.tb, len(case.a), len(case.b), c, r)


def test_built_plus_listed_is_the_whole_product():
    prod = tb.product()
    assert len(prod) == (4 * 9 + 3) * len(tb.TARGETS) and len(set(tb.TARGETS)) == len(tb.TARGETS)
    built = {c.id for c in CASES if c.group == "target"}
    assert not built & set(tb.INFEASIBLE)
    assert built | set(tb.INFEASIBLE) == {tb.case_id(*p) for p in prod}
    assert len(built) + len(tb.INFEASIBLE) == len(prod)
    for p in prod:  # the builder gives up exactly where the table says so
        assert (tb.build_operands(*p) is None) == (tb.case_id(*p) in tb.INFEASIBLE), p


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_operands_are_what_the_case_says(case):
    for t, v in ((case.ta, case.a), (case.tb, case.b)):
        assert len(v) >= 1 and np.all(np.diff(v.astype(np.int64)) > 0) and int(v[-1]) < 65536
        assert t != ARRAY or len(v) <= 4096
        assert t != BITMAP or len(v) >= 4097
    if case.group == "target":
        want = tb.target_set(*case.target)
        assert np.array_equal(tb.result_set(case.op, case.a, case.b), want)
        assert tb.card_runs(want) == case.target
        (la, ha), (lb, hb) = tb.bounds(case.op, *case.kinds)
        assert la <= len(case.a) <= ha and lb <= len(case.b) <= hb


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_oracle_type_is_the_rule(oracle, case):
    want = tb.result_set(case.op, case.a, case.b)
    c, r = tb.card_runs(want)
    res, t = oracle_result(oracle, case)
    assert np.array_equal(res.to_array(), want)
    assert res.cardinality() == c
    if case.target is not None:
        assert (c, r) == case.target
    rule = expected_type(case.op, case.ta, case.tb, len(case.a), len(case.b), c, r)
    assert t == rule, f"{case.id}: oracle {TYPE_NAME.get(t)} != rule {TYPE_NAME.get(rule)} at c={c} r={r}"
    if t == RUN:
        assert res.containers()[0][3] == r
    assert oracle.op_cardinality(OPS[case.op], oracle_bitmap(oracle, case.ta, case.a),
                                 oracle_bitmap(oracle, case.tb, case.b)) == c


def _eff_applies(op, ka, kb):
    if (ka, kb) == ("R", "R"):
        return True
    if op == "OR":
        return {ka, kb} == {"A", "R"}
    return (op == "XOR" and {ka, kb} == {"a", "R"}) or (op == "ANDNOT" and (ka, kb) == ("R", "a"))


def test_both_sides_of_every_eff_edge():
    seen = 0
    for op in OPS:
        for ka, kb in tb.kind_pairs(op):
            if not _eff_applies(op, ka, kb):
                continue
            for run_side, other_side in tb.EFF_EDGES:
                ids = [tb.case_id(op, ka, kb, t) for t in (run_side, other_side)]
                assert all(i in BY_ID for i in ids), ids
                assert rule_type(BY_ID[ids[0]]) == RUN != rule_type(BY_ID[ids[1]]), ids
                seen += 1
    assert seen == (4 + 2 + 2 + 1) * len(tb.EFF_EDGES)  # R.R of each op, A|R, R|A, a^R, R^a, R\a


def test_both_sides_of_the_array_bitmap_edge():
    seen = 0
    for op in OPS:
        for ka, kb in tb.kind_pairs(op):
            for at, above in tb.AB_EDGES:
                ids = [tb.case_id(op, ka, kb, t) for t in (at, above)]
                if all(i in tb.INFEASIBLE for i in ids):
                    continue
                if _eff_applies(op, ka, kb):  # (4096 | 4097 values, 1 | 7 runs) stay a Run on both sides
                    assert [rule_type(BY_ID[i]) for i in ids] == [RUN, RUN], ids
                    continue
                if ids[0] in tb.INFEASIBLE:  # a Bitmap operand of an OR: 4097 values is the least
                    assert op == "OR" and "B" in (ka, kb) and rule_type(BY_ID[ids[1]]) == BITMAP
                    continue
                if ids[1] in tb.INFEASIBLE:  # an Array that holds the result: 4096 values is the most
                    assert op in ("AND", "ANDNOT") and "A" in (ka, kb) and rule_type(BY_ID[ids[0]]) == ARRAY
                    continue
                assert [rule_type(BY_ID[i]) for i in ids] == [ARRAY, BITMAP], ids
                seen += 1
    # B&B B&R R&B, A|A, every XOR pair but R^R and the two with "a", B\A B\B B\R R\A R\B
    assert seen == (3 + 1 + 8 + 5) * len(tb.AB_EDGES)


def test_the_8_kib_and_lazy_or_edges_beyond_the_pairs():
    for op in OPS:  # 8190 values in 2047 runs: the largest Run that ties with its Array size is far below
        assert rule_type(BY_ID[tb.case_id(op, "R", "R", (8190, 2047))]) == RUN
    assert rule_type(BY_ID[tb.case_id("OR", "A", "R", (8192, 4096))]) == BITMAP   # 4096 runs: still a Run list, EFF
    assert rule_type(BY_ID[tb.case_id("OR", "A", "R", (8194, 4097))]) == BITMAP   # 4097 runs: lazy Bitmap, repaired
    assert rule_type(BY_ID[tb.case_id("OR", "R", "R", (65536, 1))]) == RUN
    assert rule_type(BY_ID[tb.case_id("OR", "B", "B", (65536, 1))]) == RUN
    assert rule_type(BY_ID[tb.case_id("XOR", "B", "B", (65536, 1))]) == BITMAP
    for op in ("AND", "XOR", "ANDNOT"):
        assert any(c.op == op and c.target == (0, 0) for c in CASES)


def test_each_31_32_pair_differs_in_type(oracle):
    for lo, hi in tb.ARRAY32_PAIRS:
        t31, t32 = oracle_result(oracle, BY_ID[lo])[1], oracle_result(oracle, BY_ID[hi])[1]
        assert t31 == RUN and t32 in (ARRAY, BITMAP), (lo, hi)
        assert rule_type(BY_ID[lo]) == t31 and rule_type(BY_ID[hi]) == t32
    got = {i: tb.card_runs(tb.result_set(BY_ID[i].op, BY_ID[i].a, BY_ID[i].b)) for p in tb.ARRAY32_PAIRS for i in p}
    assert got["XOR-R1000^A31"] == (969, 33) and got["XOR-R30000^A31"] == (29969, 33)
    assert got["ANDNOT-R1000-A32"][0] == 968 and got["ANDNOT-R30000-A32"][0] == 29968


@pytest.mark.parametrize("opname", list(OPS))
def test_many_key_bitmaps_hold_every_case(oracle, opname):
    """The two bitmaps with case k's operands at key k: the oracle's result has case k's container at key k, and
    the host layout built for the device holds the same containers."""
    cases = tb.cases_of(opname)
    ca, cb = tb.many_key_bitmaps(cases)
    res = oracle.op(OPS[opname], tb.oracle_keyed(oracle, ca), tb.oracle_keyed(oracle, cb))
    got = {k: (t, c) for k, t, c, _ in res.containers()}
    for k, case in enumerate(cases):
        want = oracle_result(oracle, case)
        assert got.get(k, (None, 0)) == (want[1], want[0].cardinality()), case.id
    soa = tb.keyed_soa([ca, cb])
    assert soa.n_bitmaps == 2 and soa.n_containers == 2 * len(cases)
    for b, conts in enumerate((ca, cb)):
        vals = np.concatenate([v.astype(np.uint32) | np.uint32(k << 16) for k, _, v in conts])
        assert np.array_equal(soa.values(b), vals)
        assert [int(t) for t in soa.type[int(soa.begin[b]):int(soa.begin[b + 1])]] == [t for _, t, _ in conts]
    small = tb.cases_of(opname, small_path_only=True)
    assert 100 <= len(small) < len(cases) and all(c.max_operand_runs <= 2048 for c in small)


def test_operand_group_sits_on_the_staging_and_fit_edges(oracle):
    runs = {c.max_operand_runs for c in CASES if c.group == "operand"}
    assert {2047, 2048, 2049, 5000} <= runs
    want = {"run": RUN, "array": ARRAY, "empty": None}
    for ra, rb in tb.FIT_PAIRS:
        for a, b in {(ra, rb), (rb, ra)}:
            for kind, t in want.items():
                case = BY_ID[f"AND-R{a}&R{b}-{kind}"]
                assert oracle_result(oracle, case)[1] == t, case.id
    assert [((ra + 3) & ~3) + rb <= 2048 for ra, rb in tb.FIT_PAIRS] == [True, False, True, False, True]
    assert oracle_result(oracle, BY_ID["AND-R1500&R1500-bitmap"])[1] == BITMAP
