"""The reference's container-type pins (tests/type_pins.py) through the MI355X path: every pin whose
entry point the device serves (static and/or/xor/andNot, FastAggregation.or, ParallelAggregation.or,
in-place x1.or(x2) (rbgpu_pairwise_inplace), runOptimize (rbgpu_set_run_optimize), bitmapOf
construction) must give the pinned type and the oracle's bytes.  Pins with non-canonical inputs
(32768-value ArrayContainers) run with the canonical form of the same sets.  The pairwise pins run on both pair
paths: as one pair through the small-batch kernel, and with RBGPU_NO_SMALL_PAIRS=1 repeated to more pairs than
the task kernels' grids hold waves, so that the register-path kernel meets the pin with a neighbour behind it."""
import numpy as np
import pytest

from type_pins import PINS, RUN, RUN_ARG_SETS, TYPE_NAME, ab_type, one_container_soa, oracle_bitmap

pytestmark = pytest.mark.gpu
OPS = {"AND": 0, "OR": 1, "XOR": 2, "ANDNOT": 3}
DEVICE_PINS = [p for p in PINS if p.how.split(":")[0] in ("op", "wide", "build", "inplace", "runopt")]
GENERAL_PAIRS = 4096 + 1  # more than the 4096 waves of the copy + filter kernel (the register path's: <= 2048)
PAIR_PATHS = ("small", "general")


def _take_path(monkeypatch, path):
    monkeypatch.setenv("RBGPU_NO_SMALL_PAIRS", "1" if path == "general" else "0")
    monkeypatch.setenv("RBGPU_SMALL_KERNEL_TIMES", "1")  # the small-batch kernel then shows in the call's stats


def _check_pin(out, want, pin, what):
    h = out.download()
    got = out.serialize()
    assert len(got) >= 1
    for i, g in enumerate(got):
        assert g == want, (pin.cite, what, i)
    if pin.expect is not None:
        assert len(h.type) == len(got) and all(int(t) == pin.expect for t in h.type), \
            f"{pin.cite} ({what}): {sorted({TYPE_NAME[int(t)] for t in h.type})} != {TYPE_NAME[pin.expect]}"
    if pin.card is not None:
        assert all(int(c) == pin.card for c in out.cardinalities()), (pin.cite, what)


def test_every_pin_runs_on_the_device():
    assert len(DEVICE_PINS) == len(PINS)


@pytest.mark.parametrize("pin", DEVICE_PINS, ids=[p.name for p in DEVICE_PINS])
def test_type_pin_on_device(ctx, oracle, pin, monkeypatch):
    import roaringbitmap_amd as rb
    kind, _, what = pin.how.partition(":")
    inputs = pin.canonical_inputs()
    if kind in ("op", "inplace"):
        s = ctx.upload_soa(one_container_soa(inputs))
        refs = [oracle_bitmap(oracle, t, v) for t, v in inputs]
        if kind == "op":
            call = ctx.pairwise
            want = oracle.op(OPS[what], refs[0], refs[1]).serialize()
        else:
            call = ctx.pairwise_inplace
            oracle.op_inplace(OPS[what], refs[0], refs[1])
            want = refs[0].serialize()
        for path in PAIR_PATHS:
            _take_path(monkeypatch, path)
            n = 1 if path == "small" else GENERAL_PAIRS
            out = call(OPS[what], s, s, np.zeros(n, np.uint32), np.ones(n, np.uint32))
            st = ctx.stats()
            if path == "small":
                assert [k["name"] for k in st["kernels"]] == ["k_pair_small"], st
            else:
                assert st["tasks"] == n, st["tasks"]
            assert len(out) == n
            _check_pin(out, want, pin, path)
        return
    if kind == "build":
        out = ctx.upload_values([inputs[0][1]])
        want = oracle.RefBitmap.of(inputs[0][1]).serialize()
    elif kind == "runopt":
        s = ctx.upload_soa(one_container_soa(inputs))
        out, any_run = s.run_optimize()
        ref = oracle_bitmap(oracle, *inputs[0])
        assert bool(any_run[0]) == ref.run_optimize(), pin.cite
        want = ref.serialize()
    else:
        s = ctx.upload_soa(one_container_soa(inputs))
        refs = [oracle_bitmap(oracle, t, v) for t, v in inputs]
        out = ctx.wide(getattr(rb, what), s)
        want = oracle.wide(getattr(oracle, what), refs).serialize()
    assert len(out) == 1
    _check_pin(out, want, pin, kind)


@pytest.mark.parametrize("opname", list(OPS))
def test_run_argument_equivalence_on_device(ctx, oracle, opname, monkeypatch):
    """RunContainerArg_Array{AND,ANDNOT,OR,XOR} (TestRunContainer.java:2294-2416) on the device: b_k op
    r_l and b_k op b_l have the same content and each equals the oracle's bytes (Run operands of up to
    32768 runs take the > 8 KiB staging path, which the small-batch kernel refuses: both settings reach the
    general pipeline, the second with every pair repeated)."""
    op = OPS[opname]
    n = len(RUN_ARG_SETS)
    conts = [(RUN, v) for v in RUN_ARG_SETS] + [(ab_type(v), v) for v in RUN_ARG_SETS]
    s = ctx.upload_soa(one_container_soa(conts))
    refs = [oracle_bitmap(oracle, t, v) for t, v in conts]
    a_idx = np.repeat(np.arange(n, 2 * n), n).astype(np.uint32)          # b_k
    b_run = np.tile(np.arange(n), n).astype(np.uint32)                   # r_l
    b_oth = b_run + n                                                    # b_l
    want_r = [oracle.op(op, refs[a_idx[i]], refs[b_run[i]]).serialize() for i in range(n * n)]
    want_o = [oracle.op(op, refs[a_idx[i]], refs[b_oth[i]]).serialize() for i in range(n * n)]
    for path in PAIR_PATHS:
        _take_path(monkeypatch, path)
        rep = 1 if path == "small" else -(-GENERAL_PAIRS // (n * n))
        got_r = ctx.pairwise(op, s, s, np.tile(a_idx, rep), np.tile(b_run, rep))
        tasks_r = ctx.stats()["tasks"]
        got_o = ctx.pairwise(op, s, s, np.tile(a_idx, rep), np.tile(b_oth, rep))
        if path == "general":
            assert rep * n * n >= GENERAL_PAIRS and tasks_r == rep * n * n == ctx.stats()["tasks"]
        br, bo = got_r.serialize(), got_o.serialize()
        assert len(br) == len(bo) == rep * n * n
        for i in range(rep * n * n):  # every copy
            assert br[i] == want_r[i % (n * n)], (opname, path, i)
            assert bo[i] == want_o[i % (n * n)], (opname, path, i)
        hr, ho = got_r.download(0, n * n), got_o.download(0, n * n)
        for i in range(n * n):
            assert np.array_equal(hr.values(i), ho.values(i)), (opname, path, i)
