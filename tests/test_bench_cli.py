"""bench.py's command line: a plain run is the headline alone, --full adds the CPU baselines and the
secondary lines, --dump-outputs writes the last timed step's result the same way every run."""
import json
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.secondary, a.no_cpu_baseline, a.dump_outputs) == \
        (7, 2, False, "none", True, None)
    # what the scripts pass already stays valid
    a = _parse(monkeypatch, "--secondary", "none", "--no-cpu-baseline")
    assert (a.secondary, a.no_cpu_baseline) == ("none", True)


def test_full_run_keeps_todays_defaults(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert (a.secondary, a.no_cpu_baseline) == ("all", False)
    a = _parse(monkeypatch, "--full", "--secondary", "census,wide_or", "--no-cpu-baseline")
    assert (a.secondary, a.no_cpu_baseline) == ("census,wide_or", True)


def test_secondary_lines_need_full(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--secondary", "census")


def test_last_result_keeps_only_the_last_step():
    class R:
        closed = False

        def close(self):
            self.closed = True

    rs = [R() for _ in range(3)]
    last = bench.LastResult(True, 3)
    for r in rs:
        last.done(r)
    assert [r.closed for r in rs] == [True, True, False] and last.r is rs[2]
    rs = [R() for _ in range(3)]
    last = bench.LastResult(False, 3)
    for r in rs:
        last.done(r)
    assert all(r.closed for r in rs) and last.r is None


def test_container_values_decodes_every_container_type():
    from roaringbitmap_amd.engine import soa_from_values
    rng = np.random.default_rng(3)
    v = np.unique(np.concatenate([rng.choice(1 << 16, 100), (1 << 16) + np.arange(50000),
                                  (2 << 16) + rng.choice(1 << 16, 30000), (3 << 16) + np.arange(5, 9),
                                  (3 << 16) + np.arange(100, 3000), [(5 << 16) + 65535]])).astype(np.uint32)
    for run_optimize in (False, True):
        h = soa_from_values([v], run_optimize=run_optimize)
        assert np.array_equal(bench.container_values(h, range(h.n_containers)), v)
        assert np.array_equal(bench.container_values(h, [1, 3]), v[(v >> 16 == 1) | (v >> 16 == 3)])


@pytest.mark.gpu
def test_dump_outputs_is_repeatable_and_is_the_result(ctx, tmp_path, monkeypatch, capsys):
    import roaringbitmap_amd as rb
    npairs, dirs = 3000, [tmp_path / "run0", tmp_path / "run1"]
    for d in dirs:
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                                          "--pairs", str(npairs), "--dump-outputs", str(d)])
        bench.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and len(line["step_ms"]) > 0
        assert "secondary" not in line and "cpu_baseline" not in line
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == sorted(p.name for p in dirs[1].iterdir()) and "cardinalities.npy" in names
    got = {n[:-4]: np.load(dirs[0] / n) for n in names}
    assert sum(x.nbytes for x in got.values()) <= bench.DUMP_MAX_BYTES
    for n in names:
        assert got[n[:-4]].dtype == np.float64
        assert np.array_equal(got[n[:-4]], np.load(dirs[1] / n)), n
    # the same call outside the benchmark
    a, b = ctx.generate(rb.WL_FILTER_POSTING, npairs, seed=42)
    r = ctx.pairwise(rb.AND, a, b)
    assert np.array_equal(got["bitmap_index"], np.arange(npairs))
    assert np.array_equal(got["cardinalities"], r.cardinalities())
    assert np.array_equal(got["serialized_sizes"], r.serialized_sizes())
    assert got["cardinalities"].sum() > 0
    h = r.download()
    sample = got["sample_bitmaps"].astype(np.int64)
    assert len(sample) == bench.DUMP_SAMPLE and len(set(sample)) == len(sample)
    cap = bench.DUMP_VALUES // len(sample)
    cb, vb = got["sample_container_begin"].astype(np.int64), got["sample_value_begin"].astype(np.int64)
    for j, bm in enumerate(sample):
        lo, hi = int(h.begin[bm]), int(h.begin[bm + 1])
        assert hi - lo <= bench.DUMP_VALUE_CONTAINERS
        assert np.array_equal(got["sample_container_keys"][cb[j]:cb[j + 1]], h.key[lo:hi])
        assert np.array_equal(got["sample_container_types"][cb[j]:cb[j + 1]], h.type[lo:hi])
        assert np.array_equal(got["sample_container_cardinalities"][cb[j]:cb[j + 1]], h.card[lo:hi])
        assert np.array_equal(got["sample_values"][vb[j]:vb[j + 1]], h.values(int(bm))[:cap])
    for s in (a, b, r):
        s.close()
