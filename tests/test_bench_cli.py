"""bench.py's command line: what a plain run prints and what --dump-outputs writes (helpers on the CPU, one short run on the GPU)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def load_bench():
    spec = importlib.util.spec_from_file_location("_mv_bench", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_sample_index_is_fixed_sorted_and_in_range():
    b = load_bench()
    n = 110_000_000
    i1, i2 = b.dump_sample_index(n), b.dump_sample_index(n)
    assert i1.dtype == np.int64 and len(i1) == b.DUMP_SAMPLE
    assert np.array_equal(i1, i2)
    assert (np.diff(i1) > 0).all() and i1[0] >= 0 and i1[-1] < n
    assert np.array_equal(b.dump_sample_index(1000), np.arange(1000))


def test_dump_outputs_writes_float_arrays_and_refuses_the_rest(tmp_path):
    b = load_bench()
    d = tmp_path / "out"
    names = b.dump_outputs(str(d), {"a": np.arange(6, dtype=np.float32), "b": np.ones((2, 3), dtype=np.float64)})
    assert names == ["a", "b"]
    assert np.array_equal(np.load(d / "a.npy"), np.arange(6, dtype=np.float32))
    assert np.load(d / "b.npy").dtype == np.float64
    with pytest.raises(ValueError):
        b.dump_outputs(str(tmp_path / "int"), {"i": np.arange(3)})
    with pytest.raises(ValueError):
        b.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(b.DUMP_MAX_BYTES // 4 + 1, dtype=np.float32)})
    assert not (tmp_path / "int").exists() and not (tmp_path / "big").exists()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """bench.py without --full: one JSON line with the headline fields and nothing that needs runs of its own; --steps sets the
    number of timed steps; --dump-outputs writes the last step's counters and the parameter sample."""
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=840, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-4000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "pairs/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and abs(out["value"] - 64 / (out["ms_per_step"] / 1e3)) < 1e-6 * out["value"]
    assert "roofline" not in out and "cpu_baseline" not in out and "padded_ms_per_step" not in out["config"]
    stats = np.load(d / "stats.npy")
    p, dp = np.load(d / "params_sample.npy"), np.load(d / "params_change_sample.npy")
    assert stats.dtype == np.float32 and stats.shape == (6,) and stats[4] == 64 and stats[1] > 0
    assert p.dtype == dp.dtype == np.float32 and p.shape == dp.shape
    assert np.isfinite(p).all() and np.isfinite(dp).all() and (dp != 0).any()
    assert sum(f.stat().st_size for f in d.iterdir()) <= 64 << 20
