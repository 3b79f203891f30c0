"""bench.py without --full: the K timed steps and the result line only, and --dump-outputs writes what the last timed step returned --
the same per-locus results as one blocking call on the same seeded batch."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--loci", "400",
           "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "loci/s" and d["unit"] == "loci/s" and d["higher_is_better"] is True and d["dtype"]
    assert d["steps"] == 5 and d["warmup"] == 1 and d["config"]["loci_per_gpu"] == 400
    assert abs(d["value"] - 400 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.02
    for k in ("roofline", "cpu_baseline", "parity", "configs", "e2e", "detail"):
        assert k not in d, k
    spec = importlib.util.spec_from_file_location("bench_plain", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from trgt_amd import locus
    b = bench.make_batch(2, 400, 0)
    want = bench.output_arrays(b, locus.run_batch(b), np.arange(400))
    assert sorted(os.listdir(tmp_path / "out")) == sorted(k + ".npy" for k in want)
    for k, v in want.items():
        got = np.load(tmp_path / "out" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v), k
