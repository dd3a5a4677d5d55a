"""A plain bench.py run on the GPU (one rank, a small C2 index): it times the
steps asked for and prints the headline line without the --full parts, and
--dump-outputs writes the last timed step's results, which are the oracle's.
A fresh child process, as the bench is run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

STEPS, BATCH, K = 3, 4096, 10


def test_plain_run_dumps_last_step(built, tmp_path):
    from oracle.oracle import OracleVacuum
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "2",
           "--workload", "c2", "--docs", "50000", "--vocab", "50000", "--queries", "20000",
           "--index-dir", str(tmp_path), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["n_gpus"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "u32/f64"
    assert d["full"] is False
    for moved in ("legs", "cpu_baseline", "roofline", "parity_checked_queries", "forms"):
        assert moved not in d, moved
    # value = queries of the timed steps / their wall time; ms_per_step = that time / steps
    # (printed to 1e-4 ms: up to 1 % of a step of some hundredths of a millisecond)
    assert d["value"] == pytest.approx(BATCH / (d["ms_per_step"] * 1e-3), rel=0.02)

    ids = np.load(out / "doc_ids.npy")
    scores = np.load(out / "scores.npy")
    counts = np.load(out / "hit_counts.npy")
    assert ids.dtype == scores.dtype == counts.dtype == np.float64
    assert ids.shape == scores.shape == (BATCH, K) and counts.shape == (BATCH,)
    # step s runs batch s of the log: the last timed step's queries
    idx = tmp_path / "c2_50000_50000"
    log = [l.split() for l in open(idx / "two_term_20000.log").read().splitlines()]
    first = (STEPS - 1) * BATCH
    orc = OracleVacuum(str(idx))
    nonempty = 0
    for i in range(0, BATCH, 16):
        want, _ = orc.search(log[first + i], K)
        n = int(counts[i])
        got = [(int(ids[i, j]), float(scores[i, j])) for j in range(n)]
        assert got == want, (log[first + i], got[:3], want[:3])
        assert (ids[i, n:] == -1).all() and (scores[i, n:] == 0).all()
        nonempty += bool(want)
    orc.close()
    assert nonempty > 0
