"""bench.py on the device: --steps is the number of timed iterations, `ms_per_step` their time over that number, and
--dump-outputs writes what the last of them computed -- the same arrays from run to run with the same arguments (seeded inputs,
seeded initial state, a Philox chain keyed by the iteration)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "bnmf_1024_k16", "--steps", str(steps), "--warmup", "2",
                        "--no-cpu-baseline", "--no-clock", "--dump-outputs", out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_dumps_the_same_outputs_from_run_to_run(tmp_path):
    a, b = _bench(str(tmp_path / "a"), 7), _bench(str(tmp_path / "b"), 7)
    for r in (a, b):
        assert r["steps"] == 7 and r["repeats"]["n"] == 1
        assert r["ms_per_step"] > 0 and abs(r["ms_per_step"] - 1e3 * r["repeats"]["timed_seconds"] / 7) <= 1e-9 * r["ms_per_step"]
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["U.npy", "V.npy", "metrics.npy", "tau.npy"] and sorted(os.listdir(str(tmp_path / "b"))) == names
    for n in names:
        x, y = np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n))
        assert x.dtype == np.float64 and np.array_equal(x, y), n
    U, V, m = (np.load(str(tmp_path / "a" / n)) for n in ("U.npy", "V.npy", "metrics.npy"))
    assert U.shape == (1024, 16) and V.shape == (1024, 16) and np.isfinite(U).all() and (U >= 0).all()
    assert m[0] == a["mse_first_last"][1]          # the MSE of the last timed iteration
