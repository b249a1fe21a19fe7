"""bench.py's plain run and --dump-outputs: the plain line carries the headline only (the CPU baseline and the other configurations
are --full's), and what the last timed step computed is written as float64 .npy files that are the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MCMCX_COMM_KEY")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs_are_reproducible(tmp_path):
    n = 20480                                                   # above the dump's sample size: the sample is a seeded subset
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--chains-per-gpu", str(n)]
    outs = []
    for tag in ("a", "b"):
        line = _run(args + ["--dump-outputs", str(tmp_path / tag), "--dump-moments", str(tmp_path / (tag + ".f64"))])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "cpu_baseline" not in line and "other_configs" not in line
        files = sorted(os.listdir(tmp_path / tag))
        assert files == ["chain_ids.npy", "pooled_moments.npy", "scalars.npy", "theta.npy", "totals.npy"], files
        arrs = {f[:-4]: np.load(str(tmp_path / tag / f)) for f in files}
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        ids = arrs["chain_ids"]
        assert 0 < len(ids) < n and np.all(np.diff(ids) > 0) and ids[-1] < n
        assert arrs["theta"].shape == (len(ids), 50) and arrs["scalars"].shape == (len(ids), 4)
        assert np.isfinite(arrs["theta"]).all()
        m = np.fromfile(str(tmp_path / (tag + ".f64")), dtype=np.float64)
        assert np.array_equal(arrs["pooled_moments"].view(np.uint64), m.view(np.uint64)) and m[0] == n
        outs.append(arrs)
    for k in outs[0]:
        assert np.array_equal(outs[0][k].view(np.uint64), outs[1][k].view(np.uint64)), k
