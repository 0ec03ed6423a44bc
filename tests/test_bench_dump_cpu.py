"""bench.py --dump-outputs / --full on CPU with a tiny model: seeded
inputs make two runs with the same arguments write the same outputs,
--steps sets the number of timed steps, and --full still prints the
one result line."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, extra=()):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"),
           "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--layers", "2", "--hidden", "128", "--batch", "4",
           "--seq-len", "64", "--device", "cpu",
           "--dump-outputs", str(out_dir)] + list(extra)
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         env=env, cwd=REPO)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    line = [l for l in out.stdout.splitlines()
            if l.startswith("{") and '"metric"' in l]
    assert len(line) == 1, out.stdout[-2000:]
    return json.loads(line[0])


def test_dump_outputs_reproducible_and_full_accepted(tmp_path):
    rec_a = _run(tmp_path / "a")
    rec_b = _run(tmp_path / "b", ["--full"])
    for rec in (rec_a, rec_b):
        assert rec["steps"] == 3 and rec["warmup"] == 1
        assert rec["ms_per_step"] > 0
        assert rec["metric"] == "samples_per_sec"
    assert sorted(os.listdir(tmp_path / "a")) == ["loss.npy"]
    a = np.load(tmp_path / "a" / "loss.npy")
    b = np.load(tmp_path / "b" / "loss.npy")
    assert a.dtype == np.float32 and a.shape == (1,)
    assert np.isfinite(a).all()
    # same arguments -> same weights and data -> same loss (CPU fp32 is
    # deterministic)
    assert np.array_equal(a, b), (a, b)
