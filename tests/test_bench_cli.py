"""bench.py's command line: a plain run times the steps and prints the headline figures only (everything that takes runs of its own is
behind --full), --steps sets the number of timed steps, and --dump-outputs writes what the last timed step computed, the same from
run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "parity", "roofline", "end_to_end", "ipm_iterations_per_s_end_to_end", "box_probe", "refined_block_solves")


def test_options_are_there():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout, opt


def test_dump_outputs_is_float64_and_bounded(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    big = np.arange(300000, dtype=np.float32)           # 2.4 MB as float64: above its share, sampled
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, {"small": [1, 2, 3], "big": big})
    total = 0
    for d in ("a", "b"):
        for f in os.listdir(tmp_path / d):
            a = np.load(tmp_path / d / f)
            assert a.dtype == np.float64, f
            total += a.nbytes
    assert total <= 2 * (1 << 20)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), [1.0, 2.0, 3.0])
    idx = np.load(tmp_path / "a" / "big_sample_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "big_sample_index.npy"))          # a fixed sample
    assert np.array_equal(np.load(tmp_path / "a" / "big.npy"), big[idx.astype(np.int64)])
    bench.dump_outputs(str(tmp_path / "c"), 1, {"small": [1.0]})
    assert os.path.isfile(tmp_path / "c" / "rank1" / "small.npy")


def _plain_run(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k != "CLARABEL_HIPKKT_TESTING" and not k.startswith("HIPKKT_")}    # the product library
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    line = _plain_run(tmp_path / "a", 3)
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-2 * 1e3      # value = steps / s, ms_per_step = ms / step
    for k in FULL_ONLY:
        assert k not in line, k
    n = line["config"]["N"]
    sols = np.load(tmp_path / "a" / "solutions.npy")
    assert sols.dtype == np.float64 and sols.shape[0] == 3 and sols.shape[1] <= n
    assert np.all(np.isfinite(sols)) and np.max(np.abs(sols)) > 0
    steps = np.load(tmp_path / "a" / "refinement_steps.npy")
    assert steps.shape == (3,) and np.all(steps >= 0)
    # the same arguments: the same inputs, the same outputs
    again = _plain_run(tmp_path / "b", 3)
    assert again["config"] == line["config"]
    for f in ("solutions.npy", "refinement_steps.npy", "regularisation.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
