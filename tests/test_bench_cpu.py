"""bench.py contract on the CPU plumbing config (BASELINE config 1): one JSON line with the
driver's keys, single process and a 2-rank gloo DDP run (replicas must stay in sync)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _last_json(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def _bench_cpu(dump_dir, *extra):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu", "--steps", "40",
                        "--warmup", "5", "--dump-outputs", str(dump_dir), *extra],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return _last_json(r.stdout)


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    return _bench_cpu(d), d


def test_bench_cpu_single_process_contract(plain_run):
    out, _ = plain_run
    assert KEYS <= set(out) and out["steps"] == 40 and out["warmup"] == 5 and out["value"] > 0
    assert out["config"]["global_batch"] == 4 and out["config"]["parallelism"] == "dp1-cpu-gloo"
    assert out["extra"]["losses_finite"] and out["extra"]["params_in_sync"]
    # a plain run leaves the validation pass to --full
    assert "val_loss" not in out["extra"] and "val_acc" not in out["extra"]


def test_bench_dump_outputs_and_full(plain_run):
    """--dump-outputs writes the timed steps' losses and the state they left as float32 .npy;
    --full adds the validation figures and changes nothing about what the timed steps compute:
    the same arguments give the same arrays, element for element."""
    import numpy as np

    _, d_plain = plain_run
    n_params = 5 * 128 + 128 + 128 * 128 + 128 + 128 * 2 + 2  # weather-mlp-3x128
    sizes = {"loss": 40, "params": n_params, "adam_m": n_params, "adam_v": n_params}
    assert sorted(os.listdir(d_plain)) == sorted(k + ".npy" for k in sizes)
    plain = {k: np.load(os.path.join(d_plain, k + ".npy")) for k in sizes}
    for k, n in sizes.items():
        assert plain[k].dtype == np.float32 and plain[k].shape == (n,) and np.isfinite(plain[k]).all(), k
    assert np.abs(plain["adam_m"]).max() > 0 and (plain["adam_v"] >= 0).all()

    d_full = os.path.join(d_plain, "full")
    out = _bench_cpu(d_full, "--full")
    assert 0 < out["extra"]["val_loss"] < 10 and 0 <= out["extra"]["val_acc"] <= 1
    for k in sizes:
        assert np.array_equal(plain[k], np.load(os.path.join(d_full, k + ".npy"))), k


@pytest.mark.slow
def test_bench_cpu_two_rank_gloo_ddp():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", "--master-port=29661", os.path.join(ROOT, "bench.py"), "--device", "cpu",
           "--gpus", "2", "--steps", "30", "--warmup", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = _last_json(r.stdout)
    assert out["config"]["global_batch"] == 8 and out["config"]["parallelism"] == "dp2-cpu-gloo"
    assert out["extra"]["params_in_sync"] is True
