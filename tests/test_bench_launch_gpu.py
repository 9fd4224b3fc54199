"""-m gpu: ``python bench.py --gpus N`` launches its own ranks (VERDICT r3 "next" 2).  Two ranks on the one leased GPU over gloo
(``--share-gpu``: a plumbing check, never a measurement): the JSON line must report what the collective library saw."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_gpus_2_launches_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                        "--steps", "2", "--warmup", "1", "--workload", "c1", "--no-cpu-baseline", "--no-roofline"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2
    assert d["config"]["global_batch"] == 4 and d["config"]["parallelism"] == "dp2"
    assert d["backend"] == "gloo" and d["distinct_devices"] == 1
    assert d["value"] > 0 and d["steps"] == 2
    assert d["config"]["deterministic_wgrad"] is False and "dump_outputs" not in d        # a plain run measures the shipped path
    # VERDICT r5 task 7: the N > 1 line says what the gradient exchange did
    dp = d["data_parallel"]
    assert dp["stream"] == "wgrad" and dp["bucket_mb"] == 32 and dp["buckets"] >= 1
    assert dp["buckets_sent_in_backward"] == dp["buckets"] and dp["buckets_sent_by_finish"] == 0
    assert dp["exposed_comm_ms"] is not None and len(dp["exposed_comm_ms_per_rank"]) == 2
    assert d["ms_per_step_rank_min"] <= d["ms_per_step_rank_max"] <= d["ms_per_step"] * 1.0001 + 1e-6


@pytest.mark.gpu
def test_bench_data_parallel_switches_select_the_alternatives():
    """LNN_DP_BUCKET_MB / LNN_DP_STREAM (parallel.py): smaller buckets on the exchange's own stream -- same JSON contract, more buckets,
    every one of them still launched from inside backward."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(LNN_DP_BUCKET_MB="4", LNN_DP_STREAM="own")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                        "--steps", "2", "--warmup", "1", "--workload", "c1", "--no-cpu-baseline", "--no-roofline"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    dp = d["data_parallel"]
    assert dp["stream"] == "own" and dp["bucket_mb"] == 4 and dp["buckets"] == 6          # 22.4 MB arena of the 40x56x40 plan
    assert dp["buckets_sent_in_backward"] == 6 and dp["buckets_sent_by_finish"] == 0 and d["ranks_seen"] == 2


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """``--dump-outputs DIR``: after exactly ``--steps`` timed steps the last one's loss, gradient norm, logits of every
    deep-supervision level and updated parameters are written as float arrays; a second run with the same arguments starts
    from the same inputs and arrives at bit-identical numbers (a dump run uses the ordered weight-gradient reductions)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    runs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--workload", "c1", "--no-cpu-baseline", "--no-roofline", "--no-extras", "--other-workloads", "none",
                            "--dump-outputs", str(tmp_path / name)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dump_outputs"]["step"] == 3 and d["config"]["deterministic_wgrad"]
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["grad_norm.npy", "loss.npy", "output_0.npy", "output_1.npy", "output_2.npy", "params.npy"]
        assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64e6
        arr = {f[:-4]: np.load(tmp_path / name / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arr.values())
        assert arr["output_0"].shape == (2, 3, 40, 56, 40) and arr["output_2"].shape == (2, 3, 10, 14, 10)
        assert abs(float(arr["loss"][0]) - d["config"]["loss"]) <= 1e-6 * abs(d["config"]["loss"])
        runs.append(arr)
    # ordered weight-gradient reductions (no fp32 atomics): two runs are bit-identical
    a, b = runs
    for k in a:
        assert np.array_equal(a[k], b[k]), k


_FULL_ONLY = ("roofline", "regulariser_kernels", "cpu_baseline", "parity", "other_workloads", "value_h2d_inclusive")


@pytest.mark.gpu
def test_bench_plain_run_leaves_the_rest_to_full():
    """A plain run is set-up, warm-up, the timed steps and the line; ``--full`` adds the roofline, the regulariser kernels, the
    loss-fetch and H2D-inclusive repeats and the CPU baseline with its parity gates to the same line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--cpu-sample", "small", "--other-workloads", "none"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--workload", "c1"] + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines[mode] = json.loads(out[0])
    plain, full = lines["plain"], lines["full"]
    for d in (plain, full):
        assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "patches/s"
        assert d["higher_is_better"] is True and d["config"]["deterministic_wgrad"] is False
    assert not [k for k in _FULL_ONLY if k in plain] and "eager_loss_fetch" not in plain["config"]
    assert "h2d_inclusive" not in plain["config"]
    assert all(k in full for k in _FULL_ONLY if k != "other_workloads") and "eager_loss_fetch" in full["config"]
    assert full["roofline"]["slowest_family"] in full["roofline"]["families"]
    assert full["parity"]["gates"]["loss_rel_err<=1e-4"], full["parity"]


def test_bench_other_workloads_need_full():
    """Further configurations are part of ``--full``: asking a plain run for them is an error, not a silent no-op (CPU test)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--other-workloads", "c3"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--full" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_refuses_a_world_that_is_not_gpus():
    """A launcher that exports WORLD_SIZE=1 while asking for 8 GPUs must not record a 1-GPU number as n_gpus 8 (CPU test)."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr and "--gpus 8" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
