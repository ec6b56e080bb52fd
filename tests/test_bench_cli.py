"""bench.py's plain run, --full and --dump-outputs.

A plain run times its steps and prints the headline record alone; --full adds the records that take
runs of their own; --dump-outputs writes the last timed step's kgpu_result fields, identical from run
to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("node", "feasible", "evaluated", "scored", "score")
TINY = ["--gpus", "1", "--config", "b", "--nodes", "96", "--pods-per-step", "40", "--steps", "3", "--warmup", "1"]
FULL_ONLY = ("roofline", "cpu_baseline", "latency", "compile", "dropin", "extender", "summary")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_dump_outputs_writes_every_result_field(tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    from kgpu import abi
    res = np.zeros(5, abi.RESULT)
    res["node"] = [3, -1, 0, 7, 2]
    res["score"] = [200, 0, 1 << 40, 5, 6]
    out = str(tmp_path / "sub" / "dump")
    bench.dump_outputs(out, res)
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in FIELDS)
    for f in FIELDS:
        a = np.load(os.path.join(out, f + ".npy"))
        assert a.dtype == np.float64 and a.shape == (5,)
        assert np.array_equal(a, res[f].astype(np.float64))


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_repeats(tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    rec = _bench(TINY + ["--dump-outputs", d1])
    assert rec["metric"] == "pods scheduled/sec" and rec["unit"] == "pods/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "int64" and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["config"]["pods"] == 120 and rec["config"]["pods_per_step"] == 40
    assert rec["ms_per_step"] > 0
    # value and ms_per_step state the same elapsed time (ms_per_step is rounded to 1e-4 ms; a step of 40
    # pods takes more than 0.02 ms, so the rounding is below 2.5e-3 of it)
    assert rec["value"] == pytest.approx(40 / (rec["ms_per_step"] / 1e3), rel=5e-3)
    for k in FULL_ONLY + ("extra",):
        assert k not in rec, k
    _bench(TINY + ["--dump-outputs", d2])
    for f in FIELDS:
        a, b = np.load(os.path.join(d1, f + ".npy")), np.load(os.path.join(d2, f + ".npy"))
        assert a.dtype == np.float64 and a.shape == (40,)
        assert np.array_equal(a, b), f
    node = np.load(os.path.join(d1, "node.npy"))
    assert (node >= 0).any() and node.max() < 96


@pytest.mark.gpu
def test_full_run_keeps_every_record(tmp_path):
    rec = _bench(TINY + ["--full", "--cpu-sample", "40", "--latency-pods", "8", "--dropin-pods", "8",
                         "--extender-pods", "3", "--extras", "b:128", "--extra-steps", "2", "--extra-cpu-sample",
                         "40", "--dump-outputs", str(tmp_path / "d")])
    for k in FULL_ONLY:
        assert rec.get(k) is not None, k
    assert rec["roofline"]["kernel"] == "k_batch" and rec["roofline"]["us_per_pod"] > 0
    assert "placements match" in rec["cpu_baseline"]["sample"]
    assert rec["latency"]["pods"] == 8 and rec["dropin"]["pods"] == 8
    assert rec["ms_per_step"] > 0 and rec["steps"] == 3
    # an extra record runs --extra-steps steps, however many the headline runs
    (extra,) = rec["extra"]
    assert extra["series"] == "b:128" and extra["steps"] == 2 and extra["config"]["pods"] == 80
    assert extra["roofline"] is not None and "placements match" in extra["cpu_baseline"]["sample"]
    assert sorted(os.listdir(str(tmp_path / "d"))) == sorted(f + ".npy" for f in FIELDS)


@pytest.mark.parametrize("n_nodes,n_pods,head", [(50, 3000, 1000), (300, 4100, 16), (7, 40, 39)])
def test_config_b_queries_equal_the_object_path(n_nodes, n_pods, head):
    """bench.config_b_queries (the queue past its head compiled by requests) against compiling every
    pod object: the same queries, byte for byte, and the same pools."""
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    from kgpu import cluster
    from kgpu.framework import GpuFramework
    nodes, ex, pods, prof = cluster.fit_least_balanced(n_nodes=n_nodes, n_pods=n_pods)
    want_q, _, want_pools, errs = GpuFramework(prof, nodes, ex, pods_hint=pods[:16],
                                               create_engine=False).compile_pods(pods)
    assert not errs
    fw = GpuFramework(prof, nodes, ex, pods_hint=pods[:16], create_engine=False)
    q, _, pools = bench.config_b_queries(fw, pods[:head], n_nodes, n_pods)
    assert q.dtype == want_q.dtype and q.tobytes() == want_q.tobytes()
    assert sorted(pools) == sorted(want_pools)
    for k in want_pools:
        assert np.asarray(pools[k]).tobytes() == np.asarray(want_pools[k]).tobytes(), k
