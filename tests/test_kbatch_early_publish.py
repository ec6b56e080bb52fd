"""KGPU_OPT_BATCH_EARLY_PUBLISH: the helper-wave instantiation of the persistent batch kernel publishes
both variants of a pod (rows as they are; the previous pod assumed on this workgroup's candidate) before
the previous pod resolves, and every reader takes variant B from the slot of the workgroup that won the
pod before and variant A from every other slot.  k_batch_fixup picks the feasible counts the same way.

With the option at 1 and at 0 the kernel must give the C restatement's (oracle/c) placements,
FeasibleNodes, scored flags, scores and final node rows, on the Fit + LeastAllocated +
BalancedAllocation profile, at the sizes where the protocol can go wrong:

 * N = 40: one workgroup, which wins every feasible pod, so variant B is chosen every time;
 * N = 63, 64: per = 63 -- the last row lane holds a node, the lane after it is the spare; at 64 a second
   workgroup holds one node;
 * N = 130: three workgroups, the last one short.

The queues hold runs of pods that fit nowhere (key 0, no winner: the pod after them reads variant A
everywhere) and pods with exactly one feasible node (the fixup's unscored shortcut).  In the "slow"
queue every third pod carries a host port or an extended resource: the pod after it has no variant B,
so the workgroup that may win defers its store to after the resolve and the winner evaluates its row
again, and the pod after that is back on the early path.

The assume = 0 path: kgpu_schedule_one is a diagnostic cycle and never launches the persistent kernel;
the only launches with assume = 0 are the one-pod runs of a cluster that lists a node twice, and in a
one-pod run the kernel reads `assume` only after its single pod was published and resolved.  The
one-pod batch below runs exactly that code."""
import functools

import numpy as np
import pytest

from kgpu import abi, cluster
from kgpu.compile import Profile
from kgpu.framework import GpuFramework

ROW_KEYS = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "num_pods")
FIELDS = ("node", "feasible", "scored", "score")
N_PODS = 300
DEV = "example.com/dev"


def _queue(kind):
    r = np.random.RandomState(20240)
    pods = []
    for i in range(N_PODS):
        if i % 25 in (10, 11, 12):
            p = cluster.pod("p%d" % i, "1000", "1Gi")  # fits nowhere: a run of three
        elif i % 40 == 5:
            p = cluster.pod("p%d" % i, "20", "1Gi")  # the one large node only, while it has room
        else:
            p = cluster.pod("p%d" % i, "%dm" % (100 * (1 + r.randint(15))), "%dMi" % (128 * (1 + r.randint(16))))
        c = p["spec"]["containers"][0]
        if kind in ("slow", "ext") and i % 3 == 1:
            if kind == "slow" and i % 2 == 0:
                c["ports"] = [{"containerPort": 8080, "hostPort": 8000 + i % 5, "protocol": "TCP"}]
            else:
                c.setdefault("resources", {}).setdefault("requests", {})[DEV] = "1"
        pods.append(p)
    return pods


@functools.lru_cache(maxsize=None)
def _case(n_nodes, kind):
    """Framework, compiled queue and the C restatement's records and node rows (computed once)."""
    from oracle.cref import RefEngine
    nodes = [cluster.node("n%d" % i, "64" if i == 7 else "8", "32Gi", 110, "100Gi") for i in range(n_nodes)]
    for i, n in enumerate(nodes):
        if i % 2 == 0:
            n["status"]["allocatable"][DEV] = "4"
            n["status"]["capacity"][DEV] = "4"
    pods = _queue(kind)
    prof = Profile(filters=["NodeResourcesFit"],
                   scores=[("NodeResourcesBalancedAllocation", 1), ("NodeResourcesLeastAllocated", 1)])
    fw = GpuFramework(prof, nodes, [], pods_hint=pods[:16])
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    ref = RefEngine(fw.config, fw.snap, threads=1)
    want, rows = ref.schedule(q, pc), ref.read_nodes()
    # the queue holds what the test is about
    assert (want["node"] < 0).sum() >= 3 and ((want["node"] >= 0) & (want["feasible"] == 1)).sum() >= 1
    return fw, q, pc, want, rows


def _run(fw, q, pc, early, cuts, pipelined=False):
    e = fw.engine
    e.upload(fw.snap, fw.arrays)
    e.set_option(abi.OPT_BATCH_EARLY_PUBLISH, early)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if pipelined:
            e.schedule_batch_submit(q[a:b], pc, first_seq=a)
            if e.pipelined() > 1:
                out.append(e.schedule_batch_wait()[0])
        else:
            out.append(e.schedule_batch(q[a:b], pc, first_seq=a)[0])
            inst = e.instantiation()
            assert inst["helper"] and inst["persistent_pods"] == b - a, inst
    while pipelined and e.pipelined():
        out.append(e.schedule_batch_wait()[0])
    return np.concatenate(out), e.read_nodes(fw.snap.n_nodes)


def _check(want, rows, got, got_rows, what):
    for f in FIELDS:
        np.testing.assert_array_equal(want[f], got[f], err_msg="%s: %s" % (what, f))
    for k in ROW_KEYS:
        np.testing.assert_array_equal(rows[k], got_rows[k], err_msg="%s: %s" % (what, k))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "slow"])
@pytest.mark.parametrize("n_nodes", [40, 63, 64, 130])
def test_early_publish_matches_oracle(n_nodes, kind):
    fw, q, pc, want, rows = _case(n_nodes, kind)
    for early in (1, 0):
        got, got_rows = _run(fw, q, pc, early, [0, N_PODS])
        _check(want, rows, got, got_rows, "N=%d %s early=%d" % (n_nodes, kind, early))


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes", [40, 130])
def test_one_and_two_pod_batches(n_nodes):
    fw, q, pc, want, rows = _case(n_nodes, "slow")
    for early in (1, 0):
        got, got_rows = _run(fw, q, pc, early, [0, 1, 3, 5, 6, N_PODS])
        _check(want, rows, got, got_rows, "N=%d short batches early=%d" % (n_nodes, early))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["slow", "ext"])
def test_submit_wait_three_batches(kind):
    """Three batches through kgpu_schedule_batch_submit / _wait.  The "ext" queue (extended resources, no
    host ports) is carried by the pipeline, whose two slots' granule areas are sized per batch and zeroed
    by the other slot's fixup; the "slow" queue's batches hold host ports and run synchronously inside
    submit.  Option 0 first, so the slot areas grow for option 1."""
    fw, q, pc, want, rows = _case(130, kind)
    for early in (0, 1):
        got, got_rows = _run(fw, q, pc, early, [0, 90, 200, N_PODS], pipelined=True)
        _check(want, rows, got, got_rows, "submit/wait %s early=%d" % (kind, early))
