"""The pod chain of the persistent batch kernel's helper-wave instantiation: its query ring in LDS (four
slots; the prologue stages pods 0..2, the communication wave pod i+3 after it has published pod i, the row
wave and the helper waves read pod i+1 at the top of iteration i) and its traced twin.

Every case is the smallest at which that code can go wrong -- 130 nodes are three workgroups of the
one-row-wave geometry (63 + 63 + 4 nodes) -- and compares `node`, `feasible`, `scored`, `score` and the six
node-row columns with the C restatement (oracle/c), exactly, with KGPU_OPT_BATCH_HELPER 1 and 0."""
import functools

import numpy as np
import pytest

from kgpu import abi, cluster
from kgpu.framework import GpuFramework

ROW_KEYS = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "num_pods")
PER = 63         # nodes per workgroup of the 64 x 1 geometry (the last lane is the spare)
SLOW_SEED = 20   # cluster.fit_least_balanced seed of the `slow` case (test_slow_case_reference_property)


def _pods(name):
    if name == "ties":
        # one workgroup wins every pod: variant B decides every placement
        nodes = [cluster.node("n%d" % i, "16", "64Gi", 110, "100Gi") for i in range(PER)]
        pods = [cluster.pod("p%d" % i, "500m", "1Gi") for i in range(150)]
        return nodes, pods, cluster.fit_least_balanced(n_nodes=1, n_pods=1)[3]
    if name == "slow":
        nodes, _, pods, prof = cluster.fit_least_balanced(n_nodes=130, n_pods=150, seed=SLOW_SEED)
        for i, n in enumerate(nodes):
            if i % 3 == 0:
                n["status"]["allocatable"]["example.com/dev"] = "4"
                n["status"]["capacity"]["example.com/dev"] = "4"
        for i, p in enumerate(pods):
            if i % 5 == 1:
                pods[i] = p = cluster.pod("p%d" % i)  # no requests: KGPU_Q_FIT_ALL_ZERO
            c = p["spec"]["containers"][0]
            if i % 7 == 3:
                c["ports"] = [{"containerPort": 8080, "hostPort": 8000 + i % 5, "protocol": "TCP"}]
            if i % 11 == 5:
                c.setdefault("resources", {}).setdefault("requests", {})["example.com/dev"] = "1"
        return nodes, pods, prof
    nodes, _, pods, prof = cluster.fit_least_balanced(n_nodes=130, n_pods={"ring": 224, "b200": 200, "b300": 300}[name])
    return nodes, pods, prof


@functools.lru_cache(maxsize=None)
def _case(name, engine=True):
    """The case's framework, compiled queries and the reference's records and node rows (computed once)."""
    from oracle.cref import RefEngine
    nodes, pods, prof = _pods(name)
    fw = GpuFramework(prof, nodes, [], pods_hint=pods[:16], create_engine=engine)
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    ref = RefEngine(fw.config, fw.snap, threads=8)
    return fw, q, pc, ref.schedule(q, pc), ref.read_nodes()


def _same(want, got, what):
    for f in ("node", "feasible", "scored", "score"):
        np.testing.assert_array_equal(want[f], got[f], err_msg="%s: %s" % (what, f))


def _run(name, cuts, helper, submit=False, trace=False):
    """The case's pods in consecutive calls (cuts) on a fresh upload; records and rows against the reference."""
    fw, q, pc, want, want_rows = _case(name)
    e = fw.engine
    e.upload(fw.snap, fw.arrays)
    e.set_option(abi.OPT_BATCH_HELPER, helper)
    e.set_option(abi.OPT_PHASE_TRACE, 1 if trace else 0)
    out = []
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            if submit:
                e.schedule_batch_submit(q[a:b], pc, first_seq=a)
            else:
                out.append(e.schedule_batch(q[a:b], pc, first_seq=a)[0])
        while submit and e.pipelined():
            out.append(e.schedule_batch_wait()[0])
        stamps = e.phase_trace(cuts[-1] - cuts[-2] + 1) if trace else None
    finally:
        e.set_option(abi.OPT_PHASE_TRACE, 0)
    got = np.concatenate(out)
    what = "%s helper=%d" % (name, helper)
    _same(want, got, what)
    rows = e.read_nodes(fw.snap.n_nodes)
    for k in ROW_KEYS:
        np.testing.assert_array_equal(want_rows[k], rows[k], err_msg="%s: %s" % (what, k))
    return got, stamps


@pytest.mark.gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_ring_edges(helper):
    """Batches of 1, 2, 3, 4, 5 and 9 pods (a prologue with fewer pods than ring slots, the first wrap),
    then one of 200, on one engine."""
    _run("ring", [0, 1, 3, 6, 10, 15, 24, 224], helper)


@pytest.mark.gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_one_workgroup_wins_every_pod(helper):
    """63 identical nodes, 150 identical pods: every pod after the first takes variant B, so the spare row
    and pod i-1's staged req / nz decide each placement."""
    _run("ties", [0, 150], helper)


def test_slow_case_reference_property():
    """The `slow` case exercises what it is for: in the reference, a slow-path pod (host ports or an
    extended resource) and a bare pod are each followed by a pod placed in the same workgroup."""
    _, q, _, want, _ = _case("slow", engine=False)
    node = want["node"]
    wg = node // PER
    nxt = (node[:-1] >= 0) & (node[1:] >= 0) & (wg[:-1] == wg[1:])
    slow = (q["scalars"]["count"][:-1] | q["ports"]["count"][:-1]) != 0
    bare = (q["flags"][:-1] & abi.Q_FIT_ALL_ZERO) != 0
    assert (nxt & slow).any() and (nxt & bare & ~slow).any()


@pytest.mark.gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_slow_path_through_ring(helper):
    """Host ports every 7th pod, an extended resource every 11th, bare pods every 5th: consecutive pods
    differ in every staged field, and the winning row of a slow-path pod is evaluated again."""
    _run("slow", [0, 150], helper)


@pytest.mark.gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_traced_instantiation(helper):
    """KGPU_OPT_PHASE_TRACE = 1 (the helper-wave instantiation's traced twin): the records of the untraced
    run, and stamps that are non-zero and non-decreasing per workgroup."""
    plain, _ = _run("b200", [0, 200], helper)
    traced, t = _run("b200", [0, 200], helper, trace=True)
    _same(plain, traced, "traced vs untraced helper=%d" % helper)
    assert t.shape == (201, 2, 8)
    for w in range(2):  # workgroup 0 and the last one
        a = t[1:200, w, :]  # iterations with a current and a previous pod
        row = a[:, [0, 5, 1, 2, 4]]  # row wave: start, evaluated, partials, past barrier (c), end
        assert (row > 0).all() and (np.diff(row.reshape(-1)) >= 0).all()
        assert (a[:, 7] > 0).all() and (np.diff(a[:, 7]) >= 0).all()  # communication wave: pod i-1 resolved
        pub = a[:, [6, 3]]  # pod i's partials complete, pod i published
        assert (pub > 0).all() and (np.diff(pub.reshape(-1)) >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_pipelined_steps(helper):
    """Three kgpu_schedule_batch_submit calls of 100 pods, waited in order: the path bench.py times."""
    _run("b300", [0, 100, 200, 300], helper, submit=True)
