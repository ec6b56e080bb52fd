"""Delta stream (kgpu_apply_delta, kgpu/cache.py) against the reference cache semantics.

A seeded stream of informer / scheduler events (schedule + assume, confirm, forget, expire, pod
add / update / delete, node add / update / delete, pods on not-yet-known nodes) drives the host
mirror of the scheduler cache.  After every event the mirror syncs the device (UpdateSnapshot) and:

  * CPU: the mirror's list order must equal an independent replay of the node events on the
    oracle's nodeTree (oracle/refsched/nodeinfo.py NodeTreeRef), and the pods it keeps on device
    rows must equal the NodeInfo pod sets of the listed nodes;
  * GPU: a probe pod scheduled on the delta-maintained device mirror must get the placement,
    feasible count and score the Python oracle computes from scratch on the same cluster state,
    and every node row (requested, non-zero requested, pod count) must equal the oracle's NodeInfo.
"""
import copy

import pytest

import gen_random
from delta_stream import Stream
from oracle.refsched import nodeinfo as NI
from kgpu.cache import SchedulerCache
from kgpu.compile import Cluster, Profile


def _cluster(seed, n_nodes):
    nodes, existing, _, services, rss = gen_random.topo_cluster(seed, n_nodes=n_nodes, n_existing=2 * n_nodes,
                                                                n_pods=0)
    return nodes, existing, services, rss


def _tree_replay(events):
    t = NI.NodeTreeRef()
    for ev in events:
        if ev[0] == "add":
            t.add_node(ev[1])
        elif ev[0] == "remove":
            t.remove_node(ev[1])
        else:
            t.update_node(ev[1], ev[2])
    return t


@pytest.mark.parametrize("seed", range(4))
def test_cache_mirror_host_bookkeeping(seed):
    nodes, existing, services, rss = _cluster(seed, 24)
    c = SchedulerCache(Profile(), nodes, existing, cluster=Cluster(services, rss=rss), create_engine=False)
    s = Stream(seed, c, nodes, services, rss, gpu=False)
    tree = _tree_replay(s.node_events)
    want_list = [tree.next() for _ in range(tree.num_nodes)]
    assert c.list == want_list
    for _ in range(120):
        before = len(s.node_events)
        s.step()
        changed = any(ev[0] in ("add", "remove") for ev in s.node_events[before:])
        for ev in s.node_events[before:]:
            if ev[0] == "add":
                tree.add_node(ev[1])
            elif ev[0] == "remove":
                tree.remove_node(ev[1])
            else:
                tree.update_node(ev[1], ev[2])
        c.sync()
        if changed:
            # updateAllLists: the list is the next numNodes outputs of the (stateful) nodeTree
            want_list = [tree.next() for _ in range(tree.num_nodes)]
        assert c.list == want_list
        want_dev = {u: nm for nm in dict.fromkeys(c.list) for u in c.node_pods.get(nm, {})}
        assert c.dev_pods == want_dev


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
def test_delta_stream_matches_oracle(seed):
    nodes, existing, services, rss = _cluster(seed, 40)
    c = SchedulerCache(Profile(), nodes, existing, cluster=Cluster(services, rss=rss))
    try:
        s = Stream(seed, c, nodes, services, rss, gpu=True)
        s.check_rows()
        for _ in range(60):
            s.step()
            c.sync()
            s.check_rows()
            s.schedule_probe(s.fresh_pod())
        assert c.uploads >= 1
    finally:
        c.close()


@pytest.mark.gpu
def test_forget_snapshot_and_assumed_pods():
    """kgpu_forget_pod on batch-assumed pods (one k_delta op) and REMOVE_POD of snapshot pods bring
    the rows back to the oracle's NodeInfos."""
    from kgpu.framework import GpuFramework
    nodes, existing, pods = gen_random.cluster(7, n_nodes=30, n_existing=40, n_pods=20)
    fw = GpuFramework(Profile(), nodes, existing, pods_hint=pods)
    try:
        res = fw.schedule(pods)
        placed = [i for i in range(len(pods)) if res[i]["node"] >= 0]
        assert placed
        slot0 = fw.snap.n_pods
        # forget every other assumed pod
        kept = []
        for k, i in enumerate(placed):
            if k % 2 == 0:
                fw.engine.forget(slot0 + k)
            else:
                p = copy.deepcopy(pods[i])
                p["spec"]["nodeName"] = fw.order[int(res[i]["node"])]
                kept.append(p)
        snap = NI.Snapshot([fw.nodes[nm] for nm in fw.order], list(existing) + kept, order="given")
        rows = fw.engine.read_nodes(len(fw.order))
        for j, ni in enumerate(snap.list):
            assert int(rows["req_cpu"][j]) == ni.requested.milli_cpu
            assert int(rows["num_pods"][j]) == len(ni.pods)
    finally:
        fw.engine.close()


@pytest.mark.gpu
def test_host_ports_beyond_initial_slots():
    """More distinct host-port pods on one node than the snapshot's port slots: every UsedPorts entry
    is kept (the slot table grows), so NodePorts keeps rejecting each taken port."""
    from kgpu.framework import GpuFramework
    node = {"metadata": {"name": "solo", "labels": {"kubernetes.io/hostname": "solo"}}, "spec": {},
            "status": {"allocatable": {"cpu": "64", "memory": "64Gi", "pods": "110"}}}

    def port_pod(i, port):
        return {"metadata": {"name": "pp%d" % i, "namespace": "default", "uid": "pp%d" % i},
                "spec": {"containers": [{"name": "c", "ports": [{"containerPort": 80, "hostPort": port,
                                                                 "protocol": "TCP"}]}]}}

    pods = [port_pod(i, 20000 + i) for i in range(12)] + [port_pod(100 + i, 20000 + i) for i in range(12)]
    fw = GpuFramework(Profile(), [node], [], pods_hint=pods)
    try:
        res = fw.schedule(pods)
        assert all(int(r["node"]) == 0 for r in res[:12])
        assert all(int(r["node"]) == -1 for r in res[12:]), [int(r["node"]) for r in res]
    finally:
        fw.engine.close()
