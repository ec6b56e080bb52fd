"""Topology pods under percentageOfNodesToScore below 100 inside ONE persistent launch (k_tbatch's cut-mode
instantiation, KGPU_OPT_CUT_TOPO_PERSISTENT).

The rule is test_percentage.py's: the first to_find feasible nodes in rotated Snapshot.List() order are
kept, p = the rotated position of feasible node to_find + 1 (N if none) is EvaluatedNodes, and
nextStartNodeIndex advances by p.  Under a cut PodTopologySpread, InterPodAffinity, DefaultPodTopologySpread,
NodeAffinity and TaintToleration take their PreScore / NormalizeScore statistics over the KEPT nodes only,
so the small clusters here are built so that the kept set does not see what the feasible set sees: the
"rack" cluster labels blocks of consecutive nodes (a key nodeTree does not interleave) and a window of
to_find feasible nodes covers three or four of its six racks.

The reference is the C restatement (oracle/c) on the compiled queries, compared exactly: node, feasible,
evaluated, scored, score of every pod and all six node-row columns afterwards; the rack cluster is also
held to the Python oracle on the CPU.  Every GPU case asks the engine what it ran (kgpu_debug_geometry,
kgpu_debug_instantiation, the seventh counter of kgpu_debug_counters), so a silent fall-back to the per-pod
topology pipeline fails the case.

Two limits of k_tbatch itself (at any percentage) shape the inputs:
  * a DoNotSchedule constraint on a node-unique key (kubernetes.io/hostname) sends a pod to the per-pod
    pipeline (t_add, kgpu_api.cpp), so the rack pods carry their DoNotSchedule constraint on `pair`, a key
    two neighbouring nodes share; the hostname form is kept as one case that must take the per-pod pipeline
    and still match;
  * the smallest k_tbatch workgroup holds 256 nodes, so the edge pods run on 400 nodes at percentage 50
    (to_find 200, workgroups 0..255 and 256..399) rather than on 200.
Evaluation ahead is off inside a cut-mode run, so there is no KGPU_OPT_TOPO_AHEAD axis."""
import functools
import os
import re

import numpy as np
import pytest

from kgpu import abi, cluster
from kgpu.compile import Cluster, Profile
from kgpu.framework import GpuFramework
from kgpu.native import Engine, KgpuError

import test_percentage as TP
from test_percentage_persistent import _Case, _equal, _sel_pod, _to_find

TGEO = [(256, 1), (512, 1), (512, 2), (512, 4), (512, 8)]
SEL = {"matchLabels": {"app": "web"}}


class _TCase(_Case):
    """_Case with the objects DefaultSelector lists (services, replica sets)."""

    def __init__(self, prof, nodes, existing, pods, calls=None, services=(), rss=()):
        from oracle.cref import RefEngine
        self.fw = GpuFramework(prof, nodes, existing, cluster=Cluster(services=list(services), rss=list(rss)),
                               pods_hint=pods, create_engine=False)
        self.q, self.pc, _, errs = self.fw.compile_pods(pods)
        assert not errs
        self.n = self.fw.snap.n_nodes
        self.calls = calls or [("batch", 0, len(self.q))]
        ref = RefEngine(self.fw.config, self.fw.snap, threads=4)
        self.want = np.concatenate([ref.schedule(self.q[a:b], self.pc, first_seq=a) for a, b in self._spans()])
        self.rows = ref.read_nodes()
        ref.close()
        self.start = np.concatenate([[0], np.cumsum(self.want["evaluated"].astype(np.int64)) % self.n])[:-1]


# ---------------------------------------------------------------- inputs
RACKS, RACK_PODS = 6, 24


def _rack_nodes(n_nodes):
    """rack = i // (N / 6) and no zone label (nodeTree keeps the list order); every third node has 1 CPU;
    the first half of rack 1 carries a PreferNoSchedule taint."""
    per = n_nodes // RACKS
    nodes = []
    for i in range(n_nodes):
        rack = min(i // per, RACKS - 1)
        taints = [{"key": "spot", "value": "true", "effect": "PreferNoSchedule"}] if rack == 1 and i % per < per // 2 else None
        nodes.append(cluster.node("node%d" % i, "1" if i % 3 == 0 else "8", "32Gi", 110, labels={
            "rack": "rack%d" % rack, "pair": "pair%d" % (i // 2), cluster.HOSTNAME: "node%d" % i, "idx": str(i)},
            taints=taints))
    return nodes


def _rack_pod(i, hard_key="pair"):
    """2 CPU; ScheduleAnyway on rack, DoNotSchedule on `hard_key`; every other pod prefers one rack."""
    spec = {"topologySpreadConstraints": [
        {"maxSkew": 1, "topologyKey": "rack", "whenUnsatisfiable": "ScheduleAnyway", "labelSelector": SEL},
        {"maxSkew": 1, "topologyKey": hard_key, "whenUnsatisfiable": "DoNotSchedule", "labelSelector": SEL}]}
    if i % 2 == 1:
        spec["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 10, "preference": {"matchExpressions": [
                {"key": "rack", "operator": "In", "values": ["rack%d" % (i % RACKS)]}]}}]}}
    return cluster.pod("p%d" % i, "2", "1Gi", labels={"app": "web"}, **spec)


@functools.lru_cache(maxsize=None)
def _rack(pct, n_nodes=600, prof="default", tie=0, hard_key="pair", n_pods=RACK_PODS, calls=None):
    p = _PROFILES[prof]()
    p.percentage_of_nodes_to_score = pct
    p.tie_break_mode = tie
    nodes = _rack_nodes(n_nodes)
    pods = [_rack_pod(i, hard_key) for i in range(n_pods)]
    return _TCase(p, nodes, [], pods, calls=list(calls) if calls else None), (nodes, pods)


def _most():
    scores = [s for s in Profile.DEFAULT_SCORES if s[0] != "NodeResourcesLeastAllocated"]
    return Profile(scores=scores + [("NodeResourcesMostAllocated", 1), ("RequestedToCapacityRatio", 2),
                                    ("NodeResourceLimits", 1)])


# name -> profile; the k_tbatch profile row each takes (launch_tbatch): 0 runtime, 1 runtime with Least / Most
# over the default resources, 2 default provider, 3 ClusterAutoscaler provider
_PROFILES = {"least21": lambda: Profile(least_resources=(("cpu", 2), ("memory", 1))), "most": _most,
             "default": Profile, "autoscaler": Profile.cluster_autoscaler}
PROFILE_ROWS = {"least21": 0, "most": 1, "default": 2, "autoscaler": 3}


@functools.lru_cache(maxsize=None)
def _ipa(pct):
    nodes, ex, pods, _, _ = TP._topo_cluster("d")
    return _TCase(Profile(percentage_of_nodes_to_score=pct), nodes, ex, pods)


@functools.lru_cache(maxsize=None)
def _service_case():
    """Pods matched by a Service (DefaultPodTopologySpread live), four zones, matching pods already placed
    unevenly; every third node has 1 CPU; percentage 30 of 400 nodes: to_find 120."""
    nodes = []
    for i in range(400):
        nodes.append(cluster.node("node%d" % i, "1" if i % 3 == 0 else "8", "32Gi", 110,
                                  labels={cluster.ZONE: "zone%d" % (i * 4 // 400), cluster.HOSTNAME: "node%d" % i}))
    existing = [cluster.pod("e%d" % i, "100m", "64Mi", labels={"app": "web"}, node_name="node%d" % ((i * i * 7 + 1) % 400))
                for i in range(60)]
    pods = [cluster.pod("p%d" % i, "2", "1Gi", labels={"app": "web"}) for i in range(20)]
    svc = {"metadata": {"name": "web", "namespace": "default"}, "spec": {"selector": {"app": "web"}}}
    return _TCase(Profile(percentage_of_nodes_to_score=30), nodes, existing, pods, services=[svc])


# geometry index -> (nodes of the rack cluster, percentage): two or three workgroups, the last partly empty
# (4,200 nodes at 66 %: to_find 2,772 of 2,800 feasible, so the first pod's cut falls on node 4,159, among the
# 104 nodes of the second 512 x 8 workgroup)
GEO_CASES = {0: (600, 30), 1: (600, 30), 2: (1500, 30), 3: (2600, 30), 4: (4200, 66)}

EDGE_N, EDGE_PCT, EDGE_WG = 400, 50, 256  # to_find 200; 256 x 1: workgroups 0..255 and 256..399
# name -> ranges of feasible nodes; in batch order, each starting where the previous one left the rotation
# (s = nextStartNodeIndex before the pod)
EDGE_PODS = [
    ("first_of_next", [(0, 199), (256, 256)]),  # s 0: rank 201 = node 256, the first node of workgroup 1, p 256
    ("last_after_wrap", [(256, 399), (0, 55), (255, 255)]),  # s 256: ranks 1-144, 145-200 after the wrap, rank 201 =
                                                # node 255, the last node of workgroup 0, p 399
    ("k_plus_1", [(255, 399), (0, 55)]),        # s 255: exactly 201 feasible, rank 201 = node 55 after the wrap, p 200
    ("exactly_k", [(100, 299)]),                # s 55: 200 feasible, p = N
    ("fewer", [(10, 39)]),                      # 30 feasible, p = N
    ("one", [(77, 77)]),                        # the unscored shortcut, p = N
    ("none", [(900, 1000)]),                    # FitError, s advances by N
    ("last_of_wg", [(55, 255)]),                # s 55: rank 201 = node 255, p 200
    ("after", []),                              # s 255: every node, the window 255..399, 0..54 spans both workgroups, p 200
]


def _edge_nodes():
    return [cluster.node("n%d" % i, "64", "256Gi", 110, labels={"idx": str(i), "blk": "blk%d" % (i // 50)})
            for i in range(EDGE_N)]


def _edge_pod(name, ranges):
    p = _sel_pod(name, *ranges)
    p["metadata"]["labels"] = {"app": "web"}
    p["spec"]["topologySpreadConstraints"] = [
        {"maxSkew": 1, "topologyKey": "blk", "whenUnsatisfiable": "ScheduleAnyway", "labelSelector": SEL}]
    return p


@functools.lru_cache(maxsize=None)
def _edge_case():
    return _TCase(Profile(percentage_of_nodes_to_score=EDGE_PCT), _edge_nodes(), [],
                  [_edge_pod(name, ranges) for name, ranges in EDGE_PODS])


@functools.lru_cache(maxsize=None)
def _nofilter_case():
    """No filter plugins: the first to_find nodes in NON-rotated order, p = to_find (pct 60: 240 of 400)."""
    pods = [_edge_pod("p%d" % i, []) for i in range(10)]
    return _TCase(Profile(filters=[], percentage_of_nodes_to_score=60), _edge_nodes(), [], pods)


SEAM_PODS = 37


@functools.lru_cache(maxsize=None)
def _seam_case():
    """The rack cluster at pct 30 with three kinds of pods in turn: a rack pod (k_tbatch), a plain pod that
    tolerates the PreferNoSchedule taint (k_cbatch), a pod with a preferred node-affinity term and no
    topology state (the per-pod cut pipeline).  Calls: a batch, one kgpu_schedule_one cycle, a batch."""
    pods = []
    for i in range(SEAM_PODS):
        if i % 3 == 0:
            pods.append(_rack_pod(i))
        elif i % 3 == 1:
            pods.append(cluster.pod("p%d" % i, "1500m", "1Gi", tolerations=[
                {"key": "spot", "operator": "Exists", "effect": "PreferNoSchedule"}]))
        else:
            pods.append(cluster.pod("p%d" % i, "1500m", "1Gi", affinity={"nodeAffinity": {
                "preferredDuringSchedulingIgnoredDuringExecution": [{"weight": 5, "preference": {"matchExpressions": [
                    {"key": "rack", "operator": "In", "values": ["rack%d" % (i % RACKS)]}]}}]}}))
    half = SEAM_PODS // 2
    calls = [("batch", 0, half), ("one", half), ("batch", half + 1, SEAM_PODS)]
    return _TCase(Profile(percentage_of_nodes_to_score=30), _rack_nodes(600), [], pods, calls=calls)


def _seam_kinds(lo, hi):
    k = np.arange(lo, hi) % 3
    return int((k == 0).sum()), int((k == 1).sum())


def _split_pods(c, per):
    """Pods whose rotation start and cut position lie in different workgroups of `per` nodes."""
    s = c.start
    p = c.want["evaluated"].astype(np.int64)
    cut = (s + p - 1) % c.n
    return np.nonzero((p < c.n) & (s // per != cut // per))[0]


# ---------------------------------------------------------------- CPU: the generators produce what they list
def test_option_and_counter_are_mirrored():
    assert abi.OPT_CUT_TOPO_PERSISTENT == 25
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "kgpu.h")).read()
    assert re.search(r"#define KGPU_OPT_CUT_TOPO_PERSISTENT 25\b", hdr)


def test_rack_cluster_kept_set_differs_from_feasible_set():
    """From the Python oracle's records and totals at pct 30: the kept nodes are the first to_find feasible
    nodes from the rotation start, they cover strictly fewer racks than the feasible nodes for at least a
    quarter of the pods, a window wraps past node N - 1, and the C restatement agrees on every record."""
    from oracle.refsched import framework as F
    c, (nodes, pods) = _rack(30)
    N, K = 600, _to_find(600, 30)
    assert K == 180
    res = F.schedule_sequence(nodes, [], pods, F.Profile(percentage_of_nodes_to_score=30))
    name_idx = {n["metadata"]["name"]: i for i, n in enumerate(nodes)}
    assert [c.fw.order[i] for i in range(N)] == [n["metadata"]["name"] for n in nodes]  # list order kept
    used = np.zeros(N, np.int64)       # CPUs taken by the pods placed so far
    pairs = np.zeros(N // 2, np.int64)  # matching pods per `pair` domain
    cap = np.array([1 if i % 3 == 0 else 8 for i in range(N)])
    s, fewer, wraps = 0, 0, 0
    for i, r in enumerate(res):
        assert not isinstance(r, (F.FitError, F.ScheduleError))
        feas = np.nonzero((cap - used >= 2) & (pairs[np.arange(N) // 2] + 1 - pairs.min() <= 1))[0]
        assert len(feas) == 400 or i > 0  # 400 of 600 nodes fit the first pod; each placement takes a pair away
        order = np.concatenate([feas[feas >= s], feas[feas < s]])
        kept = order[:K]
        assert sorted(name_idx[n] for n, _ in r.totals) == sorted(kept.tolist()), i
        p = (int(order[K]) - s) % N if len(order) > K else N
        assert (r.feasible, r.evaluated) == (len(kept), p), i
        assert (int(c.want["feasible"][i]), int(c.want["evaluated"][i]), int(c.start[i])) == (len(kept), p, s), i
        assert c.fw.order[int(c.want["node"][i])] == r.host, i
        rk, rf = set((kept * RACKS // N).tolist()), set((feas * RACKS // N).tolist())
        fewer += rk < rf
        wraps += s + p > N
        assert len(rk) in (3, 4) and len(rf) == RACKS, (i, rk)
        w = name_idx[r.host]
        used[w] += 2
        pairs[w // 2] += 1
        s = (s + p) % N
    assert 4 * fewer >= RACK_PODS and wraps >= 1, (fewer, wraps)


def test_inputs_trim_and_split():
    """Every cluster is cut (to_find < feasible for most pods), every pod of the topology cases carries
    topology state the kernel plans, the geometry cases have a pod whose start and cut lie in different
    workgroups, and the edge pods have exactly the stated feasible counts and positions."""
    for pct in (0, 30, 60):
        c, _ = _rack(pct)
        assert (c.want["node"] >= 0).all() and (c.want["evaluated"] < c.n).sum() >= RACK_PODS // 2, pct
    for pct in (0, 40):
        c = _ipa(pct)
        assert (c.want["evaluated"] < c.n).sum() >= 3 and (c.want["node"] >= 0).sum() >= 16, pct  # few pods pass IPA on many nodes
    sv = _service_case()
    assert (sv.q["dpts"]["reqs"]["count"] > 0).all() and (sv.want["evaluated"] < sv.n).all()
    assert (sv.want["feasible"] == _to_find(400, 30)).all()
    for geo, (n, pct) in GEO_CASES.items():
        c, _ = _rack(pct, n_nodes=n)
        per = TGEO[geo][0] * TGEO[geo][1]
        assert 1 < (n + per - 1) // per <= 3 and n % per != 0
        assert len(_split_pods(c, per)) >= 1, geo
    e = _edge_case()
    K, N = _to_find(EDGE_N, EDGE_PCT), EDGE_N
    assert K == 200
    idx = {name: i for i, (name, _) in enumerate(EDGE_PODS)}

    def rec(name):
        i = idx[name]
        return (int(e.start[i]), int(e.want["node"][i]) >= 0, int(e.want["feasible"][i]), int(e.want["evaluated"][i]),
                int(e.want["scored"][i]))

    assert rec("first_of_next") == (0, True, K, EDGE_WG, 1)                  # the cut on node 256
    assert rec("last_after_wrap") == (256, True, K, 399, 1)                  # ... on node 255, after the wrap
    assert rec("k_plus_1") == (255, True, K, 200, 1)                         # 201 feasible, the cut on node 55
    assert rec("exactly_k") == (55, True, K, N, 1)
    assert rec("fewer") == (55, True, 30, N, 1)
    assert rec("one") == (55, True, 1, N, 0) and int(e.want["node"][idx["one"]]) == 77
    assert rec("none") == (55, False, 0, N, 0)
    assert rec("last_of_wg") == (55, True, K, 200, 1)
    assert rec("after") == (255, True, K, 200, 1)
    nf = _nofilter_case()
    Kn = _to_find(EDGE_N, 60)
    assert nf.fw.config.n_filters == 0 and (nf.want["evaluated"] == Kn).all() and (nf.want["feasible"] == Kn).all()
    assert (nf.want["node"] >= 0).all() and (nf.want["node"] < Kn).all() and (nf.start >= Kn).any()
    sm = _seam_case()
    assert (sm.want["node"] >= 0).all() and (sm.want["evaluated"] < sm.n).all()
    assert (sm.q["pref_terms"]["count"] > 0).tolist() == [i % 3 == 2 or (i % 3 == 0 and i % 2 == 1) for i in range(SEAM_PODS)]


# ---------------------------------------------------------------- GPU
def _ran_cut_mode(insts, geos, counters, pods, call=0):
    assert insts[call]["persistent_pods"] == pods, insts
    assert geos[call]["kernel"] == "k_tbatch", geos
    assert counters["cut_topo_persistent_pods"] == pods and counters["cut_persistent_pods"] == 0, counters


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [0, 30, 60])
def test_gpu_rack_cluster_and_twin(pct):
    """Every pod inside one cut-mode launch; option 25 = 0 on a second engine: the per-pod topology
    pipeline, equal in every field and node row."""
    c, _ = _rack(pct)
    got1, rows1, insts1, geos1, cnt1 = c.run_gpu()
    _ran_cut_mode(insts1, geos1, cnt1, RACK_PODS)
    assert cnt1["persistent_launches"] == 1 and insts1[0]["row"] == 2
    _equal(c.want, got1, c.rows, rows1)
    got0, rows0, insts0, geos0, cnt0 = c.run_gpu([(abi.OPT_CUT_TOPO_PERSISTENT, 0)])
    assert insts0[0]["persistent_pods"] == 0 and geos0[0]["kernel"] is None and cnt0["cut_topo_persistent_pods"] == 0
    _equal(got1, got0, rows1, rows0)
    _equal(c.want, got0, c.rows, rows0)


@pytest.mark.gpu
def test_gpu_hostname_do_not_schedule_keeps_the_per_pod_pipeline():
    """A DoNotSchedule constraint on kubernetes.io/hostname is outside k_tbatch at any percentage: those pods
    take the per-pod pipeline under option 25 = 1 too, on the same rotation."""
    c, _ = _rack(30, hard_key=cluster.HOSTNAME)
    got, rows, insts, geos, counters = c.run_gpu()
    assert insts[0]["persistent_pods"] == 0 and counters["cut_topo_persistent_pods"] == 0
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [0, 40])
def test_gpu_pod_affinity_under_a_cut(pct):
    """cluster.pod_affinity(400, 400, 32): InterPodAffinity filter, score and normalize over the kept set."""
    c = _ipa(pct)
    got, rows, insts, geos, counters = c.run_gpu()
    own = sum(1 for i in range(len(c.q)) if i % 16 != 0)  # pods with (anti-)affinity terms of their own
    assert counters["cut_topo_persistent_pods"] >= own, counters
    assert counters["cut_topo_persistent_pods"] + counters["cut_persistent_pods"] == insts[0]["persistent_pods"]
    assert geos[0]["kernel"] is not None
    _equal(c.want, got, c.rows, rows)
    _, _, insts0, _, cnt0 = c.run_gpu([(abi.OPT_CUT_TOPO_PERSISTENT, 0)])
    assert cnt0["cut_topo_persistent_pods"] == 0


@pytest.mark.gpu
def test_gpu_service_zone_sums_over_the_kept_nodes():
    c = _service_case()
    got, rows, insts, geos, counters = c.run_gpu()
    _ran_cut_mode(insts, geos, counters, len(c.q))
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", sorted(GEO_CASES))
def test_gpu_cut_topo_geometry(geo):
    n, pct = GEO_CASES[geo]
    c, _ = _rack(pct, n_nodes=n)
    threads, k = TGEO[geo]
    per = threads * k
    assert len(_split_pods(c, per)) >= 1
    got, rows, insts, geos, counters = c.run_gpu([(abi.OPT_TBATCH_GEO, geo)])
    used = geos[0]
    assert (used["index"], used["threads"], used["rows_per_lane"], used["groups"], used["per"]) == \
        (geo, threads, k, (n + per - 1) // per, per), used
    _ran_cut_mode(insts, geos, counters, RACK_PODS)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_topo_edge_pods():
    c = _edge_case()
    got, rows, insts, geos, counters = c.run_gpu([(abi.OPT_TBATCH_GEO, 0)])
    assert geos[0]["groups"] == 2 and geos[0]["index"] == 0
    _ran_cut_mode(insts, geos, counters, len(c.q))
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_topo_no_filter_profile():
    c = _nofilter_case()
    got, rows, insts, geos, counters = c.run_gpu([(abi.OPT_TBATCH_GEO, 0)])
    assert geos[0]["groups"] == 2
    _ran_cut_mode(insts, geos, counters, len(c.q))
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("prof", sorted(PROFILE_ROWS))
def test_gpu_cut_topo_profile_rows(prof):
    c, _ = _rack(30, prof=prof)
    got, rows, insts, geos, counters = c.run_gpu()
    assert insts[0]["row"] == PROFILE_ROWS[prof] and not insts[0]["sharded"], insts
    _ran_cut_mode(insts, geos, counters, RACK_PODS)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_topo_first_max_tie_mode():
    c, _ = _rack(30, tie=1)
    got, rows, insts, geos, counters = c.run_gpu()
    _ran_cut_mode(insts, geos, counters, RACK_PODS)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_topo_seams():
    """Topology pods (k_tbatch), plain pods (k_cbatch) and pods on the per-pod cut pipeline in turn, then a
    kgpu_schedule_one cycle, then a second batch, on one rotation; each counter counts its own pods."""
    c = _seam_case()
    got, rows, insts, geos, counters = c.run_gpu()
    half = SEAM_PODS // 2
    t0, p0 = _seam_kinds(0, half)
    t1, p1 = _seam_kinds(half + 1, SEAM_PODS)
    assert insts[0]["persistent_pods"] == t0 + p0
    assert insts[1]["persistent_pods"] == 0  # the diagnostic cycle keeps the per-pod pipeline
    assert insts[2]["persistent_pods"] == t1 + p1
    assert counters["cut_topo_persistent_pods"] == t0 + t1 and counters["cut_persistent_pods"] == p0 + p1, counters
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_topo_resident_state():
    """Two consecutive cut batches of one template: the second starts from the resident topology state the
    first wrote back, and equals the run with KGPU_OPT_TOPO_RESIDENT 0."""
    half = RACK_PODS // 2
    c, _ = _rack(30, calls=(("batch", 0, half), ("batch", half, RACK_PODS)))

    def run(options):
        e = Engine(c.fw.config)
        try:
            e.upload(c.fw.snap, c.fw.arrays)
            for opt, v in options:
                e.set_option(opt, v)
            got = [e.schedule_batch(c.q[a:b], c.pc, first_seq=a)[0] for a, b in ((0, half), (half, RACK_PODS))]
            return np.concatenate(got), e.read_nodes(c.n), e.topo_resident(), e.counters()
        finally:
            e.close()

    got1, rows1, res1, cnt1 = run([])
    got0, rows0, res0, cnt0 = run([(abi.OPT_TOPO_RESIDENT, 0)])
    assert res1 == (1, 1) and res0[0] == 0, (res1, res0)
    assert cnt1["cut_topo_persistent_pods"] == RACK_PODS and cnt0["cut_topo_persistent_pods"] == RACK_PODS
    _equal(got1, got0, rows1, rows0)
    _equal(c.want, got1, c.rows, rows1)


@pytest.mark.gpu
def test_gpu_cut_topo_missing_workgroup_retried_cooperatively():
    """KGPU_OPT_HOLD_GROUP on an ordinary launch: the counts round of the run's first pod times out (0.5 s)
    before any pod resolved -- a clean abort; the call is issued again cooperatively, and nextStartNodeIndex
    is as the run found it."""
    c, _ = _rack(30)
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
        e.set_option(abi.OPT_HOLD_GROUP, 1)
        got, _ = e.schedule_batch(c.q, c.pc)
        e.set_option(abi.OPT_HOLD_GROUP, -1)
        cnt = e.counters()
        assert cnt["coop_retries"] == 1 and cnt["coop_launches"] >= 1, cnt
        assert cnt["cut_topo_persistent_pods"] == RACK_PODS and e.instantiation()["persistent_pods"] == RACK_PODS
        assert e.geometry()["kernel"] == "k_tbatch"
        _equal(c.want, got, c.rows, e.read_nodes(c.n))
    finally:
        e.close()


@pytest.mark.gpu
def test_gpu_cut_topo_abort_hook_fails_the_batch_and_recovers():
    """KGPU_OPT_ABORT_AT inside a cut-mode run: KGPU_E_DEVICE, cycles refused until the next upload, then the
    reference's records (an aborted run leaves nextStartNodeIndex as it found it)."""
    c, _ = _rack(30)
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
        e.set_option(abi.OPT_ABORT_AT, 11)
        with pytest.raises(KgpuError) as ex:
            e.schedule_batch(c.q, c.pc)
        assert ex.value.code == abi.E_DEVICE and "re-upload" in str(ex.value)
        e.set_option(abi.OPT_ABORT_AT, -1)
        with pytest.raises(KgpuError):
            e.schedule_batch(c.q[:1], c.pc)
        e.upload(c.fw.snap, c.fw.arrays)
        got, _ = e.schedule_batch(c.q, c.pc)
        assert e.counters()["coop_retries"] == 0 and e.geometry()["kernel"] == "k_tbatch"
        _equal(c.want, got, c.rows, e.read_nodes(c.n))
    finally:
        e.close()
