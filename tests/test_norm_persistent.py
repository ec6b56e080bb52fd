"""Pods that need a normalize pass inside ONE persistent launch (k_nbatch, KGPU_OPT_NORM_PERSISTENT).

NodeAffinity and TaintToleration normalize their raw scores by the maximum over the pod's feasible nodes
(helper.DefaultNormalizeScore); under percentageOfNodesToScore < 100 over the kept nodes.  A pod with a
preferred node-affinity term, or one that does not tolerate a PreferNoSchedule taint of the cluster, needs
those maxima; option 26 sends runs of such pods (without topology state) through k_nbatch, which exchanges
them between the workgroups as one granule per workgroup.

The reference is the C restatement (oracle/c) on the compiled queries.  Every comparison is exact: node,
feasible, evaluated, scored, score of every pod and all six node-row columns afterwards
(test_percentage_persistent._equal).  Every GPU case sets option 26 itself and asks the engine what it ran
(the eighth counter of kgpu_debug_counters, kgpu_debug_instantiation, kgpu_debug_geometry).

The CPU tests assert from the reference alone that the inputs produce what the GPU cases are meant to
exercise: maxima that change mid-run, a kept-set maximum that is not monotonic, a taint whose single node
the kept window decides, and the edge pods."""
import functools
import os
import re

import numpy as np
import pytest

from kgpu import abi, cluster, native
from kgpu.compile import Profile
from kgpu.native import Engine

import test_percentage as TP
import test_percentage_persistent as PP
from test_percentage_persistent import _Case, _equal, _sel_pod, _to_find, GEO, GEO_CASES

TIER_N, TIER_PODS = 200, 30
GOLD = (5, 70, 135, 199)  # one per 63-node workgroup of the 64 x 1 geometry
TIER_SCORES = [("NodeResourcesBalancedAllocation", 1), ("NodeResourcesLeastAllocated", 1), ("NodeAffinity", 3),
               ("TaintToleration", 2)]
TIER_FILTERS = ["NodeResourcesFit", "NodeAffinity", "TaintToleration"]


def _taint(key):
    return {"key": key, "value": "true", "effect": "PreferNoSchedule"}


def _pref(*terms):
    """preferredDuringSchedulingIgnoredDuringExecution: (weight, key, value) terms."""
    return {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
        {"weight": w, "preference": {"matchExpressions": [{"key": k, "operator": "In", "values": [v]}]}}
        for w, k, v in terms]}}


def _tier_nodes(sparse=None, ext=False):
    nodes = []
    for i in range(TIER_N):
        labels = {"idx": str(i)}
        if i in GOLD:
            labels["tier"] = "gold"
        elif i % 10 == 3:
            labels["tier"] = "silver"
        taints = [_taint(k) for k, m in (("spot", 5), ("burst", 20), ("old", 40)) if i % m == 0]
        if sparse is not None and i == sparse:
            taints.append(_taint("rare"))
        n = cluster.node("n%d" % i, "1" if i in GOLD else "64", "256Gi", 110, labels=labels, taints=taints)
        if ext:
            n["status"]["allocatable"]["example.com/dev"] = "4"
            n["status"]["capacity"]["example.com/dev"] = "4"
        nodes.append(n)
    return nodes


def _tier_pods():
    pods = []
    for i in range(TIER_PODS):
        spec = {}
        if i % 6 != 5:
            spec["affinity"] = _pref((80, "tier", "gold"), (20, "tier", "silver"))
        if i % 4 == 3:
            spec["tolerations"] = [{"key": "spot", "operator": "Exists", "effect": "PreferNoSchedule"}]
        pods.append(cluster.pod("t%d" % i, "400m", "64Mi", **spec))
    return pods


def _tier_profile(pct, filters=TIER_FILTERS, scores=TIER_SCORES, tie=0):
    return Profile(filters=list(filters), scores=list(scores), percentage_of_nodes_to_score=pct, tie_break_mode=tie)


@functools.lru_cache(maxsize=None)
def _tier(pct, sparse=None):
    return _Case(_tier_profile(pct), _tier_nodes(sparse), [], _tier_pods())


def _diag_maxima(case):
    """Pod by pod through the reference with diag: (max raw taint, max raw node affinity) over the nodes whose
    status word is 0, and the records."""
    from oracle.cref import RefEngine
    ref = RefEngine(case.fw.config, case.fw.snap, threads=4)
    out, recs = [], []
    for i in range(len(case.q)):
        res, st, raw, _ = ref.schedule(case.q[i:i + 1], case.pc, first_seq=i, diag=True)
        ok = st == 0
        out.append((int(raw[abi.S_TAINT][ok].max()) if ok.any() else 0,
                    int(raw[abi.S_NODE_AFFINITY][ok].max()) if ok.any() else 0))
        recs.append(res)
    ref.close()
    return out, np.concatenate(recs)


def _normalize_pass(case):
    """The pods the engine routes as normalize-pass pods in the tier cluster: burst and old are tolerated by
    nobody, so every pod is one."""
    return np.ones(len(case.q), bool)


# ---------------------------------------------------------------- edge pods: the tier cluster's 30, then these
# (to_find = 100 at pct 50; s = nextStartNodeIndex before the pod).  Every one carries a preferred term.
EDGE_PODS = [
    ("k_plus_1", [(0, 100)], {}),
    ("exactly_k", [(50, 149)], {}),
    ("fewer", [(10, 39)], {}),
    ("one", [(77, 77)], {}),
    ("none", [(500, 600)], {}),
    ("wrapped", [(120, 199), (0, 49)], {}),
    ("to_tail", [(20, 119), (195, 199)], {}),
    ("from_tail", [], {}),
    ("port_a", [], {"host_port": 8080}),
    ("ext_a", [], {"ext": 3}),
    ("port_b", [], {"host_port": 8080}),
    ("ext_b", [], {"ext": 3}),
    ("no_match", [(10, 12), (14, 22)], {"pref": (50, "tier", "gold")}),  # no gold node among them: maximum 0
    ("after", [], {}),
]
EDGE_FILTERS = ["NodeResourcesFit", "NodePorts", "NodeAffinity", "TaintToleration"]


def _edge_pods():
    pods = []
    for name, ranges, kw in EDGE_PODS:
        kw = dict(kw)
        pref = kw.pop("pref", (20, "tier", "silver"))
        p = _sel_pod(name, *ranges, **kw)
        na = p["spec"].setdefault("affinity", {}).setdefault("nodeAffinity", {})
        na.update(_pref(pref)["nodeAffinity"])  # beside the required terms
        pods.append(p)
    return pods


@functools.lru_cache(maxsize=None)
def _edge(pct):
    """The rotation the edge pods are built for starts at 0: they are a batch of their own on the tier nodes."""
    return _Case(_tier_profile(pct, filters=EDGE_FILTERS), _tier_nodes(ext=True), [], _edge_pods())


@functools.lru_cache(maxsize=None)
def _zone_case(n_nodes, pct, tie=0, scores=None, seed=0):
    """TP._cluster (every third node's CPU cut to 1, four zones), every other pod with a preferred zone term."""
    nodes, ex, pods, _, _ = TP._cluster(seed, n_nodes)
    for i, p in enumerate(pods):
        if i % 2 == 1:
            p["spec"]["affinity"] = _pref((10, cluster.ZONE, "zone%d" % (i % 4)))
    prof = Profile(percentage_of_nodes_to_score=pct, tie_break_mode=tie)
    if scores == "autoscaler":
        prof = Profile(percentage_of_nodes_to_score=pct, tie_break_mode=tie,
                       scores=[("NodeResourcesMostAllocated", w) if n == "NodeResourcesLeastAllocated" else (n, w)
                               for n, w in Profile().scores])
    return _Case(prof, nodes, ex, pods)


@functools.lru_cache(maxsize=None)
def _nofilter_case():
    pods = [cluster.pod("p%d" % i, "%dm" % (100 * (1 + i % 7)), "%dMi" % (256 * (1 + i % 5)),
                        affinity=_pref((30, "tier", "gold"), (10, "tier", "silver"))) for i in range(12)]
    prof = _tier_profile(60, filters=(), scores=[("NodeAffinity", 2), ("NodeResourcesLeastAllocated", 1)])
    return _Case(prof, _tier_nodes(), [], pods)


SEAM_PODS = 36


@functools.lru_cache(maxsize=None)
def _seam_case():
    """Constant-maxima and normalize-pass pods alternate; a batch, one kgpu_schedule_one cycle, a batch."""
    nodes, ex, pods, _, _ = TP._cluster(1, 700)
    pods = pods[:SEAM_PODS]
    for i, p in enumerate(pods):
        if i % 2 == 1:
            p["spec"]["affinity"] = _pref((10, cluster.ZONE, "zone%d" % (i % 4)))
    half = SEAM_PODS // 2
    calls = [("batch", 0, half), ("one", half), ("batch", half + 1, SEAM_PODS)]
    return _Case(Profile(percentage_of_nodes_to_score=30), nodes, ex, pods, calls)


def norm_bench_workload(n_nodes, n_pods, pct, every=1):
    """tools/norm_bench.py's workload (imported from the tool, so the test and the tool cannot drift)."""
    import importlib.util
    path = os.path.join(os.path.dirname(__file__), "..", "tools", "norm_bench.py")
    spec = importlib.util.spec_from_file_location("norm_bench", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.workload(n_nodes, n_pods, pct, every)


# ---------------------------------------------------------------- CPU
def test_option_and_counter_are_mirrored():
    assert abi.OPT_NORM_PERSISTENT == 26
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "kgpu.h")).read()
    assert re.search(r"#define KGPU_OPT_NORM_PERSISTENT 26\b", hdr)
    assert "norm_persistent_pods" in native.Engine.counters.__doc__


def test_tier_cluster_at_pct_100_produces_what_it_claims():
    c = _tier(100)
    mx, recs = _diag_maxima(c)
    _equal(c.want, recs, c.rows, c.rows)  # pod by pod with diag is the batch
    terms = np.arange(TIER_PODS) % 6 != 5
    tol = np.arange(TIER_PODS) % 4 == 3
    assert (c.q["pref_terms"]["count"] > 0).tolist() == terms.tolist()
    na = [m[1] for m in mx]
    # the eight gold slots (four 1-CPU nodes, 400m pods: two each) fill: the node that held the maximum leaves
    # the feasible set mid-run
    assert [na[i] for i in range(9) if terms[i]] == [80] * 8 and na[5] == 0
    assert all(na[i] == (20 if terms[i] else 0) for i in range(9, TIER_PODS))
    # spot + burst + old on node 0 (and every 40th): 3 untolerated, 2 with the spot toleration
    assert [m[0] for m in mx] == [2 if t else 3 for t in tol]
    sc = c.want["score"]
    assert (c.want["scored"] == 1).all() and (c.want["feasible"] >= 192).all() and (c.want["evaluated"] == TIER_N).all()
    with_t = [int(sc[i]) for i in range(TIER_PODS) if terms[i]]
    assert with_t[0] == 639 and with_t[7] == 513 and with_t[8] == 698, with_t
    assert sorted(set(with_t[:8]), reverse=True) == [639, 579, 573, 513]
    assert all(int(sc[i]) == 398 for i in range(TIER_PODS) if not terms[i])


def test_tier_cluster_at_pct_50_kept_maximum_is_not_monotonic():
    c = _tier(50)
    assert _to_find(TIER_N, 50) == 100
    mx, recs = _diag_maxima(c)
    _equal(c.want, recs, c.rows, c.rows)
    na = [m[1] for m in mx]
    # at pod 8 the feasible gold node 135 lies beyond the cut; at pod 9 it is inside the kept window again
    assert na[8] == 20 and na[9] == 80 and all(v in (20, 0) for v in na[10:]), na
    assert ((c.want["evaluated"] >= 100) & (c.want["evaluated"] <= 103)).all()
    assert (c.want["feasible"] == 100).all()


SPARSE = 160  # spot + burst + old, and alone the fourth taint: four untolerated where every other node has three at most


def test_sparse_taint_is_decided_by_the_kept_window():
    """One node alone carries a fourth taint: at pct 50 the taint maximum counts it exactly for the pods whose
    kept window holds that node, at pct 100 for every pod."""
    tol = np.arange(TIER_PODS) % 4 == 3
    base = np.where(tol, 2, 3)
    c = _tier(50, sparse=SPARSE)
    t = np.array([m[0] for m in _diag_maxima(c)[0]])
    inside = (SPARSE - c.start) % TIER_N < c.want["evaluated"]
    assert inside.any() and not inside.all()
    assert (t - base == inside.astype(int)).all(), (t, inside)
    c100 = _tier(100, sparse=SPARSE)
    assert (np.array([m[0] for m in _diag_maxima(c100)[0]]) == base + 1).all()


def test_edge_pods_produce_every_listed_condition():
    c = _edge(50)
    K, N = 100, TIER_N
    w, s = c.want, c.start
    idx = {e[0]: i for i, e in enumerate(EDGE_PODS)}

    def rec(n):
        i = idx[n]
        return int(s[i]), int(w["node"][i]), int(w["feasible"][i]), int(w["evaluated"][i]), int(w["scored"][i])

    assert (c.q["pref_terms"]["count"] > 0).all()
    assert rec("k_plus_1")[2:] == (K, 100, 1) and rec("k_plus_1")[0] == 0
    assert rec("exactly_k")[2:] == (K, N, 1)
    assert rec("fewer")[2:] == (30, N, 1)
    assert rec("one")[1:] == (77, 1, N, 0)
    assert rec("none")[1:4] == (-1, 0, N) and int(s[idx["none"] + 1]) == int(s[idx["none"]])
    sw, _, fw_, pw, _ = rec("wrapped")
    assert fw_ == K and pw < N and sw + pw > N
    last_lo = (N - 1) // 63 * 63
    st, _, ft, pt, _ = rec("from_tail")
    assert st >= last_lo and ft == K and pt < N and st + pt > N
    for a, b in (("port_a", "port_b"), ("ext_a", "ext_b")):
        assert rec(a)[1] >= 0 and rec(b)[1] >= 0 and rec(a)[1] != rec(b)[1]
    assert c.q["ports"]["count"][idx["port_a"]] > 0 and c.q["scalars"]["count"][idx["ext_a"]] > 0
    # a preferred term that matches no feasible node: still a normalize-pass pod, maximum 0
    mx, _ = _diag_maxima(c)
    assert mx[idx["no_match"]][1] == 0 and rec("no_match")[2] == 12
    # the same pods at pct 100: every feasible node counted, nothing rotates
    c100 = _edge(100)
    assert (c100.want["evaluated"] == N).all()
    assert int(c100.want["feasible"][idx["k_plus_1"]]) == 101 and int(c100.want["scored"][idx["one"]]) == 0
    assert int(c100.want["node"][idx["none"]]) == -1


def test_geometry_inputs_and_bench_workload():
    for geo, (n, pct, options, groups) in GEO_CASES.items():
        c = _zone_case(n, 30)
        assert (c.q["pref_terms"]["count"] > 0).sum() == len(c.q) // 2
        assert (c.want["node"] >= 0).all()
    fw, q, pc = norm_bench_workload(400, 20, 0)
    assert (q["pref_terms"]["count"] > 0).all()
    assert fw.config.n_filters == 3 and fw.config.n_scores == 4


# ---------------------------------------------------------------- GPU
def _run(case, v, more=()):
    return case.run_gpu([(abi.OPT_NORM_PERSISTENT, v)] + list(more))


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [None, SPARSE])
@pytest.mark.parametrize("pct", [100, 50])
def test_gpu_tier_cluster(pct, sparse):
    c = _tier(pct, sparse)
    got, rows, insts, geos, counters = _run(c, 1, [(abi.OPT_BATCH_GEO, 0)])
    assert geos[0]["index"] == 0 and geos[0]["groups"] == 4 and geos[0]["kernel"] == "k_batch"
    npods = int(_normalize_pass(c).sum())
    assert counters["norm_persistent_pods"] == npods and insts[0]["persistent_pods"] == len(c.q)
    assert counters["cut_persistent_pods"] == 0
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [100, 50])
def test_gpu_tier_cluster_twin(pct):
    c = _tier(pct)
    got1, rows1, _, _, cnt1 = _run(c, 1)
    got0, rows0, insts0, _, cnt0 = _run(c, 0)
    assert cnt1["norm_persistent_pods"] == len(c.q) and cnt0["norm_persistent_pods"] == 0
    assert insts0[0]["persistent_pods"] == 0
    _equal(got1, got0, rows1, rows0)
    _equal(c.want, got0, c.rows, rows0)
    _equal(c.want, got1, c.rows, rows1)


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [30, 100])
def test_gpu_absorb_rule(pct):
    """Every other pod of the 700-node batch has constant maxima.  26 = 8: one run holds all of them (the last
    pod is a normalize-pass pod).  26 = 1: the normalize-pass pods alone, the others through k_batch / k_cbatch.
    26 = 2 absorbs too (the next pod is always a normalize-pass pod)."""
    c = _zone_case(700, pct)
    nrm = c.q["pref_terms"]["count"] > 0
    assert nrm[-1] and not nrm[0]
    n = len(c.q)
    for v, want_norm in ((8, n - 1), (1, int(nrm.sum())), (2, n - 1)):
        got, rows, insts, geos, counters = _run(c, v)
        assert counters["norm_persistent_pods"] == want_norm, (v, counters)
        assert insts[0]["persistent_pods"] == n
        assert counters["cut_persistent_pods"] == (n - want_norm if pct < 100 else 0)
        _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_tier_cluster_with_a_window():
    """26 = 8 on the tier cluster: every pod of the batch inside k_nbatch launches, the counter is the batch length."""
    c = _tier(50)
    got, rows, insts, geos, counters = _run(c, 8)
    assert counters["norm_persistent_pods"] == len(c.q) and insts[0]["persistent_pods"] == len(c.q)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [50, 100])
def test_gpu_edge_pods(pct):
    c = _edge(pct)
    got, rows, insts, geos, counters = _run(c, 1, [(abi.OPT_BATCH_GEO, 0)])
    assert geos[0]["groups"] == 4 and geos[0]["index"] == 0
    assert counters["norm_persistent_pods"] == len(c.q) and insts[0]["persistent_pods"] == len(c.q)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [30, 100])
@pytest.mark.parametrize("geo", sorted(GEO_CASES))
def test_gpu_geometry_matrix(geo, pct):
    n, _, options, groups = GEO_CASES[geo]
    c = _zone_case(n, pct)
    got, rows, insts, geos, counters = _run(c, 1, options)
    threads, k = GEO[geo]
    used = geos[0]
    assert (used["kernel"], used["index"], used["threads"], used["rows_per_lane"], used["groups"], used["per"]) == \
        ("k_batch", geo, threads, k, groups, threads * k - 1), used
    nrm = int((c.q["pref_terms"]["count"] > 0).sum())
    assert counters["norm_persistent_pods"] == nrm and insts[0]["persistent_pods"] == len(c.q)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("row", [0, 2, 3])
def test_gpu_profile_rows(row):
    c = {0: lambda: _tier(50), 2: lambda: _zone_case(700, 30), 3: lambda: _zone_case(700, 30, scores="autoscaler")}[row]()
    got, rows, insts, geos, counters = _run(c, 8)
    assert insts[0]["row"] == row, insts
    assert counters["norm_persistent_pods"] >= len(c.q) - 1
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_no_filter_profile():
    c = _nofilter_case()
    assert c.fw.config.n_filters == 0
    K = _to_find(TIER_N, 60)
    assert (c.want["evaluated"] == K).all() and (c.want["node"] < K).all()  # non-rotated ranks, p = to_find
    got, rows, insts, geos, counters = _run(c, 1)
    assert counters["norm_persistent_pods"] == len(c.q)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_first_max_tie_mode():
    c = _zone_case(700, 30, tie=1)
    got, rows, insts, geos, counters = _run(c, 8)
    assert counters["norm_persistent_pods"] == len(c.q) - 1
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_seams_on_one_rotation():
    c = _seam_case()
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
        e.set_option(abi.OPT_NORM_PERSISTENT, 1)
        got, before = [], {"cut_persistent_pods": 0, "norm_persistent_pods": 0}
        for call in c.calls:
            if call[0] == "batch":
                got.append(e.schedule_batch(c.q[call[1]:call[2]], c.pc, first_seq=call[1])[0])
            else:
                res, _ = e.schedule_one(c.q[call[1]], c.pc, seq=call[1], assume=True)
                one = np.zeros(1, abi.RESULT)
                for f in PP.FIELDS:
                    one[0][f] = res[f]
                got.append(one)
            cnt = e.counters()
            d = {k: cnt[k] - before[k] for k in before}
            before = {k: cnt[k] for k in before}
            pp = e.instantiation()["persistent_pods"]
            assert d["cut_persistent_pods"] + d["norm_persistent_pods"] == pp
            if call[0] == "batch":
                nrm = c.q["pref_terms"]["count"][call[1]:call[2]] > 0
                assert pp == call[2] - call[1] and d["norm_persistent_pods"] == int(nrm.sum())
            else:
                assert pp == 0  # the diagnostic cycle keeps the per-pod pipeline
        _equal(c.want, np.concatenate(got), c.rows, e.read_nodes(c.n))
    finally:
        e.close()


@pytest.mark.gpu
def test_gpu_cooperative_launch():
    c = _zone_case(700, 30)
    got, rows, insts, geos, counters = _run(c, 8, [(abi.OPT_COOPERATIVE, 1)])
    assert counters["coop_launches"] >= 1 and counters["coop_retries"] == 0, counters
    assert counters["norm_persistent_pods"] == len(c.q) - 1
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_abort_hook_fails_the_batch_and_recovers():
    """KGPU_OPT_ABORT_AT inside a k_nbatch run: the kernel returns, the host gets KGPU_E_DEVICE and refuses
    cycles until the next upload; then the reference's records, the rotation untouched."""
    from kgpu.native import KgpuError
    c = _tier(30)  # every pod a normalize-pass pod: the batch is one run, so no earlier run has moved the rotation
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
        e.set_option(abi.OPT_NORM_PERSISTENT, 1)
        e.set_option(abi.OPT_ABORT_AT, 17)
        with pytest.raises(KgpuError) as ex:
            e.schedule_batch(c.q, c.pc)
        assert ex.value.code == abi.E_DEVICE and "re-upload" in str(ex.value)
        e.set_option(abi.OPT_ABORT_AT, -1)
        with pytest.raises(KgpuError):
            e.schedule_batch(c.q[:1], c.pc)
        e.upload(c.fw.snap, c.fw.arrays)
        got, _ = e.schedule_batch(c.q, c.pc)
        assert e.counters()["coop_retries"] == 0
        _equal(c.want, got, c.rows, e.read_nodes(c.n))
    finally:
        e.close()


@pytest.mark.gpu
def test_gpu_missing_workgroup_is_a_clean_abort():
    """KGPU_OPT_HOLD_GROUP on an ordinary launch: the first exchange of the run's first pod times out before
    any pod resolved; the call is issued again cooperatively and counts its pods once."""
    c = _tier(30)
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
        e.set_option(abi.OPT_NORM_PERSISTENT, 1)
        e.set_option(abi.OPT_BATCH_GEO, 0)
        e.set_option(abi.OPT_HOLD_GROUP, 1)
        got, _ = e.schedule_batch(c.q, c.pc)
        e.set_option(abi.OPT_HOLD_GROUP, -1)
        cnt = e.counters()
        assert cnt["coop_retries"] == 1 and cnt["coop_launches"] >= 1, cnt
        assert cnt["norm_persistent_pods"] == len(c.q) and e.instantiation()["persistent_pods"] == len(c.q)
        _equal(c.want, got, c.rows, e.read_nodes(c.n))
        # the mirror stays valid: the next call needs no upload
        e.schedule_batch(c.q[:1], c.pc, first_seq=len(c.q))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [0, 100])
def test_gpu_full_size(pct):
    """5,000 nodes, 300 pods of norm_bench's workload (pct 0: to_find 500), every pod inside k_nbatch."""
    from oracle.cref import RefEngine
    fw, q, pc = norm_bench_workload(5000, 300, pct)
    ref = RefEngine(fw.config, fw.snap, threads=8)
    want = ref.schedule(q, pc)
    want_rows = ref.read_nodes()
    ref.close()
    e = Engine(fw.config)
    try:
        e.upload(fw.snap, fw.arrays)
        e.set_option(abi.OPT_NORM_PERSISTENT, 1)
        got, _ = e.schedule_batch(q, pc)
        assert e.counters()["norm_persistent_pods"] == 300 and e.instantiation()["persistent_pods"] == 300
        _equal(want, got, want_rows, e.read_nodes(fw.snap.n_nodes))
        if pct == 0:
            assert (got["feasible"][got["node"] >= 0] <= 500).all()
    finally:
        e.close()
