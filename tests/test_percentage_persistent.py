"""percentageOfNodesToScore below 100 inside ONE persistent launch (k_cbatch, KGPU_OPT_CUT_PERSISTENT).

The rule is test_percentage.py's: the first to_find feasible nodes in rotated Snapshot.List() order are
kept, p = the rotated position of feasible node to_find + 1 (N if none) is EvaluatedNodes, and
nextStartNodeIndex advances by p; a profile without filters keeps the first to_find nodes in
NON-rotated order and p = to_find.  The reference is the C restatement (oracle/c) on the compiled
queries; the two smallest clusters are also held to the Python oracle.  Every comparison is exact:
node, feasible, evaluated, scored, score of every pod and all six node-row columns afterwards.

Each GPU case also asks the engine what it ran (kgpu_debug_geometry, kgpu_debug_instantiation and the
sixth counter of kgpu_debug_counters: pods resolved inside cut-mode persistent launches): a silent
fall-back to the per-pod cut pipeline fails the case.  Every geometry of the table is expected to run
persistently (GEO_CASES names them).

The edge pods (EDGE_*) and the seam batch are built by construction; the CPU test runs the reference on
them and asserts from its feasible / evaluated columns and the start positions they imply that every
listed condition occurs."""
import functools

import numpy as np
import pytest

from kgpu import abi, cluster, native
from kgpu.compile import Cluster, Profile
from kgpu.framework import GpuFramework
from kgpu.native import Engine

import test_percentage as TP

ROW_KEYS = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "num_pods")
FIELDS = ("node", "feasible", "evaluated", "scored", "score")
GEO = [(64, 1), (128, 1), (192, 1), (448, 1), (960, 1), (512, 4), (512, 8)]


def _fit_profile(pct, filters=("NodeResourcesFit",)):
    return Profile(filters=list(filters), scores=[("NodeResourcesBalancedAllocation", 1), ("NodeResourcesLeastAllocated", 1)],
                   percentage_of_nodes_to_score=pct)


class _Case:
    """One cluster, one profile, a sequence of calls: ("batch", lo, hi) or ("one", k).  Compiled once,
    scheduled once by the C restatement; GPU cases leave it unchanged."""

    def __init__(self, prof, nodes, existing, pods, calls=None):
        from oracle.cref import RefEngine
        self.fw = GpuFramework(prof, nodes, existing, cluster=Cluster(services=[], rss=[]), pods_hint=pods,
                               create_engine=False)
        self.q, self.pc, _, errs = self.fw.compile_pods(pods)
        assert not errs
        self.n = self.fw.snap.n_nodes
        self.calls = calls or [("batch", 0, len(self.q))]
        ref = RefEngine(self.fw.config, self.fw.snap, threads=4)
        self.want = np.concatenate([ref.schedule(self.q[a:b], self.pc, first_seq=a) for a, b in self._spans()])
        self.rows = ref.read_nodes()
        ref.close()
        # nextStartNodeIndex before every pod, as the evaluated column implies
        self.start = np.concatenate([[0], np.cumsum(self.want["evaluated"].astype(np.int64)) % self.n])[:-1]

    def _spans(self):
        return [(c[1], c[2]) if c[0] == "batch" else (c[1], c[1] + 1) for c in self.calls]

    def run_gpu(self, options=()):
        """The same calls on a fresh engine: (records, node rows, per-call instantiation, geometry, counters)."""
        e = Engine(self.fw.config)
        try:
            e.upload(self.fw.snap, self.fw.arrays)
            for opt, v in options:
                e.set_option(opt, v)
            got, insts, geos = [], [], []
            for c in self.calls:
                if c[0] == "batch":
                    got.append(e.schedule_batch(self.q[c[1]:c[2]], self.pc, first_seq=c[1])[0])
                else:
                    res, _ = e.schedule_one(self.q[c[1]], self.pc, seq=c[1], assume=True)
                    one = np.zeros(1, abi.RESULT)
                    for f in FIELDS:
                        one[0][f] = res[f]
                    got.append(one)
                insts.append(e.instantiation())
                geos.append(e.geometry())
            return np.concatenate(got), e.read_nodes(self.n), insts, geos, e.counters()
        finally:
            e.close()


def _equal(want, got, want_rows, got_rows):
    for f in FIELDS:
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, "%s differs at pods %s: want %s got %s" % (f, bad[:5], want[f][bad[:5]], got[f][bad[:5]])
    for k in ROW_KEYS:
        np.testing.assert_array_equal(want_rows[k], got_rows[k], err_msg=k)


def _to_find(n, pct):
    """numFeasibleNodesToFind (generic_scheduler.go:379-399)."""
    if n < 100 or pct >= 100:
        return n
    if pct <= 0:
        pct = max(50 - n // 125, 5)
    return max(n * pct // 100, 100)


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _c700(pct, tie=0, n_nodes=700):
    """test_percentage._cluster: every third node's CPU cut to 1, the default profile."""
    nodes, ex, pods, _, _ = TP._cluster(0, n_nodes)
    return _Case(Profile(percentage_of_nodes_to_score=pct, tie_break_mode=tie), nodes, ex, pods), (nodes, ex, pods)


@functools.lru_cache(maxsize=None)
def _fit_case(n_nodes, pct, n_pods=40):
    nodes, ex, pods, _ = cluster.fit_least_balanced(n_nodes=n_nodes, n_pods=n_pods, seed=3)
    for i, n in enumerate(nodes):
        if i % 3 == 0:
            n["status"]["allocatable"]["cpu"] = "1"
    return _Case(_fit_profile(pct), nodes, ex, pods)


EDGE_N, EDGE_PCT = 200, 50  # to_find = 100; 64 x 1: workgroups of 63 nodes, the last holds 189..199


def _edge_nodes():
    return [cluster.node("n%d" % i, "64", "256Gi", 110, labels={"idx": str(i)}) for i in range(EDGE_N)]


def _sel_pod(name, *ranges, **kw):
    """A small pod feasible exactly on the nodes whose index lies in one of the inclusive `ranges`
    (required node affinity over the numeric label idx); no range: every node."""
    spec = {}
    if ranges:
        terms = [{"matchExpressions": ([{"key": "idx", "operator": "Gt", "values": [str(a - 1)]}] if a > 0 else []) +
                  [{"key": "idx", "operator": "Lt", "values": [str(b + 1)]}]} for a, b in ranges]
        spec["affinity"] = {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": terms}}}
    p = cluster.pod(name, "10m", "16Mi", **spec)
    c = p["spec"]["containers"][0]
    if kw.get("host_port"):
        c["ports"] = [{"containerPort": 80, "hostPort": kw["host_port"], "protocol": "TCP"}]
    if kw.get("ext"):
        c["resources"]["requests"]["example.com/dev"] = str(kw["ext"])
    return p


# name -> (ranges, extras); in batch order, each starting where the previous one left the rotation
# (to_find = 100; s = nextStartNodeIndex before the pod):
EDGE_PODS = [
    ("k_plus_1", [(0, 100)], {}),             # s 0: 101 feasible, rank 101 = node 100, p 100
    ("exactly_k", [(50, 149)], {}),           # s 100: 100 feasible, p = N
    ("fewer", [(10, 39)], {}),                # s 100: 30 feasible, p = N
    ("one", [(77, 77)], {}),                  # s 100: the unscored shortcut, p = N
    ("none", [(500, 600)], {}),               # s 100: FitError, s advances by N
    ("wrapped", [(120, 199), (0, 49)], {}),   # s 100: ranks 1-80 at 120..199, rank 101 = node 20 < s, p 120
    ("to_tail", [(20, 119), (195, 199)], {}), # s 20: rank 101 = node 195, p 175
    ("from_tail", [], {}),                    # s 195, inside the last workgroup: every node, p 100
    ("port_a", [], {"host_port": 8080}),      # the slow path: a host port ...
    ("ext_a", [], {"ext": 3}),                # ... and an extended resource
    ("port_b", [], {"host_port": 8080}),      # the node port_a took is now infeasible
    ("ext_b", [], {"ext": 3}),                # a node holds 4: the one ext_a took is infeasible
    ("after", [], {}),
]


@functools.lru_cache(maxsize=None)
def _edge_case():
    nodes = _edge_nodes()
    for n in nodes:
        n["status"]["allocatable"]["example.com/dev"] = "4"
        n["status"]["capacity"]["example.com/dev"] = "4"
    pods = [_sel_pod(name, *ranges, **kw) for name, ranges, kw in EDGE_PODS]
    prof = _fit_profile(EDGE_PCT, filters=("NodeResourcesFit", "NodePorts", "NodeAffinity"))
    return _Case(prof, nodes, [], pods), (nodes, pods, prof)


@functools.lru_cache(maxsize=None)
def _nofilter_case():
    """No filter plugins: the first to_find nodes in NON-rotated order, p = to_find (pct 60: 120 of 200,
    so the start wraps 0, 120, 40, 160, 80, 0 while the kept set stays nodes 0..119)."""
    pods = [cluster.pod("p%d" % i, "%dm" % (100 * (1 + i % 7)), "%dMi" % (256 * (1 + i % 5))) for i in range(12)]
    return _Case(_fit_profile(60, filters=()), _edge_nodes(), [], pods)


SEAM_PODS = 36


@functools.lru_cache(maxsize=None)
def _seam_case():
    """The default profile on 700 nodes at pct 30; every other pod carries a preferred node-affinity
    term (a normalize pass: the per-pod cut pipeline), and a fifth of the nodes a PreferNoSchedule taint
    that only the pods named t* do not tolerate.  Calls: a batch, one kgpu_schedule_one cycle, a batch."""
    nodes, ex, pods, _, _ = TP._cluster(1, 700)
    pods = pods[:SEAM_PODS]
    for i, p in enumerate(pods):
        if i % 2 == 1:
            p["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                {"weight": 10, "preference": {"matchExpressions": [
                    {"key": cluster.ZONE, "operator": "In", "values": ["zone%d" % (i % 4)]}]}}]}}
    half = SEAM_PODS // 2
    calls = [("batch", 0, half), ("one", half), ("batch", half + 1, SEAM_PODS)]
    return _Case(Profile(percentage_of_nodes_to_score=30), nodes, ex, pods, calls)


@functools.lru_cache(maxsize=None)
def _taint_seam_case():
    """A PreferNoSchedule taint present: the pods that tolerate it stay persistent-eligible, the others
    take the normalize pass."""
    nodes, ex, pods, _, _ = TP._cluster(2, 400)
    for i, n in enumerate(nodes):
        if i % 5 == 0:
            n["spec"]["taints"] = [{"key": "spot", "value": "true", "effect": "PreferNoSchedule"}]
    pods = pods[:24]
    for i, p in enumerate(pods):
        if i % 3 != 0:
            p["spec"]["tolerations"] = [{"key": "spot", "operator": "Exists", "effect": "PreferNoSchedule"}]
    return _Case(Profile(percentage_of_nodes_to_score=40), nodes, ex, pods)


def _seam_eligible(case):
    return case.q["pref_terms"]["count"] == 0


# ---------------------------------------------------------------- CPU: the generators produce what they list
def test_generators_produce_every_listed_condition():
    c, _ = _edge_case()
    K, N = _to_find(EDGE_N, EDGE_PCT), EDGE_N
    assert K == 100
    w, s = c.want, c.start
    names = [e[0] for e in EDGE_PODS]
    idx = {n: i for i, n in enumerate(names)}
    last_lo = (N - 1) // 63 * 63  # first node of the last, partly filled workgroup of the 64 x 1 geometry
    assert N - last_lo < 63

    def rec(n):
        i = idx[n]
        return int(s[i]), int(w["node"][i]), int(w["feasible"][i]), int(w["evaluated"][i]), int(w["scored"][i])

    # exactly K + 1 feasible: capped at K, and the cut falls on the last of them
    assert rec("k_plus_1") == (0, rec("k_plus_1")[1], K, 100, 1)
    # exactly K (p = N), fewer than K, one (unscored), none (FitError; s still advances by N)
    assert rec("exactly_k")[2:] == (K, N, 1)
    assert rec("fewer")[2:] == (30, N, 1)
    assert rec("one")[1:] == (77, 1, N, 0)
    assert rec("none")[1:4] == (-1, 0, N) and int(s[idx["none"] + 1]) == int(s[idx["none"]])
    # rank K + 1 lies before s, in the wrapped part: s + p > N
    sw, _, fw_, pw, _ = rec("wrapped")
    assert fw_ == K and pw < N and sw + pw > N and (sw + pw) % N < sw
    # a start inside the last, partly filled workgroup, with a cut that wraps into the first
    st, _, ft, pt, _ = rec("from_tail")
    assert st >= last_lo and ft == K and pt < N and st + pt > N
    # the slow path: host ports and extended resources, each followed by a pod its assume excludes
    for a, b in (("port_a", "port_b"), ("ext_a", "ext_b")):
        assert rec(a)[1] >= 0 and rec(b)[1] >= 0 and rec(a)[2] == K and rec(b)[2] == K
    assert c.q["ports"]["count"][idx["port_a"]] > 0 and c.q["scalars"]["count"][idx["ext_a"]] > 0
    assert (w["node"][[idx[n] for n in names if n != "none"]] >= 0).all()
    # the start, the cut and the wrap of one pod fall in different workgroups
    assert len({sw // 63, ((sw + pw) % N) // 63, (N - 1) // 63}) == 3

    # no filter plugins: non-rotated, p = K, while the start keeps rotating
    nf = _nofilter_case()
    Kn = _to_find(EDGE_N, 60)
    assert nf.fw.config.n_filters == 0
    assert (nf.want["evaluated"] == Kn).all() and (nf.want["feasible"] == Kn).all()
    assert (nf.want["node"] >= 0).all() and (nf.want["node"] < Kn).all()
    assert len(set(nf.start.tolist())) >= 4 and (nf.start >= Kn).any()

    # seams: both kinds of pods, interleaved, in both batches; the pods with a normalize pass score
    sm = _seam_case()
    el = _seam_eligible(sm)
    assert el[0::2].all() and not el[1::2].any()
    assert (sm.want["node"] >= 0).all() and (sm.want["evaluated"] < sm.n).any()
    assert len(set(sm.start.tolist())) > SEAM_PODS // 2
    ts = _taint_seam_case()
    assert (ts.want["node"] >= 0).all() and len(set(ts.start.tolist())) > 12


def test_small_clusters_match_the_python_oracle():
    """The two smallest clusters (the edge pods and the no-filter batch) against oracle.refsched."""
    from oracle.refsched import framework as F
    c, (nodes, pods, prof) = _edge_case()
    oprof = F.Profile(filters=prof.filters, prefilters=["NodeResourcesFit", "NodePorts"], prescores=[],
                      scores=prof.scores, percentage_of_nodes_to_score=EDGE_PCT)
    _cmp_oracle(c, TP.oracle_run(nodes, [], pods, [], [], EDGE_PCT, profile=oprof))
    nf = _nofilter_case()
    nprof = F.Profile(filters=[], prefilters=[], prescores=[], scores=nf.fw.profile.scores, percentage_of_nodes_to_score=60)
    nf_pods = [cluster.pod("p%d" % i, "%dm" % (100 * (1 + i % 7)), "%dMi" % (256 * (1 + i % 5))) for i in range(12)]
    _cmp_oracle(nf, TP.oracle_run(_edge_nodes(), [], nf_pods, [], [], 60, profile=nprof))


def _cmp_oracle(c, want):
    got = []
    for r in c.want:
        got.append((None, 0, None, None) if r["node"] == -1 else
                   (c.fw.order[r["node"]], int(r["feasible"]), int(r["score"]) if r["scored"] else None, int(r["evaluated"])))
    TP._cmp(want, got)


def test_option_and_counter_are_mirrored():
    assert abi.OPT_CUT_PERSISTENT == 24
    import re
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "kgpu.h")).read()
    assert re.search(r"#define KGPU_OPT_CUT_PERSISTENT 24\b", hdr)


# ---------------------------------------------------------------- GPU
def _all_persistent(case, insts, counters, pods):
    assert insts[-1]["persistent_pods"] == pods, insts
    assert counters["cut_persistent_pods"] == pods, counters
    assert counters["persistent_launches"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [0, 30, 60])
def test_gpu_cut_batch_runs_persistently(pct):
    """700 nodes, every third node's CPU cut to 1, 40 pods: all of them inside one cut-mode launch."""
    c, _ = _c700(pct)
    got, rows, insts, geos, counters = c.run_gpu()
    assert insts[0]["persistent_pods"] == 40
    assert geos[0]["kernel"] is not None
    assert counters["cut_persistent_pods"] == 40
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [0, 30, 60])
def test_gpu_cut_batch_twin(pct):
    """Option 24 = 0 on a second engine: the per-pod cut pipeline, equal in every field and node row."""
    c, _ = _c700(pct)
    got1, rows1, insts1, _, cnt1 = c.run_gpu()
    got0, rows0, insts0, geos0, cnt0 = c.run_gpu([(abi.OPT_CUT_PERSISTENT, 0)])
    assert insts1[0]["persistent_pods"] == 40 and cnt1["cut_persistent_pods"] == 40
    assert insts0[0]["persistent_pods"] == 0 and geos0[0]["kernel"] is None and cnt0["cut_persistent_pods"] == 0
    _equal(got1, got0, rows1, rows0)
    _equal(c.want, got0, c.rows, rows0)


# geometry index -> (nodes, pct, options, workgroups): every geometry of the table runs persistently
GEO_CASES = {
    0: (200, 50, [(abi.OPT_BATCH_GEO, 0)], 4),   # to_find 100: start, cut and wrap in different workgroups
    1: (700, 30, [(abi.OPT_BATCH_GEO, 1)], 6),
    2: (700, 30, [(abi.OPT_BATCH_GEO, 2)], 4),
    3: (700, 30, [(abi.OPT_BATCH_GEO, 3)], 2),
    4: (700, 30, [(abi.OPT_BATCH_GEO, 4)], 1),
    5: (2100, 30, [(abi.OPT_BATCH_GEO, 5)], 2),  # 512 x 4, resident: 2,047 nodes per workgroup
    6: (4100, 30, [(abi.OPT_PERSIST_GROUPS, 2)], 2),  # 512 x 8, streamed: 4,095 nodes per workgroup
}


def test_geometry_cases_are_what_the_engine_picks():
    for geo, (n, pct, options, groups) in GEO_CASES.items():
        opt = dict(options)
        g = native.geometry_for(native.KERNEL_BATCH, n, opt.get(abi.OPT_PERSIST_GROUPS, 256), opt.get(abi.OPT_BATCH_GEO, 0))
        threads, rows = GEO[geo]
        assert (g["index"], g["threads"], g["rows_per_lane"], g["groups"], g["per"]) == \
            (geo, threads, rows, groups, threads * rows - 1), (geo, g)
        assert _to_find(n, pct) < n
    # just above one workgroup's capacity at the streamed geometry
    assert GEO_CASES[6][0] > 4095 and GEO_CASES[6][0] - 4095 < 64


@pytest.mark.gpu
@pytest.mark.parametrize("geo", sorted(GEO_CASES))
def test_gpu_cut_geometry_matrix(geo):
    n, pct, options, groups = GEO_CASES[geo]
    c = _fit_case(n, pct)
    got, rows, insts, geos, counters = c.run_gpu(options)
    threads, k = GEO[geo]
    used = geos[0]
    assert (used["kernel"], used["index"], used["threads"], used["rows_per_lane"], used["groups"], used["per"]) == \
        ("k_batch", geo, threads, k, groups, threads * k - 1), used
    assert insts[0]["row"] == 1 and not insts[0]["helper"]
    _all_persistent(c, insts, counters, len(c.q))
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_edge_pods():
    c, _ = _edge_case()
    got, rows, insts, geos, counters = c.run_gpu()
    assert geos[0]["groups"] == 4 and geos[0]["index"] == 0
    _all_persistent(c, insts, counters, len(c.q))
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_no_filter_profile():
    c = _nofilter_case()
    got, rows, insts, geos, counters = c.run_gpu()
    _all_persistent(c, insts, counters, len(c.q))
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_seams():
    """Eligible pods and pods with a normalize pass alternate: persistent runs of one pod between per-pod
    launches, then a kgpu_schedule_one cycle, then a second batch, on one rotation."""
    c = _seam_case()
    got, rows, insts, geos, counters = c.run_gpu()
    el = _seam_eligible(c)
    half = SEAM_PODS // 2
    assert insts[0]["persistent_pods"] == int(el[:half].sum())
    assert insts[1]["persistent_pods"] == 0  # the diagnostic cycle keeps the per-pod pipeline
    assert insts[2]["persistent_pods"] == int(el[half + 1:].sum())
    assert counters["cut_persistent_pods"] == int(el[:half].sum()) + int(el[half + 1:].sum())
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_seams_prefer_no_schedule_taint():
    c = _taint_seam_case()
    got, rows, insts, geos, counters = c.run_gpu()
    tolerant = np.arange(len(c.q)) % 3 != 0
    assert insts[0]["persistent_pods"] == int(tolerant.sum()), insts
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_first_max_tie_mode():
    c, _ = _c700(30, tie=1)
    got, rows, insts, geos, counters = c.run_gpu()
    _all_persistent(c, insts, counters, 40)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_default_configuration_at_full_size():
    """test_gpu_pct0_5k_nodes_matches_c_restatement's (b) case: 5,000 nodes, the adaptive default
    (to_find 500), 300 pods, all inside the cut-mode launch."""
    from oracle.cref import RefEngine
    nodes, ex, pods, prof = cluster.fit_least_balanced(n_nodes=5000, n_pods=300)
    prof.percentage_of_nodes_to_score = 0
    fw = GpuFramework(prof, nodes, ex, pods_hint=pods)
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    ref = RefEngine(fw.config, fw.snap, threads=8)
    want = ref.schedule(q, pc)
    want_rows = ref.read_nodes()
    ref.close()
    got, _ = fw.engine.schedule_batch(q, pc)
    assert fw.engine.instantiation()["persistent_pods"] == 300
    assert fw.engine.counters()["cut_persistent_pods"] == 300
    _equal(want, got, want_rows, fw.engine.read_nodes(fw.snap.n_nodes))
    assert (got["feasible"][got["node"] >= 0] <= 500).all()


@pytest.mark.gpu
def test_gpu_cut_cooperative_launch():
    """KGPU_OPT_COOPERATIVE 1: the cut-mode run goes through hipLaunchCooperativeKernel (what the re-issue
    after a clean abort uses) and computes the same."""
    c, _ = _c700(30)
    got, rows, insts, geos, counters = c.run_gpu([(abi.OPT_COOPERATIVE, 1)])
    assert counters["coop_launches"] >= 1 and counters["coop_retries"] == 0, counters
    _all_persistent(c, insts, counters, 40)
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_abort_hook_fails_the_batch_and_recovers():
    """KGPU_OPT_ABORT_AT inside a cut-mode run: KGPU_E_DEVICE, cycles refused until the next upload, then
    the reference's records: an aborted run leaves nextStartNodeIndex as it found it (workgroup 0 writes it
    only at the end of a complete run)."""
    from kgpu.native import KgpuError
    c, _ = _c700(30)
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
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
