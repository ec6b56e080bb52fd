"""Parity over the persistent kernels' instantiation table: k_batch and k_tbatch are compiled once per
(profile row x geometry x sharded or not), every entry its own machine code, and one entry has been
wrong on its own before (tools/repro/stat_select.hip).  Each case runs one entry on the smallest
cluster that fills its geometry and compares placements, feasible counts, scored counts, scores and
all six node-row columns with the C restatement (oracle/c): exact integer equality, no tolerance.
Each case also asks the engine what it ran: kernel, geometry index and rows per lane
(kgpu_debug_geometry); profile row, sharding flag and how many pods of the call ran inside persistent
launches (kgpu_debug_instantiation), which must be at least half of the batch.

Inputs.  k_tbatch: gen_random.topo_cluster as it stands; KGPU_OPT_PERSISTENT is 0 there, so the few
pods without topology state take per-pod launches and the call's last persistent launch is k_tbatch's.
k_batch: gen_random.cluster with the nodes' PreferNoSchedule taints removed (_generic).  With them
(60% of the nodes carry one that 95% of the pods do not tolerate) TaintToleration's normalize maximum
is not constant, run_batch sends nearly every pod through one launch per pod, and the persistent kernel
sees a twentieth of the batch.  Without them the pods without preferred node-affinity terms -- about
60% -- are persistent-eligible, in runs broken up by the others.  The node-sharded k_batch ranks have
no RCCL communicator for the per-pod exchange, so they schedule the eligible pods only; the
node-sharded k_tbatch ranks run config (c)'s generator (cluster.taints_affinity_spread), whose pods all
carry spread constraints.

Seeds.  Chosen by running the C restatement alone on the CPU, smallest first: a streamed or multi-row
case (rows per lane >= 4) takes the first seed, searched upwards from 0, under which every row
j = (node mod per) // 512 that holds a node receives a placement in the reference run under every one
of the profiles of its family and, for the generic 512 x 8 cluster, at least one pod with extended
resources or host ports lands in a row j >= 4 (the slow path's re-evaluation of the winning row).
Only pods that run inside a persistent launch for certain count towards either (_eligible): a pod that
takes per-pod launches shows nothing about the kernel's rows.  The first-max tie-break concentrates
placements in row 0, so those cases require a placement in the upper half of the rows only.  The
node-sharded generic cluster takes the first seed under which every node-holding row of each rank
(rows 0-2 of its workgroup, by (node - base) mod per // 512) receives a placement under the three
k_batch profiles run there; config (c)'s generator is unseeded here and meets the same condition.  The
diagnostic sequence has its own seed (DIAG_SEED).  Every case checks its condition on the reference
before any GPU work."""
import functools
import os
import tempfile

import numpy as np
import pytest

import gen_random
from kgpu import abi, cluster
from kgpu.compile import Cluster, Profile
from kgpu.framework import GpuFramework
from kgpu.native import Engine

ROW_KEYS = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "num_pods")
FIELDS = ("node", "feasible", "scored", "score")


def _most():
    scores = [s for s in Profile.DEFAULT_SCORES if s[0] != "NodeResourcesLeastAllocated"]
    return Profile(scores=scores + [("NodeResourcesMostAllocated", 1), ("RequestedToCapacityRatio", 2),
                                    ("NodeResourceLimits", 1)])


def _fit():
    return Profile(filters=["NodeResourcesFit"], scores=[("NodeResourcesLeastAllocated", 1),
                                                         ("NodeResourcesBalancedAllocation", 1)])


# name: (profile, k_batch profile row (select_spec), k_tbatch profile row (launch_tbatch))
PROFILES = {
    "default": (Profile, 2, 2),
    "autoscaler": (Profile.cluster_autoscaler, 3, 3),
    "most": (_most, 0, 1),        # the runtime profile, Least/Most over the default resources
    "least21": (lambda: Profile(least_resources=(("cpu", 2), ("memory", 1))), 0, 0),  # the runtime profile
    "fit": (_fit, 1, None),       # generic pods only
    # runtime switches of the default profile
    "tie1": (lambda: Profile(tie_break_mode=1), 2, 2),
    "hpaw": (lambda: Profile(hard_pod_affinity_weight=5), 2, 2),
}
TOPO_PROFILES = ("least21", "most", "default", "autoscaler")  # k_tbatch rows 0..3

# (threads, rows per lane) by geometry index; k_batch keeps the last slot of the last lane as a spare
GEO = [(64, 1), (128, 1), (192, 1), (448, 1), (960, 1), (512, 4), (512, 8)]
TGEO = [(256, 1), (512, 1), (512, 2), (512, 4), (512, 8)]
# nodes of the smallest cluster that fills the geometry, and the seed (module docstring)
GENERIC_SHAPE = {0: (300, 0), 1: (300, 0), 2: (300, 0), 3: (300, 0), 4: (300, 0), 5: (2047, 0), 6: (4095, 0)}
TOPO_SHAPE = {0: (1500, 1), 1: (1500, 1), 2: (1500, 1), 3: (2048, 0), 4: (4096, 4)}


def _generic(seed, n_nodes, n_existing=400):
    nodes, existing, pods = gen_random.cluster(seed, n_nodes=n_nodes, n_existing=n_existing, n_pods=120)
    for n in nodes:
        taints = [t for t in n["spec"].get("taints", []) if t["effect"] != "PreferNoSchedule"]
        if taints:
            n["spec"]["taints"] = taints
        else:
            n["spec"].pop("taints", None)
    return nodes, existing, pods, None


def _topo(seed, n_nodes):
    nodes, existing, pods, services, rss = gen_random.topo_cluster(seed, n_nodes=n_nodes, n_existing=800, n_pods=80)
    return nodes, existing, pods, Cluster(services=services, rss=rss)


def _eligible(family, q, pods):
    """Pods of the batch that run inside a persistent launch for certain (a lower bound).
    Generic: no preferred node-affinity term and no scoring error, so no normalize pass (the cluster has
    no PreferNoSchedule taint).  Topology: the pod's own spread constraints or (anti-)affinity terms give
    it topology state, and it is none of what k_tbatch leaves to the per-pod pipeline (t_add): more than
    one ScheduleAnyway constraint, a DoNotSchedule constraint on the node-unique hostname key.  Pods
    that only match a service or an existing pod's term run there too but are not counted."""
    if family == "generic":
        return (q["pref_terms"]["count"] == 0) & ((q["flags"] & abi.Q_SCORE_ERROR) == 0)
    out = np.zeros(len(pods), bool)
    for i, p in enumerate(pods):
        tsc = p["spec"].get("topologySpreadConstraints", [])
        aff = p["spec"].get("affinity", {})
        soft = sum(c["whenUnsatisfiable"] == "ScheduleAnyway" for c in tsc)
        hard_host = any(c["whenUnsatisfiable"] == "DoNotSchedule" and c["topologyKey"] == gen_random.HOST for c in tsc)
        out[i] = (bool(tsc) or "podAffinity" in aff or "podAntiAffinity" in aff) and soft <= 1 and not hard_host
    return out


class _Ref:
    """One cluster under one profile: compiled once, scheduled once by the C restatement; the cases
    that share it (the geometries of one cluster size) leave it unchanged."""

    def __init__(self, family, seed, n_nodes, prof, inputs=None, profile=None):
        """inputs, profile: another generator's (nodes, existing, pods, cluster) of the same family and a
        profile object outside PROFILES (tests/test_numeric_range.py)."""
        from oracle.cref import RefEngine
        nodes, existing, pods, cl = inputs or (_generic if family == "generic" else _topo)(seed, n_nodes)
        self.family, self.n_nodes = family, n_nodes
        self.fw = GpuFramework(profile or PROFILES[prof][0](), nodes, existing, cluster=cl, pods_hint=pods,
                               create_engine=False)
        self.q, self.pc, _, errs = self.fw.compile_pods(pods)
        assert not errs
        ref = RefEngine(self.fw.config, self.fw.snap, threads=4)
        self.want = ref.schedule(self.q, self.pc)
        self.rows = ref.read_nodes()
        ref.close()
        self.sure = _eligible(family, self.q, pods)
        self.eligible = int(self.sure.sum())

    def rows_hit(self, per, threads=512):
        """Placements of the reference run per row j = (node mod per) // threads of the workgroups,
        counting only the pods that run inside a persistent launch for certain (self.sure): a pod
        that takes per-pod launches does not show that the kernel's row was assumed into."""
        placed = self.want["node"][self.sure & (self.want["node"] >= 0)]
        n_rows = (min(self.n_nodes, per) - 1) // threads + 1
        return np.bincount((placed % per) // threads, minlength=n_rows)[:n_rows]

    def slow_rows(self, per, threads=512):
        """Rows of the placed pods that take k_batch's slow path (extended resources or host ports),
        again of the certainly persistent pods only."""
        slow = (self.q["scalars"]["count"] > 0) | (self.q["ports"]["count"] > 0)
        nodes = self.want["node"][slow & self.sure & (self.want["node"] >= 0)]
        return (nodes % per) // threads


@functools.lru_cache(maxsize=None)
def _ref(family, seed, n_nodes, prof):
    return _Ref(family, seed, n_nodes, prof)


def _reference_conditions(r, threads, rows, per, all_rows=True):
    """What the reference run must show before the GPU is used: enough persistent-eligible pods, and
    placements in the rows the case is about."""
    assert 2 * r.eligible >= len(r.q), "%d of %d pods persistent-eligible: pick other inputs" % (r.eligible, len(r.q))
    if rows < 4:
        return
    hit = r.rows_hit(per, threads)
    if all_rows:
        assert (hit > 0).all(), "rows without a placement in the reference run %s: pick another seed" % hit
    else:
        assert hit[len(hit) // 2:].sum() > 0, "no placement in the upper rows %s: pick another seed" % hit
    if r.family == "generic" and rows == 8:
        assert (r.slow_rows(per, threads) >= 4).any(), "no slow-path pod placed in a row >= 4: pick another seed"


def _compare(r, got, rows_g):
    for f in FIELDS:
        bad = np.nonzero(r.want[f] != got[f])[0]
        assert len(bad) == 0, "%s differs at pods %s: want %s got %s" % (f, bad[:5], r.want[f][bad[:5]], got[f][bad[:5]])
    for k in ROW_KEYS:
        np.testing.assert_array_equal(r.rows[k], rows_g[k], err_msg=k)


def _run_engine(r, options):
    e = Engine(r.fw.config)
    try:
        e.upload(r.fw.snap, r.fw.arrays)
        for opt, v in options:
            e.set_option(opt, v)
        got, _ = e.schedule_batch(r.q, r.pc)
        return got, e.read_nodes(r.fw.snap.n_nodes), e.geometry(), e.instantiation()
    finally:
        e.close()


def _batch_case(prof, geo, all_rows=True):
    n_nodes, seed = GENERIC_SHAPE[geo]
    threads, rows = GEO[geo]
    per = threads * rows - 1
    r = _ref("generic", seed, n_nodes, prof)
    _reference_conditions(r, threads, rows, per, all_rows)
    options = [(abi.OPT_PERSISTENT, 1)]
    options += [(abi.OPT_BATCH_GEO, geo)] if rows == 1 else [(abi.OPT_PERSIST_GROUPS, 1)]
    got, rows_g, used, inst = _run_engine(r, options)
    _compare(r, got, rows_g)
    assert (used["kernel"], used["index"], used["threads"], used["rows_per_lane"], used["per"]) == \
        ("k_batch", geo, threads, rows, per)
    assert used["groups"] == (n_nodes + per - 1) // per
    assert (inst["row"], inst["sharded"]) == (PROFILES[prof][1], False)
    assert 2 * inst["persistent_pods"] >= len(r.q), inst
    assert inst["persistent_pods"] >= r.eligible, (inst, r.eligible)
    return inst


def _tbatch_case(prof, geo, all_rows=True, extra=()):
    n_nodes, seed = TOPO_SHAPE[geo]
    threads, rows = TGEO[geo]
    per = threads * rows
    r = _ref("topo", seed, n_nodes, prof)
    _reference_conditions(r, threads, rows, per, all_rows)
    options = [(abi.OPT_TOPO_PERSISTENT, 1), (abi.OPT_PERSISTENT, 0)]
    options += [(abi.OPT_TBATCH_GEO, geo)] if rows < 4 else [(abi.OPT_PERSIST_GROUPS, 1)]
    got, rows_g, used, inst = _run_engine(r, options + list(extra))
    _compare(r, got, rows_g)
    assert (used["kernel"], used["index"], used["threads"], used["rows_per_lane"], used["per"]) == \
        ("k_tbatch", geo, threads, rows, per)
    assert used["groups"] == (n_nodes + per - 1) // per
    assert (inst["row"], inst["sharded"], inst["helper"]) == (PROFILES[prof][2], False, False)
    assert 2 * inst["persistent_pods"] >= len(r.q), inst
    assert inst["persistent_pods"] >= r.eligible, (inst, r.eligible)


def test_debug_instantiation_needs_a_context():
    from kgpu import native
    out = np.zeros(4, np.int32)
    assert native.lib().kgpu_debug_instantiation(None, out.ctypes.data) == abi.E_INVAL
    assert native.lib().kgpu_debug_geometry(None, out.ctypes.data) == abi.E_INVAL


def test_reference_conditions_hold_on_the_cpu():
    """The seeds' conditions (module docstring) on the two 512 x 8 clusters under the runtime and the
    default profile, from the C restatement alone: a change of the generators shows here, without a GPU
    (every GPU case checks its own before it runs)."""
    for prof in ("most", "default"):
        r = _ref("generic", GENERIC_SHAPE[6][1], GENERIC_SHAPE[6][0], prof)
        _reference_conditions(r, 512, 8, 4095)
        r = _ref("topo", TOPO_SHAPE[4][1], TOPO_SHAPE[4][0], prof)
        _reference_conditions(r, 512, 8, 4096)


# ---- 1. k_batch, unsharded: every geometry x every profile row (row 0 under both of its profiles)
@pytest.mark.gpu
@pytest.mark.parametrize("geo", range(7))
@pytest.mark.parametrize("prof", ["most", "least21", "fit", "default", "autoscaler"])
def test_gpu_batch_instantiation(prof, geo):
    inst = _batch_case(prof, geo)
    # config (b)'s profile on the one-row-wave geometry takes the helper-wave instantiation
    assert inst["helper"] == (prof == "fit" and geo == 0)


# ---- 2. k_tbatch, unsharded: every geometry x every profile row
@pytest.mark.gpu
@pytest.mark.parametrize("geo", range(5))
@pytest.mark.parametrize("prof", TOPO_PROFILES)
def test_gpu_tbatch_instantiation(prof, geo):
    _tbatch_case(prof, geo)


# ---- 5. runtime switches on the streamed rows
@pytest.mark.gpu
def test_gpu_batch_streamed_first_max_tie_break():
    _batch_case("tie1", 6, all_rows=False)


@pytest.mark.gpu
@pytest.mark.parametrize("prof", ["tie1", "hpaw"])
def test_gpu_tbatch_streamed_profile_switches(prof):
    _tbatch_case(prof, 4, all_rows=prof != "tie1")


@pytest.mark.gpu
@pytest.mark.parametrize("wlab", [0, 1])
def test_gpu_tbatch_streamed_winner_labels_switch(wlab):
    _tbatch_case("default", 4, extra=[(abi.OPT_TBATCH_WLAB, wlab)])


# ---- 6. a diagnostic cycle (kgpu_schedule_one) on the streamed k_tbatch
# the first seed, from 0, whose first 20 pods are at least half certain k_tbatch cycles, one of them scored
# and won in the upper rows, under both geometries
DIAG_SEED = 0
@pytest.mark.gpu
@pytest.mark.parametrize("geo", [3, 4])
def test_gpu_tbatch_streamed_diagnostic_cycles(geo):
    """kgpu_schedule_one with assume over the first 20 pods of the 4,096-node topology cluster, on two
    workgroups of 512 x 4 (one holds 2,048 nodes) and on one of 512 x 8: a topology pod's cycle is a
    one-pod k_tbatch run that writes every node's status word from inside the streamed row loop and the
    per-plugin rows.  (A pod k_tbatch does not carry, such as one with a DoNotSchedule constraint on
    the hostname key, takes the per-pod pipeline and is compared all the same.)
    Each record, every status word and every plugin's raw and normalized score on the feasible nodes
    against the C restatement's diagnostic run of the same sequence."""
    from oracle.cref import RefEngine
    n_nodes = TOPO_SHAPE[4][0]
    r = _ref("topo", DIAG_SEED, n_nodes, "default")
    threads, rows = TGEO[geo]
    per = n_nodes * rows // 8
    q = r.q[:20]
    topo = r.sure[:20]  # the cycles that are one-pod k_tbatch runs for certain
    assert 2 * int(topo.sum()) >= len(q)
    ref = RefEngine(r.fw.config, r.fw.snap, threads=4)
    want = [ref.schedule(q[i:i + 1], r.pc, first_seq=i, diag=True) for i in range(len(q))]
    want_rows = ref.read_nodes()
    ref.close()
    # one of them compares its score rows (more than one feasible node) and places in the upper rows
    assert any(topo[i] and w[0][0]["feasible"] > 1 and (int(w[0][0]["node"]) % per) // threads >= rows // 2
               for i, w in enumerate(want)), "no scored k_tbatch cycle wins in the upper rows: pick another seed"
    sids = sorted(abi.SCORE_IDS[name] for name, _ in r.fw.profile.scores)
    e = Engine(r.fw.config)
    try:
        e.upload(r.fw.snap, r.fw.arrays)
        e.set_option(abi.OPT_TOPO_PERSISTENT, 1)
        e.set_option(abi.OPT_TBATCH_GEO, geo)
        e.set_option(abi.OPT_PERSIST_GROUPS, 8 // rows)
        n_tbatch = 0
        for i in range(len(q)):
            res, _ = e.schedule_one(q[i], r.pc, seq=i, assume=True)
            used, inst = e.geometry(), e.instantiation()
            words = e.filter_words(n_nodes)
            w, st, raw, norm = want[i]
            for f in FIELDS:
                assert res[f] == w[0][f], "cycle %d: %s %s vs oracle/c %s" % (i, f, res[f], w[0][f])
            np.testing.assert_array_equal(words, st, err_msg="cycle %d: status words" % i)
            if topo[i]:
                assert (used["kernel"], used["index"], used["rows_per_lane"]) == ("k_tbatch", geo, rows), (i, used)
                assert (inst["row"], inst["sharded"], inst["persistent_pods"]) == (2, False, 1), (i, inst)
            n_tbatch += used["kernel"] == "k_tbatch"
            feas = st == 0
            # one feasible node is returned unscored (generic_scheduler.go:184-191): no score rows then
            for s in sids if res["feasible"] > 1 else ():
                g_raw, g_norm = e.scores(s, n_nodes)
                np.testing.assert_array_equal(g_raw[feas], raw[s][feas], err_msg="cycle %d: raw score %d" % (i, s))
                np.testing.assert_array_equal(g_norm[feas], norm[s][feas], err_msg="cycle %d: normalized score %d" % (i, s))
        assert 2 * n_tbatch >= len(q), n_tbatch
        rows_g = e.read_nodes(n_nodes)
    finally:
        e.close()
    for k in ROW_KEYS:
        np.testing.assert_array_equal(want_rows[k], rows_g[k], err_msg=k)


# ---- 4. the node-sharded (xGMI mailbox) streamed instantiations: two ranks on one GPU
SHARD_NODES, SHARD_WORLD = 3000, 2
SHARD_SEED = 1  # of the generic cluster (module docstring: the search over the three k_batch profiles)


def _shard_inputs(kernel):
    if kernel == "k_batch":
        nodes, existing, pods, _ = _generic(SHARD_SEED, SHARD_NODES)
        return nodes, existing, pods
    nodes, existing, pods, _ = cluster.taints_affinity_spread(n_nodes=SHARD_NODES, n_pods=80)
    return nodes, existing, pods


def _shard_batch(kernel, q, pods):
    """What the ranks schedule: no communicator for the per-pod exchange, so the generic batch keeps
    its persistent-eligible pods only (config (c)'s pods all carry spread constraints)."""
    return q[_eligible("generic", q, pods)] if kernel == "k_batch" else q


@functools.lru_cache(maxsize=None)
def _shard_ref(kernel, prof):
    """The C restatement on the unsharded cluster: (batch size, records, node rows)."""
    from oracle.cref import RefEngine
    nodes, existing, pods = _shard_inputs(kernel)
    fw = GpuFramework(PROFILES[prof][0](), nodes, existing, pods_hint=pods, create_engine=False)
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    q = _shard_batch(kernel, q, pods)
    ref = RefEngine(fw.config, fw.snap, threads=4)
    want = ref.schedule(q, pc)
    rows = ref.read_nodes()
    ref.close()
    return len(q), want, rows


def _shard_rows_hit(want, per, threads=512):
    """Per rank, the reference run's placements per row j = ((node - base) mod per) // threads of the
    rank's workgroups (every pod of a sharded batch runs inside the persistent kernel)."""
    from kgpu import native
    placed = want["node"][want["node"] >= 0]
    out = []
    for rank in range(SHARD_WORLD):
        base, n = native.shard_range(SHARD_NODES, SHARD_WORLD, rank)
        local = placed[(placed >= base) & (placed < base + n)] - base
        n_rows = (min(n, per) - 1) // threads + 1
        out.append(np.bincount((local % per) // threads, minlength=n_rows)[:n_rows])
    return out


def _shard_rank(rank, world, rdv, kernel, prof, geo, out):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + rdv, rank=rank, world_size=world)
    try:
        nodes, existing, pods = _shard_inputs(kernel)
        fw = GpuFramework(PROFILES[prof][0](), nodes, existing, pods_hint=pods, device=0, shard=(rank, world))
        # before the ranks join: the sharded geometry is fixed then
        fw.engine.set_option(abi.OPT_BATCH_GEO if kernel == "k_batch" else abi.OPT_TBATCH_GEO, geo)
        h = fw.engine.xgmi_handle(world)
        hs = [None] * world
        dist.all_gather_object(hs, h)
        fw.engine.xgmi_init(world, rank, b"".join(hs))
        assert fw.engine.xgmi_active()
        q, pc, _, errs = fw.compile_pods(pods)
        assert not errs
        q = _shard_batch(kernel, q, pods)
        res, pods_in = [], 0
        half = (len(q) + 1) // 2
        for b in range(0, len(q), half):
            res.append(fw.engine.schedule_batch(q[b:b + half], pc, first_seq=b)[0])
            pods_in += fw.engine.instantiation()["persistent_pods"]
        res = np.concatenate(res)
        used, inst = fw.engine.geometry(), fw.engine.instantiation()
        rows = fw.engine.read_nodes(fw.snap.n_nodes)
        np.savez(out, node=res["node"], feasible=res["feasible"], score=res["score"], scored=res["scored"],
                 base=fw.snap.node_base, kernel=used["kernel"] or "", index=used["index"],
                 rows_per_lane=used["rows_per_lane"], row=inst["row"], sharded=inst["sharded"], pods_in=pods_in, **rows)
        fw.engine.close()
    finally:
        dist.destroy_process_group()


SHARDED = [("k_batch", "default", 6), ("k_batch", "autoscaler", 6), ("k_batch", "most", 6),
           ("k_tbatch", "least21", 4), ("k_tbatch", "most", 4), ("k_tbatch", "default", 4),
           ("k_tbatch", "autoscaler", 4), ("k_tbatch", "default", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,prof,geo", SHARDED)
def test_gpu_sharded_streamed_instantiation(kernel, prof, geo, tmp_path):
    """3,000 nodes split 1,500 + 1,500, each rank on the forced streamed geometry (rows 0-2 of its one
    workgroup hold nodes), against the C restatement of the unsharded cluster.  Before the ranks start,
    the reference run must place a pod in every node-holding row of every rank.  No RCCL communicator:
    a pod that left the persistent kernel would fail its batch."""
    import shutil

    import torch.multiprocessing as mp
    table = GEO if kernel == "k_batch" else TGEO
    threads, k = table[geo]
    per = threads * k - (1 if kernel == "k_batch" else 0)
    n_q, want, rows = _shard_ref(kernel, prof)
    assert 2 * int((want["node"] >= 0).sum()) >= n_q
    for rank, hit in enumerate(_shard_rows_hit(want, per, threads)):
        assert (hit > 0).all(), "rank %d: rows without a placement in the reference run %s: pick another seed" % (rank, hit)
    world = SHARD_WORLD
    ctx = mp.get_context("spawn")
    rdv_dir = tempfile.mkdtemp(prefix="kgpu_rdv_")
    rdv = os.path.join(rdv_dir, "store")
    outs = [str(tmp_path / ("r%d.npz" % r)) for r in range(world)]
    procs = [ctx.Process(target=_shard_rank, args=(r, world, rdv, kernel, prof, geo, outs[r])) for r in range(world)]
    for p in procs:
        p.start()
    failed = None
    try:
        for r, p in enumerate(procs):
            p.join(120)
            if p.exitcode != 0:
                failed = "rank %d exited with %r" % (r, p.exitcode)
                break
    finally:
        for p in procs:  # a rank left waiting for a dead peer must not outlive the test
            if p.is_alive():
                p.kill()
                p.join(10)
        shutil.rmtree(rdv_dir, ignore_errors=True)
    assert failed is None, failed  # nothing more runs after a failed child
    for r in range(world):
        got = np.load(outs[r])
        assert (str(got["kernel"]), int(got["index"]), int(got["rows_per_lane"])) == (kernel, geo, table[geo][1])
        assert (int(got["row"]), bool(got["sharded"])) == (PROFILES[prof][1 if kernel == "k_batch" else 2], True)
        assert int(got["pods_in"]) == n_q
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), (r, f, np.nonzero(got[f] != want[f])[0][:5])
        base = int(got["base"])
        n = len(got["num_pods"])
        for c in ROW_KEYS:
            assert np.array_equal(got[c], rows[c][base:base + n]), (r, c)
