"""The delta stream (kgpu_apply_delta) at persistent-kernel sizes, under a cut and on aliased lists.

tests/test_delta.py sends every kind of delta, but to 40 nodes (one workgroup, no cut) with one diagnostic
probe per event; the persistent kernels are held to the reference only on snapshots uploaded whole.  Here a
steered event stream (delta_stream.Stream) runs on the routing families' sizes (gen_random.FAMILIES' reasoning):

  generic  cluster() nodes and rpod pods, 200 nodes, pct 50 (to_find 100; k_batch workgroups of 63 nodes)
  topo     topo_cluster() with 24 existing pods, 400 nodes, pct 25 (to_find 100; k_tbatch workgroups of 256)

each also at percentage 100 (k_batch, k_tbatch without a cut).  A case is 12
checkpoints: six random events, a forced node remove (even checkpoints) or add (odd ones), UpdateSnapshot,
then ONE kgpu_schedule_batch of 8 fresh pods with on-device assume.  The placed pods are assumed in the
mirror and adopted on the device (SchedulerCache.adopt_assumed, as kgpu/ahead.py does), so later forget /
confirm / expire events remove or move pods that a persistent kernel assumed.  One checkpoint per case also
updates a node with a label key no node had: the delta path gives up (NeedsUpload) and the mirror is uploaded
whole, with the rotation carried over.

Aliasing: after a node ADD the nodeTree pass of UpdateSnapshot starts mid-round and the list holds one node
twice until the next node-set change; a REMOVE clears it.  So odd checkpoints run on an aliased list (the
engine then places one pod at a time and assumes through k_delta on every row of the node) and even ones on
a duplicate-free list (the persistent kernels).

Reference per checkpoint, seeded with the rotation (nextStartNodeIndex) the previous checkpoint's reference
ended with, unreduced:
  * duplicate-free list: the C restatement (oracle/c) on a FRESH compile of the mirror's nodes and pods;
  * aliased list: the Python oracle on the mirror's list as given.
Everything is exact: node, feasible, evaluated, scored and score of every pod and all six node-row columns.
`evaluated` is what pins the rotation.  At duplicate-free checkpoints the deltas of Engine.counters() and
instantiation()["persistent_pods"] are held to what the routing loop must do (test_random_routing._routing),
so a fall-back to a per-pod pipeline after a delta fails a case whose records still match: exact per batch in the
generic family; in the topology family test_random_routing's bounds (_topo_kinds_of on the mirror's pods and the
batch's own, _topo_bounds) over the case's duplicate-free checkpoints -- at least the pods that certainly have
no topology plan run in k_cbatch / k_nbatch, at most those that may have none, at least the pods with terms
k_tbatch carries run in it.

The threshold question (settled on the CPU, test_threshold_fold_is_the_reference_rule): the reference stores
nextStartNodeIndex = (nextStartNodeIndex + processedNodes) % len(allNodes) in EVERY cycle
(generic_scheduler.go:487).  Without a cut processedNodes is the list length, so the cycle only folds the
stored index into the current list.  The C restatement and the engine used to touch the index only under a
cut: with 101 nodes (to_find 100) the index reaches 100, two nodes leave (99 nodes, no cut), one batch runs,
the nodes return: the reference starts at 1, the restatement and the engine started at 100.  The defect was
real; oracle/c now folds in the uncut branch and the engine folds cut_buf once, on the host, in the first
uncut cycle after a node-list rebuild (fold_rotation, kgpu_api.cpp).  _Threshold keeps the sequence.

What the aliased checkpoints found (the engine as it was gave `evaluated` 400 where the oracle has 398, on
a 400-row list with two duplicates and a pod that no node fits):
processedNodes is len(filtered) + len(statuses) and `statuses` is a map by node NAME
(generic_scheduler.go:465-487), so a failing node whose two rows were both examined counts once, in
EvaluatedNodes and in the advance of nextStartNodeIndex.  The engine counted rows.  Its one-pod-at-a-time
loop over an aliased list now runs each cycle on the per-pod launches, reads the status words of the aliased
rows and takes the surplus off the record and off the stored index (alias_processed, kgpu_api.cpp).
selectHost on such a list sees the node once per row; the Python oracle now ranks each entry by its own list
position (framework.select_host's `rows`), which is what the engine's packed key always did.
"""
import functools
import hashlib
import types

import numpy as np
import pytest

import gen_random
from delta_stream import NEW_LABEL_KEY, Stream
from kgpu import abi
from kgpu.cache import SchedulerCache
from kgpu.compile import Cluster, Compiler, Pools, Profile
from oracle.refsched import framework as F

from test_percentage_persistent import ROW_KEYS, _equal, _to_find
from test_random_routing import (COUNTERS, OPTION_SETS as ROUTING_OPTION_SETS, _kind, _needs_norm, _routing, _topo_bounds,
                                 _topo_counts, _topo_kinds_of)

# family -> (nodes, cut percentage, fewest nodes that still make two workgroups of its persistent kernel)
FAMILIES = {"generic": (200, 50, 64), "topo": (400, 25, 257)}
CHECKPOINTS, STEPS, BATCH = 12, 6, 8
# three seeds per family; test_pinned_seeds_meet_their_conditions holds each to what the GPU cases need
SEEDS = {"generic": [0, 3, 5], "topo": [240, 450, 1339]}
OPTION_SETS = {k: ROUTING_OPTION_SETS[k] for k in ("default", "norm1", "perpod")}
THRESHOLD_SEED = 5  # the lead pods fit all 101 nodes (test_threshold_fold_is_the_reference_rule)
# sha256 (16 digits) of the list and the drawn ops after 120 steps of test_delta's seed 0, taken with the parent commit's class
STREAM0_DIGEST = "3fb17c54b80b57b4"


def _label_checkpoint(seed):
    """The checkpoint that carries the new-label-key update: 4..7, so both list kinds occur over the seeds."""
    return 4 + seed % 4


def _inputs(fam, seed, n):
    if fam == "generic":
        nodes, existing, _ = gen_random.cluster(seed, n, n // 2, 0)
        return nodes, existing, [], []
    nodes, existing, _, services, rss = gen_random.topo_cluster(seed, n, 24, 0)
    return nodes, existing, services, rss


def _rows_of(snapshot):
    cols = {k: [] for k in ROW_KEYS}
    for ni in snapshot.list:
        for k, v in zip(ROW_KEYS, (ni.requested.milli_cpu, ni.requested.memory, ni.requested.eph, ni.non_zero.milli_cpu,
                                   ni.non_zero.memory, len(ni.pods))):
            cols[k].append(v)
    return {k: np.array(v, np.int32 if k == "num_pods" else np.int64) for k, v in cols.items()}


def _oracle_records(results):
    """(host or None, feasible, evaluated, scored, score) per pod from oracle.refsched results."""
    out = []
    for w in results:
        if isinstance(w, F.FitError):
            out.append((None, 0, len(w.statuses), 0, 0))
        elif isinstance(w, F.ScheduleError):
            raise AssertionError("the stream drew a pod the reference rejects before filtering: %s" % w)
        else:
            scored = int(w.feasible > 1)
            out.append((w.host, w.feasible, w.evaluated, scored, dict(w.totals)[w.host] if scored else 0))
    return out


def _records(res, names):
    """The same tuples from kgpu_result records over the list `names`."""
    return [(names[int(r["node"])] if r["node"] >= 0 else None, int(r["feasible"]), int(r["evaluated"]), int(r["scored"]),
             int(r["score"])) for r in res]


def _fresh_compile(c, prof, cluster, pods):
    """The issue's recipe: a new Compiler on the mirror's nodes and pods in list order, and `pods` compiled by it."""
    ordered, existing = c.ordered_nodes(), c.listed_pods()
    comp = Compiler(prof, cluster)
    comp.register(ordered, existing, pods)
    snap, arrays, order = comp.compile_snapshot(ordered, existing, ordered=ordered)
    assert order == c.list
    pools = Pools()
    q = np.array([comp.compile_pod(p, pools) for p in pods], abi.QUERY)
    pc, _ = pools.finalize()
    return types.SimpleNamespace(comp=comp, config=comp.config(0), snap=snap, arrays=arrays, q=q, pc=pc)


class _Walk:
    """One case's mirror and stream.  The stream's draws never depend on a device, so the reference walk (CPU)
    and every GPU run of the case see the same events, lists and pods."""

    def __init__(self, fam, seed, pct, n_nodes=None, device=False, label_cp=None):
        n = n_nodes or FAMILIES[fam][0]
        nodes, existing, self.services, self.rss = _inputs(fam, seed, n)
        self.fam, self.seed, self.pct = fam, seed, pct
        self.prof = Profile(percentage_of_nodes_to_score=pct)
        self.oprof = F.Profile(percentage_of_nodes_to_score=pct)
        self.cluster = Cluster(services=self.services, rss=self.rss)
        self.c = SchedulerCache(self.prof, nodes, existing, cluster=self.cluster, create_engine=device)
        self.s = Stream(seed, self.c, nodes, self.services, self.rss, gpu=False, generic=(fam == "generic"))
        self.label_cp = _label_checkpoint(seed) if label_cp is None else label_cp
        self.rotation = 0  # the one integer carried between checkpoints
        self.seq = 0
        # every pod whose terms the engine may have interned since the last full upload: a term class outlives
        # its pods until then (build_plans matches a pod against all of kgpu_ctx::tclasses), so a pod that only a
        # removed pod's term matches still has a topology plan
        self.known = list(existing)
        fresh = self.s.fresh_pod

        def fresh_pod(*a, **kw):
            p = fresh(*a, **kw)
            self.known.append(p)
            return p
        self.s.fresh_pod = fresh_pod

    def advance(self, k):
        """Checkpoint k's events and UpdateSnapshot: (the batch's pods, whether the mirror was uploaded whole)."""
        c, s = self.c, self.s
        up0 = c.uploads
        for _ in range(STEPS):
            s.step()
        s.force("node_remove" if k % 2 == 0 else "node_add")
        if k == self.label_cp:
            s.force("node_new_label_key")
        c.sync()
        if c.uploads > up0:
            self.known = c.listed_pods()  # the upload interned the listed pods' terms only
        return [s.fresh_pod() for _ in range(BATCH)], c.uploads > up0

    def fresh_compile(self, pods):
        return _fresh_compile(self.c, self.prof, self.cluster, pods)

    def c_reference(self, pods, rotation):
        from oracle.cref import RefEngine
        fc = self.fresh_compile(pods)
        ref = RefEngine(fc.config, fc.snap, threads=4)
        try:
            ref.next_start = rotation
            res = ref.schedule(fc.q, fc.pc, first_seq=self.seq)
            return fc, res, ref.read_nodes(), ref.next_start
        finally:
            ref.close()

    def py_reference(self, pods, rotation):
        c, state = self.c, {}
        res = F.schedule_sequence(c.ordered_nodes(), c.listed_pods(), pods, self.oprof, services=self.services,
                                  rss=self.rss, first_seq=self.seq, order="given", image_nodes=list(c.nodes.values()),
                                  next_start=rotation, state=state)
        return _oracle_records(res), _rows_of(state["snapshot"]), state["next_start"]

    def commit(self, pods, hosts, slot=None):
        """cache.AssumePod of every placed pod on its host; on a device the pod is adopted, not sent."""
        for pod, host in zip(pods, hosts):
            if host is None:
                continue
            pod["spec"]["nodeName"] = host
            self.c.assume_pod(pod)
            key = pod["metadata"]["uid"]
            if slot is not None:
                assert self.c.adopt_assumed(slot, key, host), key
                slot += 1
            self.s.assumed[key] = pod
        self.seq += len(pods)


def _checkpoint(w, k, pods, uploaded, both=True):
    """The reference's view of one checkpoint, computed with w.rotation; advances w.rotation."""
    c = w.c
    cp = types.SimpleNamespace(k=k, names=list(c.list), n=len(c.list), uploaded=uploaded, first_seq=w.seq,
                               rotation_in=w.rotation, uids=[p["metadata"]["uid"] for p in pods],
                               to_find=_to_find(len(c.list), w.pct))
    cp.dup_free = len(set(cp.names)) == cp.n
    if cp.dup_free:
        fc, cp.res, cp.rows, cp.rotation_out = w.c_reference(pods, w.rotation)
        cp.want = _records(cp.res, cp.names)
        cp.case = types.SimpleNamespace(q=fc.q, pc=fc.pc, fw=types.SimpleNamespace(arrays=fc.arrays),
                                        calls=[("batch", 0, len(pods))], keep=fc)
        cp.kinds = [_kind(cp.case, i) for i in range(len(pods))]
        # what the topology bounds count (test_random_routing._topo_bounds), against every term the engine knows
        cp.counts = _topo_counts(*_topo_kinds_of(w.known, pods, cp.case), _needs_norm(cp.case))
        cp.score_error = int(((fc.q["flags"] & abi.Q_SCORE_ERROR) != 0).sum())
        if both:
            cp.py_want, cp.py_rows, cp.py_rotation_out = w.py_reference(pods, w.rotation)
    else:
        cp.want, cp.rows, cp.rotation_out = w.py_reference(pods, w.rotation)
    cp.hosts = [r[0] for r in cp.want]
    w.rotation = cp.rotation_out
    return cp


@functools.lru_cache(maxsize=None)
def _reference(fam, seed, pct):
    """The case's 12 checkpoints by the reference alone; the GPU cases of every option set share it unchanged."""
    w = _Walk(fam, seed, pct)
    cps = []
    for k in range(CHECKPOINTS):
        pods, uploaded = w.advance(k)
        cp = _checkpoint(w, k, pods, uploaded)
        w.commit(pods, cp.hosts)
        cps.append(cp)
    return cps


# ---------------------------------------------------------------- the threshold case
def _everywhere_pod(name, prefer_host=None):
    """No requests, every taint tolerated (NodeUnschedulable's included): feasible on every node with a free
    pod slot.  prefer_host: a preferred node-affinity term of weight 100 on that node's hostname label."""
    spec = {"containers": [{"name": "c", "image": "img0"}], "tolerations": [{"operator": "Exists"}]}
    if prefer_host is not None:
        spec["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
            {"weight": 100, "preference": {"matchExpressions": [
                {"key": gen_random.HOST, "operator": "In", "values": [prefer_host]}]}}]}}
    return {"metadata": {"name": name, "namespace": "default", "uid": name, "labels": {"app": "a"}}, "spec": spec}


THRESHOLD_N = 101  # the adaptive percentage (0) gives 50 %: to_find = max(50, 100) = 100 < 101


class _Threshold(_Walk):
    """101 generic nodes at percentage 0.  Phase 0: one batch led by a pod that fits everywhere (p = 100, the
    rotation reaches 100).  Phase 1: two removes, 99 nodes, no cut, one batch.  Phase 2: three adds, then one
    remove, 101 nodes without a duplicate, one batch led by a pod that fits everywhere and prefers list[0] --
    the node the cut drops when the pass starts at 1, and keeps when it starts at 100."""

    def __init__(self, device=False):
        super().__init__("generic", THRESHOLD_SEED, 0, n_nodes=THRESHOLD_N, device=device, label_cp=-1)

    def advance(self, k):
        c, s = self.c, self.s
        up0 = c.uploads
        # phase 2 syncs between the adds and the remove: the adds' pass lists a node twice and ends the
        # nodeTree's round, so the remove's pass is a clean one
        for ops in {0: [[]], 1: [["node_remove"] * 2], 2: [["node_add"] * 3, ["node_remove"]]}[k]:
            for op in ops:
                s.force(op)
            c.sync()
        lead = _everywhere_pod("everywhere%d" % k, prefer_host=c.nodes[c.list[0]]["metadata"]["labels"][gen_random.HOST]
                               if k == 2 else None)
        return [lead] + [s.fresh_pod() for _ in range(BATCH - 1)], c.uploads > up0


@functools.lru_cache(maxsize=None)
def _threshold_reference():
    """Every record of the threshold case is held to the PYTHON oracle (the C restatement shared the defect)."""
    w = _Threshold()
    cps = []
    for k in range(3):
        pods, uploaded = w.advance(k)
        cp = _checkpoint(w, k, pods, uploaded)
        assert cp.dup_free
        cp.c_want, cp.c_rows, cp.c_rotation_out = cp.want, cp.rows, cp.rotation_out
        cp.want, cp.rows, cp.rotation_out = cp.py_want, cp.py_rows, cp.py_rotation_out
        cp.hosts = [r[0] for r in cp.want]
        w.rotation = cp.rotation_out
        if k == 2:  # what a pass that kept the unfolded index would have given
            cp.unfolded, _, _ = w.py_reference(pods, cps[0].rotation_out)
        w.commit(pods, cp.hosts)
        cps.append(cp)
    return cps


# ---------------------------------------------------------------- CPU
def _cases():
    return [(fam, seed, pct) for fam in sorted(SEEDS) for seed in SEEDS[fam] for pct in (FAMILIES[fam][1], 100)]


def test_rotation_setter_getter_round_trip():
    """A RefEngine that schedules pods a + b in one call equals one that schedules a, has its rotation read out,
    and is recreated on its own post-assume state, seeded with that rotation, for b."""
    from oracle.cref import RefEngine
    nodes, existing, pods = gen_random.cluster(3, 200, 100, 16)
    prof, cl = Profile(percentage_of_nodes_to_score=50), Cluster()
    c = SchedulerCache(prof, nodes, existing, cluster=cl, create_engine=False)
    fc = _fresh_compile(c, prof, cl, pods)
    ref = RefEngine(fc.config, fc.snap)
    whole = ref.schedule(fc.q, fc.pc)
    whole_rows, whole_rotation = ref.read_nodes(), ref.next_start
    ref.close()
    assert (whole["evaluated"] < 200).any() and whole_rotation != 0
    ref = RefEngine(fc.config, fc.snap)
    first = ref.schedule(fc.q[:8], fc.pc)
    rotation = ref.next_start
    ref.close()
    assert rotation == int(first["evaluated"].astype(np.int64).sum()) % 200
    for p, r in zip(pods[:8], first):  # its own post-assume state
        if r["node"] >= 0:
            p["spec"]["nodeName"] = c.list[int(r["node"])]
            c.add_pod(p)
    c.sync()
    fc2 = _fresh_compile(c, prof, cl, pods[8:])
    ref = RefEngine(fc2.config, fc2.snap)
    assert ref.next_start == 0
    with pytest.raises(ValueError):
        ref.next_start = -1
    assert ref.next_start == 0
    ref.next_start = rotation
    second = ref.schedule(fc2.q, fc2.pc, first_seq=8)
    _equal(whole, np.concatenate([first, second]), whole_rows, ref.read_nodes())
    assert ref.next_start == whole_rotation
    # stored unreduced, reduced on use
    ref.next_start = rotation + 200
    assert ref.next_start == rotation + 200
    ref.close()


@pytest.mark.parametrize("fam,seed,pct", _cases())
def test_c_restatement_matches_python_oracle_with_the_carried_rotation(fam, seed, pct):
    """Every duplicate-free checkpoint: records, node rows and the rotation left behind."""
    n_dup_free = 0
    for cp in _reference(fam, seed, pct):
        if not cp.dup_free:
            continue
        n_dup_free += 1
        assert cp.want == cp.py_want, (cp.k, cp.rotation_in, cp.want, cp.py_want)
        for k in ROW_KEYS:
            np.testing.assert_array_equal(cp.rows[k], cp.py_rows[k], err_msg="checkpoint %d %s" % (cp.k, k))
        assert cp.rotation_out == cp.py_rotation_out, cp.k
    assert n_dup_free >= 3


def test_threshold_fold_is_the_reference_rule():
    """Decides the suspected defect on the CPU: the C restatement, seeded and read like the engine's cut_buf,
    equals the Python oracle in all three phases, and the phases are what the docstring says."""
    cps = _threshold_reference()
    assert [cp.n for cp in cps] == [THRESHOLD_N, 99, THRESHOLD_N] and [cp.to_find for cp in cps] == [100, 99, 100]
    assert cps[0].rotation_out >= 99, cps[0].want            # phase 0 left the index above the shrunken list
    assert cps[1].rotation_in == cps[0].rotation_out           # carried unreduced ...
    assert cps[1].rotation_out == cps[0].rotation_out % 99     # ... and folded by the uncut cycles
    assert all(r[2] == 99 for r in cps[1].want)
    for cp in cps:
        assert cp.c_want == cp.want, (cp.k, cp.c_want, cp.want)
        assert cp.c_rotation_out == cp.rotation_out, cp.k
        for k in ROW_KEYS:
            np.testing.assert_array_equal(cp.c_rows[k], cp.rows[k], err_msg="phase %d %s" % (cp.k, k))
    # phase 2's lead pod tells the two starts apart: the cut (p = 100 of 101) drops list[0] from a pass that
    # starts at 1 and keeps it in one that starts at 100, and the pod prefers that node
    lead, lead_unfolded = cps[2].want[0], cps[2].unfolded[0]
    assert lead[1:3] == (100, 100) and lead_unfolded[1:3] == (100, 100)
    assert lead[0] != cps[2].names[0] and lead_unfolded[0] == cps[2].names[0], (lead, lead_unfolded)


@pytest.mark.parametrize("fam", sorted(SEEDS))
def test_pinned_seeds_meet_their_conditions(fam):
    """From the reference alone.  Per case: node counts that keep two workgroups, at least 3 duplicate-free
    checkpoints after a k_remap reorder, at least 3 aliased ones, one full upload at the label checkpoint.  Per
    family at its cut percentage: at least a quarter of the pods cut, at most a third FitErrors, and a pod of
    every routing kind the family can produce at duplicate-free checkpoints."""
    n0, cut_pct, min_nodes = FAMILIES[fam]
    assert len(SEEDS[fam]) == 3 and _to_find(n0, cut_pct) == 100
    cut = fit = total = 0
    kinds = set()
    for seed in SEEDS[fam]:
        for pct in (cut_pct, 100):
            cps = _reference(fam, seed, pct)
            assert len(cps) == CHECKPOINTS
            assert all(cp.n >= min_nodes and abs(cp.n - n0) <= 12 for cp in cps), [cp.n for cp in cps]
            assert len({cp.n for cp in cps}) >= 2                       # N drifts
            assert sum(cp.dup_free and not cp.uploaded for cp in cps) >= 3, [(cp.dup_free, cp.uploaded) for cp in cps]
            assert sum(not cp.dup_free for cp in cps) >= 3
            assert [cp.k for cp in cps if cp.uploaded] == [_label_checkpoint(seed)]
            assert all(cp.to_find < cp.n for cp in cps) == (pct < 100)
            for cp in cps:
                if cp.dup_free:
                    assert cp.score_error == 0
                    if fam == "generic":
                        assert "topology" not in cp.kinds
            if pct == 100:
                continue
            for cp in cps:
                total += BATCH
                cut += sum(r[2] < cp.n for r in cp.want)
                fit += sum(r[0] is None for r in cp.want)
                if cp.dup_free:
                    kinds.update(cp.kinds)
    assert 4 * cut >= total, (cut, total)
    assert 3 * fit <= total, (fit, total)
    if fam == "topo":
        # the bounds bite: every case has pods k_tbatch must carry and a pod that certainly reaches k_nbatch (under
        # option 26) or k_cbatch.  The latter (no plan, both PreferNoSchedule taints tolerated, no term interned
        # since the last upload matches it) is rare here as in test_random_routing: of seeds 0..1500 only 1339 has
        # one at a duplicate-free checkpoint, so it is in the list; 240 and 450 have three and four for k_nbatch
        certain_cbatch = certain_nbatch = 0
        for seed in SEEDS[fam]:
            n = {}
            for cp in _reference(fam, seed, cut_pct):
                if cp.dup_free:
                    for x, v in cp.counts.items():
                        n[x] = n.get(x, 0) + v
            assert n["planned"] >= 3 and n["free_need"] + n["free_plain"] >= 1, (seed, n)
            certain_cbatch += n["free_plain"] >= 1
            certain_nbatch += n["free_need"] >= 1
            assert n["free_plain"] <= n["loose_plain"] and n["free_need"] <= n["loose_need"], (seed, n)
        assert certain_cbatch >= 1 and certain_nbatch >= 2
    assert kinds == ({"plain", "normalize-pass"} if fam == "generic" else {"plain", "normalize-pass", "topology"}), kinds


def test_moved_stream_draws_as_before():
    """delta_stream.Stream is tests/test_delta.py's former class: seed 0's list after 120 steps of the
    host-bookkeeping test has the digest the parent commit's class gives."""
    import test_delta
    nodes, existing, services, rss = test_delta._cluster(0, 24)
    c = SchedulerCache(Profile(), nodes, existing, cluster=Cluster(services, rss=rss), create_engine=False)
    s = Stream(0, c, nodes, services, rss, gpu=False)
    ops = []
    for _ in range(120):
        ops.append(s.step())
        c.sync()
    assert NEW_LABEL_KEY not in str(c.nodes)
    assert hashlib.sha256("\n".join(c.list + ops).encode()).hexdigest()[:16] == STREAM0_DIGEST


# ---------------------------------------------------------------- GPU
def _describe(cp, got):
    bad = [i for i, (a, b) in enumerate(zip(cp.want, got)) if a != b]
    return ("checkpoint %d (%s list of %d, to_find %d, rotation in %d, uploaded %s): pods %s differ\n  want %s\n  got  %s" %
            (cp.k, "duplicate-free" if cp.dup_free else "aliased", cp.n, cp.to_find, cp.rotation_in, cp.uploaded, bad,
             [cp.want[i] for i in bad[:3]], [got[i] for i in bad[:3]]))


def _run_gpu(w, cps, fam, opts, advance_count):
    """The reference's checkpoints on a device mirror: records and node rows exact at every checkpoint, the
    routing counters at duplicate-free ones.  Returns the routing failures (reported after the records)."""
    c, e = w.c, w.c.engine
    for opt, v in OPTION_SETS[opts]:
        e.set_option(opt, v)
    routing_bad = []
    topo_tot, topo_n = {True: {}, False: {}}, {True: {}, False: {}}  # under a cut / without: counter totals, pod counts
    for k in range(advance_count):
        cp = cps[k]
        gen0 = c.generation
        pods, uploaded = w.advance(k)
        assert c.list == cp.names and [p["metadata"]["uid"] for p in pods] == cp.uids and uploaded == cp.uploaded
        pools = Pools()
        q = np.array([c.compiler.compile_pod(p, pools) for p in pods], abi.QUERY)
        pc, _ = pools.finalize()
        before, resident0 = e.counters(), e.topo_resident()
        slot = e.next_slot()
        res, _ = e.schedule_batch(q, pc, first_seq=w.seq)
        after = e.counters()
        got = _records(res, c.list)
        assert got == cp.want, _describe(cp, got)
        rows = e.read_nodes(cp.n)
        for col in ROW_KEYS:
            np.testing.assert_array_equal(cp.rows[col], rows[col], err_msg="checkpoint %d %s" % (cp.k, col))
        if cp.dup_free:
            _equal(cp.res, res, cp.rows, rows)
            if opts in ("default", "norm1"):
                d = {x: after[x] - before[x] for x in COUNTERS}
                d["persistent_pods"] = e.instantiation()["persistent_pods"]
                pct = w.pct if cp.to_find < cp.n else 100  # what the list's length makes of the percentage
                cut = pct < 100
                if fam == "generic":
                    bad = _routing("generic_taints", w.seed, pct, opts, cp.case, [d])
                else:
                    bad = _routing("topo", w.seed, pct, opts, cp.case, [d], topo_sum=topo_tot[cut])
                    for x, v in cp.counts.items():
                        topo_n[cut][x] = topo_n[cut].get(x, 0) + v
                    # nothing between two batches of this file leaves the mirror untouched (test_topo_resident holds
                    # the hits); after a delta a run must not start from the resident state
                    if not cut and c.generation > gen0 and e.topo_resident()[0] != resident0[0]:
                        bad.append(("a run after a delta started from the resident topology state", resident0,
                                    e.topo_resident()))
                routing_bad += [(cp.k,) + tuple(b) for b in bad]
        w.commit(pods, cp.hosts, slot=slot)
    for cut, tot in topo_tot.items():  # the topology family's bounds, over the case's duplicate-free checkpoints
        if tot:
            _topo_bounds(lambda cond, *msg: cond or routing_bad.append(("all",) + msg + (topo_n[cut],)), opts, cut, tot,
                         topo_n[cut], tot["batch_pods"], False)
    return routing_bad


def _matrix():
    for fam in sorted(SEEDS):
        for seed in SEEDS[fam]:
            for pct in (FAMILIES[fam][1], 100):
                for opts in OPTION_SETS:
                    yield pytest.param(fam, seed, pct, opts, id="%s-s%d-p%d-%s" % (fam, seed, pct, opts))


@pytest.mark.gpu
@pytest.mark.parametrize("fam,seed,pct,opts", list(_matrix()))
def test_gpu_delta_stream_routing(fam, seed, pct, opts):
    cps = _reference(fam, seed, pct)
    w = _Walk(fam, seed, pct, device=True)
    try:
        uploads0 = w.c.uploads
        bad = _run_gpu(w, cps, fam, opts, CHECKPOINTS)
        assert w.c.uploads == uploads0 + 1  # the label checkpoint, and nothing else, uploaded the mirror whole
        w.c.sync()                           # the last batch's adopted pods leave nothing to send
        assert not bad, "%s seed %d pct %d %s: records equal, routing differs: %s" % (fam, seed, pct, opts, bad)
    finally:
        w.c.close()


@pytest.mark.gpu
def test_gpu_threshold_fold():
    """The sequence of the module docstring on the device, every record held to the Python oracle."""
    cps = _threshold_reference()
    w = _Threshold(device=True)
    try:
        bad = _run_gpu(w, cps, "generic", "default", 3)
        assert not bad, bad
    finally:
        w.c.close()
