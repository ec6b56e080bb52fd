"""Preemption (kgpu_select_victims: k_vict_prep + k_victims) against the oracle past one wave, at the
edges of its reductions and masks, and on state the engine itself wrote.

tests/test_preemption.py stays at 14 nodes, about 3 potential victims per node, at most 3 selecting
PDBs, and on a snapshot uploaded one line earlier.  Here, always as the product
(GpuFramework.select_nodes_for_preemption / .preempt) against oracle/refsched/preemption.py, the steps
of test_preemption._oracle_preempt (preempt_scale.oracle_preempt), integer-exact: the victim list of
every node in Victims.Pods order, numPDBViolations of every node, the picked node.

  1. size matrix      63 / 64 / 65 / 130 / 300 nodes (k_victims: one thread per node, 64 per block),
                      resources and topology clusters, one runAllFilters size
  2. k_vict_prep      330 hostname values: minimum and runner-up in the second stride of the
                      256-thread loop and in different waves, ties, shared pairs, the affinity-map count
  3. deep node        40 potential victims on one node, host ports added and removed along the
                      reprieve order
  4. 64 PDBs          bit 63 of the masks, the 65th selecting PDB
  5. engine state     victims the engine placed itself: after kgpu_schedule_batch (generic, topology,
                      mixed), after kgpu_schedule_one assumes, after kgpu_forget_pod, and the
                      cycle -> FitError -> preempt -> nominate -> cycle loop

Every GPU test asserts on the oracle's answer alone, before the comparison, that the case decides
something (candidates with victims, reprieved pods, a topology verdict that matters); the unmarked tests
hold the generators to the same conditions on the CPU, so a generator change cannot hollow the GPU
tests out.

Out of scope: pods added by kgpu_apply_delta ADD_POD as victims.  kgpu/cache.py drops the slots that
call returns, so the Python mirror cannot name such a victim.

kgpu_schedule_batch fills a placed pod's own term classes only `if (topo_on)`; topo_on is the
profile's (topo_profile(): PodTopologySpread or InterPodAffinity among its plugins), not the batch's,
so under Profile() no schedule() call of pods with terms, however routed, runs with it false."""
import functools

import pytest

import preempt_scale as S
from preempt_scale import NOW
from kgpu.compile import Cluster, Profile
from kgpu.framework import GpuFramework
from oracle.refsched import nodeinfo as NI
from oracle.refsched import preemption as PR


def _hint(*groups):
    return [p for g in groups for p in g]


# ---------------------------------------------------------------- 1. size matrix
MATRIX = S.matrix_cases()
_matrix_reference = functools.lru_cache(maxsize=None)(S.matrix_reference)


@pytest.mark.parametrize("case", MATRIX, ids=[c[0] for c in MATRIX])
def test_matrix_reference_is_not_vacuous(case):
    """Conditions (a)-(d) on the oracle alone, per parametrized case, summed over its preemptors:
    at least 8 candidate nodes with a victim, one with two or more, one reprieved pod and, for the
    topology clusters, one preemptor whose map changes when the PodTopologySpread and InterPodAffinity
    filters are taken out of the profile."""
    name, seed, topo, n, run_all = case
    _, answers, tot = _matrix_reference(seed, topo, n, run_all)
    assert sum(a is not None for a in answers) >= 3, name
    S.assert_not_vacuous(tot, topo, name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MATRIX, ids=[c[0] for c in MATRIX])
def test_matrix_matches_oracle(case):
    name, seed, topo, n, run_all = case
    (nodes, existing, pods, services, rss, pdbs, noms), answers, tot = _matrix_reference(seed, topo, n, run_all)
    S.assert_not_vacuous(tot, topo, name)
    fw = GpuFramework(Profile(run_all_filters=run_all), nodes, existing, cluster=Cluster(services=services, rss=rss),
                      pods_hint=pods + [p for p, _ in noms])
    fw.set_nominated(noms)
    for pod, want in zip(pods, answers):
        if want is None:
            continue
        got = S.gpu_answer(fw, pod, pdbs)
        assert got[0] == want[0], (name, NI.name(pod))
        assert got[1] == want[1], (name, NI.name(pod), got[1], want[1])
    fw.engine.close()


# ---------------------------------------------------------------- 2. k_vict_prep
@functools.lru_cache(maxsize=None)
def _prep_reference(variant):
    c = S.prep_case(variant)
    return c, S.oracle_preempt(c["nodes"], c["existing"], c["pod"], noms=c["noms"])


def _prep_not_vacuous(variant):
    c, want = _prep_reference(variant)
    assert want is not None
    with_v, multi, victims, reprieved = S.counts(c["existing"], c["pod"], want[0])
    assert with_v >= 8 and reprieved >= 1, (variant, with_v, multi, victims, reprieved)
    return c, want


@pytest.mark.parametrize("variant", S.PREP_VARIANTS)
def test_prep_cases_are_sensitive(variant):
    """Each directed case depends on what k_vict_prep computes: the hostname key has more than 256
    values, node i holding id i; the expected map changes when the pods that make the minimum are
    deleted from the reference's snapshot, again when those that make the runner-up are, and when the
    two topology filters are taken out of the profile."""
    c, want = _prep_not_vacuous(variant)
    fw = GpuFramework(Profile(), c["nodes"], c["existing"], pods_hint=[c["pod"]] + [p for p, _ in c["noms"]],
                      create_engine=False)
    key = fw.compiler.nkeys.key(S.HOST)
    assert len(fw.compiler.nkeys.vals[key]) == S.PREP_N > 256
    for i in (0, 44, 70, 200, 255, 256, 262, 300, 325, S.PREP_N - 1):
        assert fw.compiler.nkeys.val(key, S.prep_node_name(i)) == i
    for names in (c["key"], c["runner"]):
        if names:
            other = S.oracle_preempt(c["nodes"], S.without(c["existing"], names), c["pod"], noms=c["noms"])
            assert other[0] != want[0], (variant, names)
    plain = S.oracle_preempt(c["nodes"], c["existing"], c["pod"], noms=c["noms"], profile=S.no_topo_profile())
    assert plain[0] != want[0], variant
    if variant == "min_high_nominated":
        # the minimum's own node: its single matching pod goes only because the two nominated pods
        # lift the node above the runner-up (2 at id 262), which the verdict is then measured from
        assert want[0]["n325"] == (["w325-0"], 0)
        assert S.oracle_preempt(c["nodes"], c["existing"], c["pod"])[0]["n325"] == ([], 0)
    if variant == "affinity_wide":
        have = {p["spec"]["nodeName"] for p in c["existing"] if p["metadata"]["labels"].get("app") == "db"}
        assert len(have) > 256 and "n008" not in have and "n008" not in want[0]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", S.PREP_VARIANTS)
def test_prep_cases_match_oracle(variant):
    c, want = _prep_not_vacuous(variant)
    fw = GpuFramework(Profile(), c["nodes"], c["existing"], pods_hint=[c["pod"]] + [p for p, _ in c["noms"]])
    if c["noms"]:
        fw.set_nominated(c["noms"])
    got = S.gpu_answer(fw, c["pod"])
    assert got[0] == want[0], variant
    assert got[1] == want[1], (variant, got[1], want[1])
    fw.engine.close()


# ---------------------------------------------------------------- 3. deep node
@functools.lru_cache(maxsize=None)
def _deep_reference():
    c = S.deep_case()
    return c, [S.oracle_preempt(c["nodes"], c["existing"], p, pdbs=c["pdbs"]) for p in c["pods"]]


def _deep_not_vacuous():
    c, answers = _deep_reference()
    by = {NI.name(p): a[0] for p, a in zip(c["pods"], answers)}
    order = [NI.name(p) for p in sorted(c["existing"][:40], key=lambda p: (-PR.pod_priority(p), PR.pod_start_time(p, NOW)))]
    assert order != sorted(order)                           # MoreImportantPod order is not insertion order
    assert 15 <= len(by["half"]["deep"][0]) <= 25           # roughly half of the 40
    assert by["half"]["deep"][1] > 0                        # PDB violations among them
    # 9090 is held by d14 and d23 (one HostPortInfo entry): both go, though the CPU is there
    assert by["midport-only"]["deep"][0] == ["d14", "d23"]
    assert 5 < order.index("d14") < order.index("d23") < 35
    assert {"d14", "d23"} <= set(by["midport"]["deep"][0]) and len(by["midport"]["deep"][0]) > 5
    # 8080/TCP on the wildcard address and on 10.0.0.1; the UDP holder stays
    assert by["wild8080"]["deep"][0] == ["d17", "d05"]
    assert {"d17", "d05"} <= set(by["ip8080"]["deep"][0]) and "d12" not in by["ip8080"]["deep"][0]
    # 7070 on another address: its holder d30 is reprieved while others go
    assert by["reprieved-port"]["deep"][0] and "d30" not in by["reprieved-port"]["deep"][0]
    # 6060 is held by d29 and by a pod above the preemptor: the entry leaves with d29, and the pods
    # reprieved after d29's step see the port free (as many victims as without the port: d29 for one of them)
    assert "d29" in by["shadowed"]["deep"][0] and "d29" not in by["reprieved-port"]["deep"][0]
    assert len(by["shadowed"]["deep"][0]) == len(by["reprieved-port"]["deep"][0])
    assert by["shadowed"]["deep"][0].index("d29") == 0 and "keeper" not in by["shadowed"]["deep"][0]
    for a in answers:  # pick_one_node has nodes to choose from
        assert len(a[0]) >= 10
    return c, answers


def test_deep_reference_is_not_vacuous():
    _deep_not_vacuous()


@pytest.mark.gpu
def test_deep_node_matches_oracle():
    c, answers = _deep_not_vacuous()
    fw = GpuFramework(Profile(), c["nodes"], c["existing"], pods_hint=c["pods"])
    for pod, want in zip(c["pods"], answers):
        got = S.gpu_answer(fw, pod, c["pdbs"])
        assert got[0] == want[0], NI.name(pod)
        assert got[1] == want[1], (NI.name(pod), got[1], want[1])
    fw.engine.close()


# ---------------------------------------------------------------- 4. the 64-PDB edge
@functools.lru_cache(maxsize=None)
def _pdb_reference():
    c = S.pdb_case()
    return c, [S.oracle_preempt(c["nodes"], c["existing"], p, pdbs=c["pdbs"]) for p in c["pods"]]


def _pdb_not_vacuous():
    from kgpu.framework import _pdbs_of
    c, answers = _pdb_reference()
    used = sorted({j for p in c["existing"] for j in _pdbs_of(p, c["pdbs"])})
    assert len(used) == 64 and len(c["pdbs"]) == 66 and used[63] == c["bit63_index"]
    assert [NI.name(p) for p in c["existing"] if c["bit63_index"] in _pdbs_of(p, c["pdbs"])] == ["p04-1"]
    assert _pdbs_of(c["existing"][4 * 3 + 1], c["pdbs"]) == [c["bit63_index"]]  # its only PDB
    assert len({j for p in c["existing"] for j in _pdbs_of(p, c["pdbs"] + [c["extra"]])}) == 65
    less = [b for k, b in enumerate(c["pdbs"]) if k != c["bit63_index"]]
    for pod, want in zip(c["pods"], answers):
        assert "p04-1" in want[0][c["bit63_node"]][0] and want[0][c["bit63_node"]][1] > 0
        other = S.oracle_preempt(c["nodes"], c["existing"], pod, pdbs=less)
        assert other[0] != want[0]
        assert other[0][c["bit63_node"]][1] == want[0][c["bit63_node"]][1] - 1
    # "pair" allows one disruption and selects p06-0 and p06-2: the second one violates
    assert answers[0][0]["p06"] == (["p06-0", "p06-2", "p06-1"], 1)
    return c, answers


def test_pdb_reference_is_not_vacuous():
    _pdb_not_vacuous()


@pytest.mark.gpu
def test_64_selecting_pdbs_then_65():
    c, answers = _pdb_not_vacuous()
    fw = GpuFramework(Profile(), c["nodes"], c["existing"], pods_hint=c["pods"])
    for pod, want in zip(c["pods"], answers):
        got = S.gpu_answer(fw, pod, c["pdbs"])
        assert got[0] == want[0], NI.name(pod)
        assert got[0][c["bit63_node"]][1] > 0
        assert got[1] == want[1], (NI.name(pod), got[1], want[1])
    with pytest.raises(ValueError):
        fw.select_nodes_for_preemption(c["pods"][0], c["pdbs"] + [c["extra"]], NOW)
    got = S.gpu_answer(fw, c["pods"][0], c["pdbs"])  # the engine stays usable
    assert got == answers[0]
    fw.engine.close()


# ---------------------------------------------------------------- 5. engine-written state
def _batch_pods(kind):
    if kind == "generic":
        return S.generic_pods(60), S.generic_preemptors()
    if kind == "topology":
        return S.topo_pods(60), S.topo_preemptors()
    return S.interleave(S.generic_pods(30), S.topo_pods(30)), S.generic_preemptors() + S.topo_preemptors()


def _place(fw, orc, pods, mode, seq0):
    """Schedule `pods` on both sides (mode "batch": one fw.schedule() call; "cycle": fw.cycle(assume=True)
    per pod) and assert the hosts equal.  fw None: the oracle alone."""
    res = fw.schedule(pods, first_seq=seq0) if fw is not None and mode == "batch" else None
    placed = 0
    for i, pod in enumerate(pods):
        host, _, _ = orc.cycle(pod, seq0 + i)
        placed += host is not None
        if fw is None:
            continue
        got = fw.host_of(int(res[i]["node"])) if mode == "batch" else fw.cycle(pod, assume=True, seq=seq0 + i).host
        assert got == host, (mode, i, NI.name(pod), got, host)
    return placed


def _compare(fw, orc, pod, pdbs=()):
    want = orc.preempt_map(pod, pdbs)
    assert want is not None, NI.name(pod)
    if fw is not None:
        got = S.gpu_answer(fw, pod, pdbs)
        assert got[0] == want[0], NI.name(pod)
        assert got[1] == want[1], (NI.name(pod), got[1], want[1])
    return want


def _victims(want):
    return {v for vs, _ in want[0].values() for v in vs}


def _check_state_answers(kind, orc, batch, answers):
    """What the oracle must have decided for the case to test engine-written state."""
    placed = set(orc.placed)
    for name, want in answers.items():
        assert len(want[0]) >= 1, (kind, name)
    if kind in ("generic", "mixed"):
        assert _victims(answers["pre-big"]) & placed
        # host port 8080: the preemptor needs 100m only, so a batch-placed holder goes for its port alone
        holders = {NI.name(p) for p in batch if p["spec"]["containers"][0].get("ports")} & placed
        assert _victims(answers["pre-port"]) & holders
        gpu = {NI.name(p) for p in batch if S.GPU_RES in p["spec"]["containers"][0]["resources"]["requests"]} & placed
        assert _victims(answers["pre-gpu"]) & gpu
    if kind in ("topology", "mixed"):
        def with_term(field, app):
            out = set()
            for p in batch:
                ts = ((p["spec"].get("affinity") or {}).get(field) or {}).get("requiredDuringSchedulingIgnoredDuringExecution")
                if ts and ts[0]["labelSelector"]["matchLabels"] == {"app": app}:
                    out.add(NI.name(p))
            return out & placed
        # a batch-placed pod's required anti-affinity term rejects the preemptor (100m: nothing else does)
        assert _victims(answers["pre-exa"]) and _victims(answers["pre-exa"]) <= with_term("podAntiAffinity", "pre")
        assert _victims(answers["pre-exa-big"]) & with_term("podAntiAffinity", "pre")
        # the preemptor's own anti-affinity matches batch-placed pods
        web = {NI.name(p) for p in batch if p["metadata"]["labels"]["app"] == "web"} & placed
        assert _victims(answers["pre-anti"]) and _victims(answers["pre-anti"]) <= web
        assert _victims(answers["pre-spread"]) & placed


def _run_state(kind, mode, gpu):
    nodes, existing = S.flow_nodes(), S.flow_snapshot_pods()
    batch, pres = _batch_pods(kind)
    orc = S.OracleFlow(nodes, existing)
    fw = GpuFramework(Profile(), nodes, existing, pods_hint=_hint(batch, pres)) if gpu else None
    assert _place(fw, orc, batch, mode, 0) >= len(batch) - 5
    answers = {NI.name(p): _compare(fw, orc, p) for p in pres}
    _check_state_answers(kind, orc, batch, answers)
    if fw is not None:
        assert fw.next_slot == len(existing) + len(orc.placed)
        fw.engine.close()


STATE_CASES = [("generic", "batch"), ("topology", "batch"), ("mixed", "batch"), ("mixed", "cycle")]


@pytest.mark.parametrize("kind,mode", STATE_CASES[:3])
def test_state_reference_is_not_vacuous(kind, mode):
    _run_state(kind, mode, gpu=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode", STATE_CASES)
def test_victims_the_engine_placed(kind, mode):
    """Preemption over pods kgpu_schedule_batch ("batch") or kgpu_schedule_one ("cycle") assumed: their
    pod-table rows (namespace, labels, own term classes), the node rows, host-port columns and
    histograms the assume wrote, and the slots GpuFramework numbers them by."""
    _run_state(kind, mode, gpu=True)


def _run_forget(gpu):
    nodes, existing = S.flow_nodes(), S.flow_snapshot_pods()
    batch, pres = _batch_pods("mixed")
    later = S.generic_pods(6, tag="h") + S.topo_pods(6, tag="u")
    orc = S.OracleFlow(nodes, existing)
    fw = GpuFramework(Profile(), nodes, existing, pods_hint=_hint(batch, pres, later)) if gpu else None
    _place(fw, orc, batch, "batch", 0)
    before = {NI.name(p): _compare(fw, orc, p) for p in pres}
    # forget one victim of each kind of reason: resources, host port, a term of its own, the preemptor's term
    gone = []
    for name in ("pre-big", "pre-port", "pre-exa", "pre-anti"):
        v = sorted(_victims(before[name]) & set(orc.placed) - set(gone))
        assert v, name
        gone.append(v[0])
    for name in gone:
        _, host = orc.placed[name]
        orc.forget(name)
        if fw is not None:
            k = [i for i, (p, _) in enumerate(fw.node_pods[host]) if NI.name(p) == name]
            assert len(k) == 1
            fw.engine.forget(fw.node_pods[host].pop(k[0])[1])
    after = {NI.name(p): _compare(fw, orc, p) for p in pres}
    for name in after:
        assert not _victims(after[name]) & set(gone), name
    assert any(after[n] != before[n] for n in after)
    # placements after the forgets take new slots; preemption then names them by those slots
    _place(fw, orc, later[:6], "batch", len(batch))
    _place(fw, orc, later[6:], "cycle", len(batch) + 6)
    again = {NI.name(p): _compare(fw, orc, p) for p in pres}
    assert any(_victims(w) & {NI.name(p) for p in later} for w in again.values())
    if fw is not None:
        assert fw.next_slot == len(existing) + len(orc.placed) + len(gone)
        fw.engine.close()


def test_forget_reference_is_not_vacuous():
    _run_forget(gpu=False)


@pytest.mark.gpu
def test_forgotten_pod_is_no_victim():
    """kgpu_forget_pod on placed pods: they stop being victims, their resources, ports and histogram
    contributions leave the adjusted view, and later placements keep GpuFramework.next_slot's numbering."""
    _run_forget(gpu=True)


def _run_loop(gpu):
    """cycle -> FitError -> preempt -> victims removed -> preemptor nominated -> next cycle, three
    preemptors in a row, on a cluster a mixed batch filled."""
    nodes, existing = S.flow_nodes(cpu="2"), S.flow_snapshot_pods(every=3)
    batch = S.interleave(S.generic_pods(45), S.topo_pods(45))
    pres = [S.mkpod("loop-a", cpu="1900m", prio=10000),
            S.required(S.mkpod("loop-b", cpu="1200m", prio=10000, labels={"app": "pre"}), "podAntiAffinity",
                       [S.term(S.HOST, {"app": "web"})]),
            S.mkpod("loop-c", cpu="1900m", prio=10000, ports=[(8080, "TCP", "")])]
    pdbs = [{"namespace": "default", "selector": {"matchLabels": {"app": "gen"}}, "disruptionsAllowed": 1}]
    orc = S.OracleFlow(nodes, existing)
    fw = GpuFramework(Profile(), nodes, existing, pods_hint=_hint(batch, pres)) if gpu else None
    _place(fw, orc, batch, "batch", 0)
    seq = len(batch)
    snapshot_names = {NI.name(p) for p in existing}
    forgotten = terminating = scheduled = 0
    for pre in pres:
        host, codes, err = orc.cycle(pre, seq)
        assert host is None and err is not None, NI.name(pre)  # FitError: preemption is the way in
        node, victims, _ = PR.preempt(orc.gs, pre, err, pdbs, orc.nominator, NOW)
        assert node and victims, NI.name(pre)
        names = [NI.name(v) for v in victims]
        if fw is not None:
            cr = fw.cycle(pre, assume=False, seq=seq)
            assert cr.host is None and {n: s[0] for n, s in cr.statuses.items()} == codes
            gnode, gvictims, _ = fw.preempt(pre, cr.statuses, pdbs, NOW)
            assert (gnode, [NI.name(v) for v in gvictims]) == (node, names), NI.name(pre)
        seq += 1
        # the victims leave: assumed ones are forgotten; a snapshot pod only starts terminating
        for name in names:
            if name in snapshot_names:
                for pi in orc.snap.get(node).pods:
                    if NI.name(pi.pod) == name:
                        pi.pod["metadata"]["deletionTimestamp"] = "2020-01-01T00:00:00Z"  # the mirror's object too
                terminating += 1
                continue
            orc.forget(name)
            forgotten += 1
            if fw is not None:
                k = [i for i, (p, _) in enumerate(fw.node_pods[node]) if NI.name(p) == name]
                fw.engine.forget(fw.node_pods[node].pop(k[0])[1])
        orc.nominator.add(pre, node)
        if fw is not None:
            fw.set_nominated(fw.nominated + [(pre, node)])
        # the preemptor's next cycle, under the nominator
        host, codes, _ = orc.cycle(pre, seq)
        scheduled += host is not None
        if fw is not None:
            cr = fw.cycle(pre, assume=True, seq=seq)
            assert cr.host == host, (NI.name(pre), cr.host, host)
            assert {n: s[0] for n, s in cr.statuses.items()} == codes, NI.name(pre)
            assert sorted(NI.name(p) for p, _ in fw.nominated) == sorted(
                NI.name(p) for ps in orc.nominator.by_node.values() for p in ps)
        seq += 1
    assert forgotten >= 2 and scheduled >= 1, (forgotten, terminating, scheduled)
    if fw is not None:
        fw.engine.close()


def test_loop_reference_is_not_vacuous():
    _run_loop(gpu=False)


@pytest.mark.gpu
def test_preempt_nominate_cycle_loop():
    _run_loop(gpu=True)
