"""Clusters and reference-side helpers of tests/test_preemption_scale.py (test infrastructure).

Everything here runs on the CPU: the generators, the oracle call (the steps of test_preemption's
_oracle_preempt with the profile and the snapshot as parameters) and the counts the non-vacuity
conditions are stated in."""
import copy
import random

import gen_random
from gen_random import HOST, ZONE, REGION
from oracle.refsched import framework as F
from oracle.refsched import nodeinfo as NI
from oracle.refsched import plugins as P
from oracle.refsched import preemption as PR

NOW = 2_000_000_000 * 1_000_000_000
TOPO_FILTERS = ("PodTopologySpread", "InterPodAffinity")


def no_topo_profile(**kw):
    """The default profile without the PodTopologySpread and InterPodAffinity filters."""
    return F.Profile(filters=[f for f in F.DEFAULT_FILTERS if f not in TOPO_FILTERS], **kw)


def oracle_preempt(nodes, existing, pod, services=(), rss=(), pdbs=(), noms=(), profile=None, snap=None):
    """selectNodesForPreemption over nodesWherePreemptionMightHelp + pickOneNodeForPreemption on the
    oracle: ({node: ([victim names in Victims.Pods order], numPDBViolations)}, picked node), None when
    the pod's PreFilter rejects it.  snap: a live oracle snapshot instead of (nodes, existing)."""
    if snap is None:
        snap = NI.Snapshot(nodes, existing)
    fw = F.Framework(profile or F.Profile(), F.Handle(snap, services, (), rss))
    nominator = PR.Nominator()
    for p, nn in noms:
        nominator.add(p, nn)
    state = {}
    if fw.run_prefilter(state, pod) is not None:
        return None
    potential = []
    for ni in snap.list:
        _, _, status = PR.pod_passes_filters_on_node(fw, nominator, state, pod, ni)
        if P.code_of(status) != P.UNRESOLVABLE:
            potential.append(ni)
    n2v = PR.select_nodes_for_preemption(fw, nominator, state, pod, potential, list(pdbs), NOW)
    return ({n: ([NI.name(p) for p in v], nv) for n, (v, nv) in n2v.items()},
            PR.pick_one_node_for_preemption(n2v, NOW))


def gpu_answer(fw, pod, pdbs=()):
    """The product's answer in the oracle_preempt form."""
    n2v, pick = fw.select_nodes_for_preemption(pod, pdbs, NOW)
    return {n: ([NI.name(p) for p in v], nv) for n, (v, nv) in n2v.items()}, pick


def counts(existing, pod, n2v):
    """Of one preemptor's reference map: (candidate nodes with a victim, candidate nodes with two or
    more, victims, reprieved pods: lower-priority pods on candidate nodes left off the victim list)."""
    prio = PR.pod_priority(pod)
    lower = {}
    for p in existing:
        if PR.pod_priority(p) < prio:
            nn = p["spec"].get("nodeName", "")
            lower[nn] = lower.get(nn, 0) + 1
    with_v = sum(1 for v, _ in n2v.values() if v)
    multi = sum(1 for v, _ in n2v.values() if len(v) >= 2)
    victims = sum(len(v) for v, _ in n2v.values())
    reprieved = sum(lower.get(n, 0) - len(v) for n, (v, _) in n2v.items())
    return with_v, multi, victims, reprieved


def without(existing, names):
    names = set(names)
    return [p for p in existing if NI.name(p) not in names]


def start(day, sec=1):
    return "2019-01-%02dT01:%02d:%02dZ" % (day, sec // 60, sec % 60)


# ---------------------------------------------------------------- 1. size matrix
PRIOS = [-100, 0, 0, 100, 1000]
SIZES = [63, 64, 65, 130, 300]
SEEDS = {False: (1, 2), True: (1, 2)}
N_PREEMPTORS = 4


def _fix_keys(r, spec):
    """Topology keys every node carries: "nokey" and the region label (half of the nodes) make a
    required term or a DoNotSchedule constraint unresolvable nearly everywhere."""
    for t in spec.get("topologySpreadConstraints") or []:
        if t["topologyKey"] == REGION:
            t["topologyKey"] = r.choice([ZONE, HOST])
    for field in ("podAffinity", "podAntiAffinity"):
        sub = (spec.get("affinity") or {}).get(field) or {}
        for t in sub.get("requiredDuringSchedulingIgnoredDuringExecution") or []:
            if t["topologyKey"] in ("nokey", REGION):
                t["topologyKey"] = r.choice([ZONE, HOST])


def scale_scenario(seed, topo, n_nodes):
    """test_preemption's _scenario at n_nodes nodes with 5 existing pods per node.  The topology
    variant is shaped so that preemption has something to decide (the generator scaled up unchanged
    yields next to no candidate): 4-CPU / 8-GiB nodes, every node in a zone, no nodeSelector / required
    node affinity on the preemptors, their priority above every existing pod, their required terms and
    hard constraints on keys every node carries, and existing pods' required anti-affinity thinned out
    (a single matching term anywhere in a zone rules the whole zone out for good)."""
    r = random.Random(7000 + seed)
    n_existing = 5 * n_nodes
    if topo:
        nodes, existing, pods, services, rss = gen_random.topo_cluster(seed, n_nodes=n_nodes, n_existing=n_existing,
                                                                       n_pods=N_PREEMPTORS)
        for i, n in enumerate(nodes):
            n["status"]["allocatable"].update({"cpu": "4", "memory": "8Gi", "pods": str(r.choice([4, 6, 110]))})
            n["metadata"]["labels"].setdefault(ZONE, "z%d" % (i % 3))
    else:
        nodes, existing, pods = gen_random.cluster(seed, n_nodes=n_nodes, n_existing=n_existing, n_pods=N_PREEMPTORS)
        services, rss = [], []
    for p in existing + pods:
        p["spec"]["priority"] = r.choice(PRIOS)
        if r.random() < 0.7:
            p["status"] = {"startTime": "2019-01-0%dT01:01:01Z" % r.randrange(1, 8)}
    for p in pods:
        p["spec"]["priority"] = r.choice([2000, 3000]) if topo else r.choice([500, 1000, 2000])
        p["spec"].pop("nodeName", None)
    if topo:
        for p in existing:
            anti = (p["spec"].get("affinity") or {}).get("podAntiAffinity") or {}
            if "requiredDuringSchedulingIgnoredDuringExecution" in anti and r.random() < 0.9:
                del anti["requiredDuringSchedulingIgnoredDuringExecution"]
            _fix_keys(r, p["spec"])
        for p in pods:
            p["spec"].pop("nodeSelector", None)
            (p["spec"].get("affinity") or {}).pop("nodeAffinity", None)
            p["metadata"].pop("deletionTimestamp", None)
            _fix_keys(r, p["spec"])
    pdbs = []
    for j in range(r.choice([1, 2, 3])):
        sel = r.choice([{"matchLabels": {"app": r.choice(["a", "b", "web", "db"])}},
                        {"matchExpressions": [{"key": "app", "operator": "Exists"}]}, {}])
        pdbs.append({"namespace": r.choice(["default", "default", "other"]), "selector": sel,
                     "disruptionsAllowed": r.choice([0, 1, 2])})
    noms = []
    names = [n["metadata"]["name"] for n in nodes]
    for j in range(r.choice([2, 4])):
        p = gen_random.rpod(r, 5000 + j, names, allow_node_name=False)
        if topo:
            gen_random._topo_spec(r, p["spec"], p["metadata"], p_tsc=0.0, p_aff=0.4)
            _fix_keys(r, p["spec"])
        p["spec"]["priority"] = r.choice([0, 1000, 3000])
        noms.append((p, r.choice(names)))
    return nodes, existing, pods, services, rss, pdbs, noms


def matrix_cases():
    """(id, seed, topo, n_nodes, run_all_filters) of every parametrized case of the size matrix."""
    out = []
    for topo in (False, True):
        kind = "topology" if topo else "resources"
        for n in SIZES:
            for seed in SEEDS[topo]:
                out.append(("%s-%d-s%d" % (kind, n, seed), seed, topo, n, False))
    for seed in SEEDS[True]:
        out.append(("topology-130-s%d-runall" % seed, seed, True, 130, True))
    return out


def matrix_reference(seed, topo, n_nodes, run_all):
    """The oracle's answers of one case and the sums conditions (a)-(d) are stated in:
    (scenario, [answer or None per preemptor], {"with_victims", "multi", "victims", "reprieved",
    "topo_decides"})."""
    sc = scale_scenario(seed, topo, n_nodes)
    nodes, existing, pods, services, rss, pdbs, noms = sc
    answers = []
    tot = {"candidates": 0, "with_victims": 0, "multi": 0, "victims": 0, "reprieved": 0, "topo_decides": 0}
    for pod in pods:
        want = oracle_preempt(nodes, existing, pod, services, rss, pdbs, noms,
                              profile=F.Profile(run_all_filters=run_all))
        answers.append(want)
        if want is None:
            continue
        w, m, v, rp = counts(existing, pod, want[0])
        tot["candidates"] += len(want[0])
        tot["with_victims"] += w
        tot["multi"] += m
        tot["victims"] += v
        tot["reprieved"] += rp
        if topo:
            plain = oracle_preempt(nodes, existing, pod, services, rss, pdbs, noms,
                                   profile=no_topo_profile(run_all_filters=run_all))
            tot["topo_decides"] += plain is None or plain[0] != want[0]
    return sc, answers, tot


def assert_not_vacuous(tot, topo, case):
    assert tot["with_victims"] >= 8, (case, tot)      # (a)
    assert tot["multi"] >= 1, (case, tot)             # (b)
    assert tot["reprieved"] >= 1, (case, tot)         # (c)
    if topo:
        assert tot["topo_decides"] >= 1, (case, tot)  # (d)


# ---------------------------------------------------------------- hand-built objects
def mknode(name, cpu="4", mem="8Gi", pods="110", zone=None, scalars=None, labels=None):
    al = {"cpu": cpu, "memory": mem, "pods": pods}
    al.update(scalars or {})
    lb = {HOST: name}
    if zone is not None:
        lb[ZONE] = zone
    lb.update(labels or {})
    return {"metadata": {"name": name, "labels": lb}, "spec": {}, "status": {"allocatable": al}}


def mkpod(name, cpu="100m", mem="64Mi", prio=0, labels=None, node=None, day=None, sec=1, ports=(), ns="default",
          scalars=None):
    """ports: (hostPort, protocol, hostIP) triples; day / sec: status.startTime (None: not started)."""
    req = {"cpu": cpu, "memory": mem}
    req.update(scalars or {})
    c = {"name": "c", "image": "img0", "resources": {"requests": req}}
    if ports:
        c["ports"] = [{"containerPort": 80, "hostPort": hp, "protocol": proto, "hostIP": ip} for hp, proto, ip in ports]
    spec = {"containers": [c], "priority": prio}
    if node is not None:
        spec["nodeName"] = node
    p = {"metadata": {"name": name, "namespace": ns, "uid": "u-" + name, "labels": dict(labels or {})}, "spec": spec}
    if day is not None:
        p["status"] = {"startTime": start(day, sec)}
    return p


def hard(key, skew, sel):
    return {"maxSkew": skew, "topologyKey": key, "whenUnsatisfiable": "DoNotSchedule",
            "labelSelector": {"matchLabels": sel}}


def term(key, sel):
    return {"labelSelector": {"matchLabels": sel}, "topologyKey": key}


def required(pod, field, terms):
    pod["spec"].setdefault("affinity", {}).setdefault(field, {})["requiredDuringSchedulingIgnoredDuringExecution"] = terms
    return pod


# ---------------------------------------------------------------- 2. k_vict_prep: more than 256 topology values
# 330 nodes, not the 300-320 first planned: k_vict_prep's thread t reads value ids t and t + 256, so ids
# 256..319 all sit in wave 0; a minimum and a runner-up that are both >= 256 and in different waves
# need an id >= 320.
PREP_N = 330
PREP_VARIANTS = ["min_high_nominated", "tie_low_high", "tie_waves", "shared_pair", "affinity_wide"]


def prep_node_name(i):
    return "n%03d" % i


def prep_case(variant):
    """{"nodes", "existing", "pod", "noms", "key": [names of the pods that make the minimum],
    "runner": [names of the pods that make the runner-up]}.  Node i is value id i of the hostname key
    (the compiler numbers a key's values in first-seen order over the nodes as registered; the CPU test
    checks it)."""
    nodes = [mknode(prep_node_name(i), cpu="64", mem="256Gi", zone="z%d" % (i % 3)) for i in range(PREP_N)]
    if variant == "affinity_wide":
        return _prep_affinity(nodes)
    # matching pods per node: 3 or 4, but for the minimum (1) and the runner-up (2)
    low = {"min_high_nominated": {325: 1, 262: 2},            # t = 69 (wave 1) and t = 6 (wave 0), second stride
           "tie_low_high": {44: 1, 300: 1, 290: 1, 270: 2},   # 44 and 300 in one thread, 290 in another
           "tie_waves": {70: 1, 200: 1, 262: 2},              # waves 1 and 3
           "shared_pair": {325: 1, 262: 2}}[variant]
    existing = []
    for i in range(PREP_N):
        for j in range(low.get(i, 3 + i % 2)):
            lb = {"app": "web"}
            if variant == "shared_pair" and j == 0 and i % 4 == 0:
                lb["tier"] = "fe"
            existing.append(mkpod("w%03d-%d" % (i, j), prio=[0, 50, 100][(i + j) % 3], labels=lb, node=prep_node_name(i),
                                  day=1 + (i * 7 + j * 3) % 9, sec=j))
        if i % 5 == 0:  # a lower-priority pod the constraint does not count: always reprieved
            existing.append(mkpod("d%03d" % i, prio=10, labels={"app": "db"}, node=prep_node_name(i), day=2))
    pod = mkpod("pre", prio=1000, labels={"app": "web"})
    pod["spec"]["topologySpreadConstraints"] = [hard(HOST, 1, {"app": "web"})]
    noms = []
    if variant == "shared_pair":
        pod["metadata"]["labels"]["tier"] = "fe"
        pod["spec"]["topologySpreadConstraints"] = [hard(HOST, 1, {"app": "web"}), hard(HOST, 2, {"tier": "fe"}),
                                                    hard(ZONE, 4, {"app": "web"})]
    # nominated matching pods at or above the preemptor's priority: with them the node's own count passes
    # the runner-up, so the verdict there is taken from the minimum over the other pairs
    at = {"min_high_nominated": 325, "tie_low_high": 300, "tie_waves": 200, "shared_pair": 325}[variant]
    for k in range(2 if variant != "tie_low_high" else 1):
        noms.append((mkpod("nom%d" % k, prio=2000, labels={"app": "web"}), prep_node_name(at)))
    mn = min(low.values())
    key = ["w%03d-%d" % (i, j) for i, c in low.items() if c == mn for j in range(c)]
    runner = ["w%03d-%d" % (i, j) for i, c in low.items() if c != mn for j in range(c)]
    return {"nodes": nodes, "existing": existing, "pod": pod, "noms": noms, "key": key, "runner": runner}


def _prep_affinity(nodes):
    """Required affinity on hostname whose topologyToMatchedAffinityTerms holds 289 non-zero entries.
    The preemptor matches its own term: a node without a matching pod is a candidate exactly when the
    map is empty (filtering.go:376-388), so a count that came out 0 would show on every eighth node."""
    for n in nodes:
        n["status"]["allocatable"].update({"cpu": "2", "memory": "8Gi"})
    existing = []
    key, runner = [], []
    for i in range(PREP_N):
        nn = prep_node_name(i)
        if i % 8:
            stays = i % 3 == 0
            existing.append(mkpod("db%03d" % i, cpu="500m", prio=5000 if stays else 20, labels={"app": "db"}, node=nn,
                                  day=1 + i % 7))
            if stays and i >= 256:
                key.append("db%03d" % i)
        existing.append(mkpod("f%03d-0" % i, cpu="300m", prio=50, labels={"app": "fill"}, node=nn, day=3))
        existing.append(mkpod("f%03d-1" % i, cpu="600m", prio=[10, 60][i % 2], labels={"app": "fill"}, node=nn, day=4))
    pod = required(mkpod("pre", cpu="1000m", prio=1000, labels={"app": "db"}), "podAffinity", [term(HOST, {"app": "db"})])
    return {"nodes": nodes, "existing": existing, "pod": pod, "noms": [], "key": key, "runner": runner}


# ---------------------------------------------------------------- 3. deep node
def deep_case():
    """{"nodes", "existing", "pdbs", "pods": preemptors}: node "deep" with 40 lower-priority pods (its
    CPU all but full), 10 ordinary nodes in pairs that differ in their pods' start times only."""
    nodes = [mknode("deep", cpu="8200m", mem="64Gi", zone="z0")]
    nodes += [mknode("o%d" % i, cpu="8200m", mem="64Gi", zone="z%d" % (i % 3)) for i in range(10)]
    existing = []
    ports = {5: [(8080, "TCP", "")], 17: [(8080, "TCP", "10.0.0.1")], 12: [(8080, "UDP", "")],
             14: [(9090, "TCP", "")], 23: [(9090, "TCP", "")], 30: [(7070, "TCP", "10.0.0.1")],
             29: [(6060, "TCP", "")]}
    for i in range(40):
        prio = 100 if i == 30 else [0, 10, 50, 100][(3 * i) % 4]
        existing.append(mkpod("d%02d" % i, cpu="200m", prio=prio, labels={"app": "abc"[i % 3]}, node="deep",
                              day=1 + (i * 5) % 9, sec=i, ports=ports.get(i, ())))
    # above every preemptor, holding the HostPortInfo entry d29 holds too: removing d29 removes the entry
    # (types.go:726-756, a set), so the port is free from d29's reprieve step on though "keeper" stays
    existing.append(mkpod("keeper", cpu="0m", mem="0Mi", prio=5000, node="deep", day=1, ports=[(6060, "TCP", "")]))
    for i in range(10):
        for j in range(8):
            existing.append(mkpod("o%d-%d" % (i, j), cpu="1000m", prio=[0, 0, 10, 10, 50, 50, 100, 100][j],
                                  labels={"app": "ab"[j % 2]}, node="o%d" % i, day=1 + (i // 2 + j) % 5, sec=i % 2 + 2 * j,
                                  ports=[(9090, "TCP", "")] if (i, j) == (3, 6) else ()))
    pdbs = [{"namespace": "default", "selector": {"matchLabels": {"app": "a"}}, "disruptionsAllowed": 3},
            {"namespace": "default", "selector": {"matchLabels": {"app": "b"}}, "disruptionsAllowed": 0}]
    pods = [mkpod("half", cpu="4000m", prio=1000),
            mkpod("midport", cpu="2100m", prio=1000, ports=[(9090, "TCP", "")]),
            mkpod("midport-only", cpu="100m", prio=1000, ports=[(9090, "TCP", "10.0.0.9")]),
            mkpod("reprieved-port", cpu="2100m", prio=1000, ports=[(7070, "TCP", "10.0.0.2")]),
            mkpod("wild8080", cpu="100m", prio=1000, ports=[(8080, "TCP", "")]),
            mkpod("ip8080", cpu="2100m", prio=1000, ports=[(8080, "TCP", "10.0.0.1")]),
            mkpod("shadowed", cpu="2100m", prio=1000, ports=[(6060, "TCP", "")]),
            mkpod("below-some", cpu="4000m", prio=60, ports=[(8080, "UDP", "")])]
    return {"nodes": nodes, "existing": existing, "pdbs": pdbs, "pods": pods}


# ---------------------------------------------------------------- 4. the 64-PDB edge
def pdb_case():
    """70 nodes of three 1-CPU pods each (2.5 CPU on even nodes, 3 on odd ones).  66 PDBs, 64 of which
    select a potential victim: the last one (bit 63 of the engine's masks) allows no disruption and
    selects pod p04-1 alone; "pair" allows one and selects two pods of node p06.
    {"nodes", "existing", "pdbs", "extra": a 65th selecting PDB, "pods", "bit63_node", "bit63_index"}."""
    nodes = [mknode("p%02d" % i, cpu="2500m" if i % 2 == 0 else "3000m", zone="z%d" % (i % 3)) for i in range(70)]
    existing = []
    for i in range(70):
        for j in range(3):
            g = "g%d" % ((3 * i + j) % 62)
            if (i, j) == (4, 1):
                g = "g63"
            elif i == 6 and j != 1:
                g = "pair"
            existing.append(mkpod("p%02d-%d" % (i, j), cpu="1000m", prio=[0, 10, 20][j], labels={"g": g, "all": "x"},
                                  node="p%02d" % i, day=1 + (i + j) % 7))

    def pdb(g, allowed):
        return {"namespace": "default", "selector": {"matchLabels": {"g": g}}, "disruptionsAllowed": allowed}

    pdbs = [pdb("g%d" % k, k % 3) for k in range(62)]
    pdbs.insert(10, pdb("nobody", 0))
    pdbs.insert(40, {"namespace": "elsewhere", "selector": {"matchLabels": {"all": "x"}}, "disruptionsAllowed": 0})
    pdbs += [pdb("pair", 1), pdb("g63", 0)]
    extra = {"namespace": "default", "selector": {"matchLabels": {"all": "x"}}, "disruptionsAllowed": 5}
    pods = [mkpod("two-cpu", cpu="2000m", prio=1000), mkpod("one-cpu", cpu="1000m", prio=15)]
    return {"nodes": nodes, "existing": existing, "pdbs": pdbs, "extra": extra, "pods": pods, "bit63_node": "p04",
            "bit63_index": len(pdbs) - 1}


# ---------------------------------------------------------------- 5. engine-written state
FLOW_N = 70
GPU_RES = "example.com/gpu"


def flow_nodes(cpu="4"):
    return [mknode("f%02d" % i, cpu=cpu, zone="z%d" % (i % 3), scalars={GPU_RES: "2"} if i % 5 == 0 else None)
            for i in range(FLOW_N)]


def flow_snapshot_pods(every=1):
    return [mkpod("s%02d" % i, cpu="1000m", prio=[0, 100, 5000][(i // every) % 3], labels={"app": "base"}, node="f%02d" % i,
                  day=1 + i % 5) for i in range(0, FLOW_N, every)]


def generic_pods(n, tag="g"):
    """Low-priority pods without topology terms; every tenth holds host port 8080, some ask for the
    extended resource."""
    out = []
    for k in range(n):
        out.append(mkpod("%s%02d" % (tag, k), cpu=["500m", "1000m", "1500m"][k % 3], prio=10 * (k % 2), labels={"app": "gen"},
                         day=(1 + k % 6) if k % 2 else None, ports=[(8080, "TCP", "")] if k % 10 == 0 else (),
                         scalars={GPU_RES: "1"} if k % 12 == 5 else None))
    return out


def topo_pods(n, tag="t"):
    """Low-priority pods with spread constraints and required (anti-)affinity."""
    out = []
    for k in range(n):
        app = ["web", "db", "cache"][k % 3]
        p = mkpod("%s%02d" % (tag, k), cpu="500m", prio=10 * (k % 2), labels={"app": app}, day=(1 + k % 6) if k % 2 else None)
        kind = k % 4
        if kind == 0:
            p["spec"]["topologySpreadConstraints"] = [hard(ZONE, 2, {"app": app})]
        elif kind == 1:
            required(p, "podAntiAffinity", [term(HOST, {"app": app})])
        elif kind == 2:  # rejects a later pod labelled app=pre on its node
            required(p, "podAntiAffinity", [term(HOST, {"app": "pre"})])
        else:
            required(p, "podAffinity", [term(ZONE, {"app": "base"})])
            p["spec"]["topologySpreadConstraints"] = [dict(hard(HOST, 1, {"app": app}), whenUnsatisfiable="ScheduleAnyway")]
        out.append(p)
    return out


def generic_preemptors():
    return [mkpod("pre-big", cpu="3500m", prio=10000),
            mkpod("pre-port", cpu="100m", prio=10000, ports=[(8080, "TCP", "")]),
            mkpod("pre-gpu", cpu="3200m", prio=10000, scalars={GPU_RES: "2"}),
            mkpod("pre-mid", cpu="3500m", prio=5)]


def topo_preemptors():
    anti = required(mkpod("pre-anti", cpu="500m", prio=10000, labels={"app": "x"}), "podAntiAffinity",
                    [term(HOST, {"app": "web"})])
    spread = mkpod("pre-spread", cpu="3200m", prio=10000, labels={"app": "db"})
    spread["spec"]["topologySpreadConstraints"] = [hard(HOST, 1, {"app": "db"})]
    return [mkpod("pre-exa", cpu="100m", prio=10000, labels={"app": "pre"}), anti, spread,
            mkpod("pre-exa-big", cpu="3500m", prio=10000, labels={"app": "pre"})]


def interleave(a, b):
    out = []
    for x, y in zip(a, b):
        out += [x, y]
    return out


class OracleFlow:
    """The reference side of an engine-written-state test: a live snapshot the scheduleOne loop assumes
    into (NodeInfo.AddPod), a nominator, and preemption over that snapshot."""

    def __init__(self, nodes, existing):
        self.snap = NI.Snapshot(nodes, existing)
        self.fw = F.Framework(F.Profile(), F.Handle(self.snap))
        self.nominator = PR.Nominator()
        self.gs = F.GenericScheduler(self.fw, self.nominator)
        self.placed = {}  # pod name -> (placed pod, host)

    def cycle(self, pod, seq):
        """(host or None, {node: status code} of the infeasible nodes); assumes a placed pod."""
        try:
            r = self.gs.schedule(pod, seq)
        except F.FitError as e:
            return None, {n: st.code for n, (_, st) in e.statuses.items()}, e
        placed = copy.deepcopy(pod)
        placed["spec"]["nodeName"] = r.host
        self.snap.get(r.host).add_pod(placed)
        self.nominator.delete(pod)
        self.placed[NI.name(pod)] = (placed, r.host)
        return r.host, {n: st.code for n, (_, st) in r.statuses.items()}, None

    def forget(self, name):
        placed, host = self.placed.pop(name)
        self.snap.get(host).remove_pod(placed)

    def pods(self):
        return [pi.pod for ni in self.snap.list for pi in ni.pods]

    def preempt_map(self, pod, pdbs=()):
        noms = [(p, nn) for nn, ps in self.nominator.by_node.items() for p in ps]
        return oracle_preempt(None, None, pod, pdbs=pdbs, noms=noms, snap=self.snap)
