"""Seeded random pods across the routing seams of kgpu_schedule_batch.

The hand-built parity files of the persistent kernels (test_percentage_persistent, test_percentage_topo_persistent,
test_norm_persistent, test_kbatch_early_publish) are exact but narrow in what a pod carries, and the two random
parity files run on 20 and 16 nodes at percentage 100: one workgroup, no cut, option 26 off.  Here
gen_random's rich pods (every node-affinity operator, matchFields, NoSchedule / NoExecute taints, host ports,
init containers, extended resources, spread constraints, pod (anti-)affinity with namespaces ...) run at the
smallest sizes at which every persistent kernel has two workgroups and a cut exists (gen_random.FAMILIES):

  generic_taints  200 nodes, pct 50 (to_find 100): PreferNoSchedule taints make nearly every pod a normalize-pass pod
  generic_plain   330 nodes, pct 31 (to_find 102): no such taint, so only a preferred node-affinity term makes one
  topo            400 nodes, pct 25 (to_find 100): spread constraints and pod (anti-)affinity

each also at percentage 100, under four option sets (OPTION_SETS), as the call sequence gen_random.family_calls
derives from the seed: four to six batches, a one-pod and a two-pod batch among them, and two kgpu_schedule_one
cycles, all on one nextStartNodeIndex rotation.

The reference is the C restatement (oracle/c) on the compiled queries, scheduled over the same spans; every GPU
case ends in test_percentage_persistent._equal: exact on node, feasible, evaluated, scored and score of every pod
and on all six node-row columns.  Two seeds of each family are also held to the Python oracle at the cut
percentage.  The CPU tests assert from the reference's records and the compiled queries alone that the seed
lists produce what the GPU cases are meant to exercise (enough cut pods, FitErrors, unscored shortcuts,
placements the cut changes, and every kind of pod).

Routing: every call's deltas of Engine.counters() and instantiation()["persistent_pods"] are held to what the
routing loop (kgpu_api.cpp) must do with the call's pods, so a silent fall-back to a per-pod pipeline fails a
case whose records still match.  The rules, as the loop has them:
  * norm[k] = needs_norm or Q_SCORE_ERROR sends a pod without topology state to the per-pod launches, unless
    option 26 > 0 and it is a needs_norm pod without Q_SCORE_ERROR: then it starts a k_nbatch run;
  * a k_nbatch run absorbs a following constant-maxima pod while another normalize-pass pod lies within the next
    (option 26) - 1 pods; at 26 = 1 it holds consecutive normalize-pass pods only;
  * a topology pod joins a k_tbatch run unless t_add refuses it (a DoNotSchedule constraint on a node-unique key,
    two ScheduleAnyway constraints): it then takes the per-pod topology pipeline in the middle of the batch;
  * kgpu_schedule_one is a diagnostic cycle: under a cut nothing of it runs persistently.
In generic_plain (no topology state, no PreferNoSchedule taint, no Q_SCORE_ERROR pod) needs_norm is
pref_terms.count > 0 and the counts are exact; in generic_taints they are exact with needs_norm restated on the
compiled inputs (_needs_norm).

What the topo family turned out to route (the first run had equal records and k_cbatch / k_nbatch counts of 0
where "some" was predicted): a pod is a topology pod for the loop when it has a plan (QPlan.topo), and it has
one not only for terms of its own (Q_HAS_TSC / Q_HAS_POD_AFFINITY / Q_HAS_POD_ANTI) but also when a Service or
ReplicaSet selects it (DefaultPodTopologySpread) or a term of an existing or assumed pod matches it.  In
topo_cluster's output that is nearly every pod (41 of 46 batch pods of seed 0 ran in k_tbatch, 26 have terms of
their own), and a pod without a plan reaches k_cbatch only if it also tolerates both PreferNoSchedule taints.
So the topo counts are bounds from _topo_kinds: at least the pods with terms k_tbatch carries run in it, at
least the pods that certainly have no plan run in k_cbatch / k_nbatch, at most the pods that may have none.
"Certainly" counts the terms the engine knows when the call is planned, those of the call's later pods included
(a second run showed that: build_plans interns a call's terms before it matches them).  Of seeds 0 to 499 only
393 has such a pod with constant maxima inside a batch (k_cbatch between k_tbatch runs), so it is in the list;
seeds 1 and 303 have one with a normalize pass (k_nbatch)."""
import functools

import numpy as np
import pytest

import gen_random
from kgpu import abi
from kgpu.compile import Profile
from kgpu.native import Engine

import test_percentage as TP
from test_percentage_persistent import FIELDS, ROW_KEYS, _Case, _cmp_oracle, _equal, _to_find
from test_percentage_topo_persistent import _TCase

TOPO_FLAGS = abi.Q_HAS_TSC | abi.Q_HAS_POD_AFFINITY | abi.Q_HAS_POD_ANTI
PODS = gen_random.FAMILY_PODS
# six seeds per family; test_seed_lists_produce_what_the_gpu_cases_need holds each list to its conditions
SEEDS = {"generic_taints": [0, 1, 5, 6, 7, 11], "generic_plain": [0, 2, 3, 7, 8, 13], "topo": [0, 1, 3, 5, 303, 393]}
ORACLE_SEEDS = 2  # the first two of each list are also held to the Python oracle
# a topo seed with a pod t_add refuses inside a batch (test_topo_refusal_seed_is_named_from_the_objects)
REFUSAL_SEED = 0
OPTION_SETS = {
    "default": [],
    "norm1": [(abi.OPT_NORM_PERSISTENT, 1)],
    "norm4": [(abi.OPT_NORM_PERSISTENT, 4)],
    "perpod": [(abi.OPT_CUT_PERSISTENT, 0), (abi.OPT_CUT_TOPO_PERSISTENT, 0), (abi.OPT_NORM_PERSISTENT, 0)],
}
COUNTERS = ("cut_persistent_pods", "cut_topo_persistent_pods", "norm_persistent_pods")


@functools.lru_cache(maxsize=None)
def _case(fam, seed, pct):
    """Compiled once and scheduled once by the C restatement over the seed's call spans; GPU cases leave it
    unchanged."""
    nodes, existing, pods, services, rss = gen_random.family(fam, seed)
    prof = Profile(percentage_of_nodes_to_score=pct)
    calls = gen_random.family_calls(seed)
    if fam == "topo":
        return _TCase(prof, nodes, existing, pods, calls=calls, services=services, rss=rss)
    return _Case(prof, nodes, existing, pods, calls=calls)


def _cut_pct(fam):
    return gen_random.FAMILIES[fam][1]


def _nrm(c):
    return c.q["pref_terms"]["count"] > 0


def _topo(c):
    return (c.q["flags"] & TOPO_FLAGS) != 0


def _needs_norm(c):
    """needs_norm (kgpu_api.cpp) restated on the compiled inputs under the default profile: a preferred
    node-affinity term, or a PreferNoSchedule taint of the cluster that the pod does not tolerate."""
    union = [int(np.bitwise_or.reduce(w)) for w in c.fw.arrays["taint_prefer"]]
    words = c.pc._keep["words"]
    out = _nrm(c).copy()
    for i, tol in enumerate(c.q["tol_prefer"]):
        b, n = int(tol["begin"]), int(tol["count"])
        out[i] |= any(u & ~(int(words[b + w]) if w < n else 0) for w, u in enumerate(union))
    return out


def _kind(c, i):
    return "topology" if _topo(c)[i] else "normalize-pass" if _nrm(c)[i] else "plain"


def _t_add_refuses(pod):
    """From the object: what k_tbatch does not carry (t_add, kgpu_api.cpp) -- a DoNotSchedule constraint on
    kubernetes.io/hostname (every node has its own value) or more than one ScheduleAnyway constraint."""
    tsc = pod["spec"].get("topologySpreadConstraints", [])
    return (any(t["whenUnsatisfiable"] == "DoNotSchedule" and t["topologyKey"] == gen_random.HOST for t in tsc) or
            sum(t["whenUnsatisfiable"] == "ScheduleAnyway" for t in tsc) > 1)


def _pod_terms(pod):
    for field in ("podAffinity", "podAntiAffinity"):
        sub = pod["spec"].get("affinity", {}).get(field, {})
        for t in sub.get("requiredDuringSchedulingIgnoredDuringExecution", []):
            yield pod["metadata"]["namespace"], t
        for w in sub.get("preferredDuringSchedulingIgnoredDuringExecution", []):
            yield pod["metadata"]["namespace"], w["podAffinityTerm"]


SEL_EMPTY = 2  # kSelEmpty (kgpu_internal.h): no Service / ReplicaSet selects the pod


def _topo_kinds_of(existing, pods, c):
    """(planned, loose, free) of the batch pods among `pods`, from the objects, the compiled queries c.q and the
    calls c.calls; `existing` are the pods the engine holds before the first call.
    planned: the pod has terms of its own that k_tbatch carries (a topology plan for certain, t_add accepts it).
    loose: no terms of its own and no Service / ReplicaSet selects it (an upper bound of the pods without a plan).
    free: loose, and no (anti-)affinity term the engine knows by then matches it -- those of the existing pods
    and of every pod of the calls so far, this call's later pods included (build_plans interns a call's terms
    before it matches them): certainly no topology plan, so it belongs to k_cbatch / k_nbatch / the per-pod
    launches."""
    from kgpu.compile import label_selector_matches
    topo = _topo(c)
    in_batch = np.zeros(len(pods), bool)
    free = np.zeros(len(pods), bool)
    seen = [t for p in existing for t in _pod_terms(p)]
    spans = [(call[1], call[2]) if call[0] == "batch" else (call[1], call[1] + 1) for call in c.calls]
    for (lo, hi), call in zip(spans, c.calls):
        seen += [t for p in pods[lo:hi] for t in _pod_terms(p)]
        if call[0] != "batch":
            continue
        in_batch[lo:hi] = True
        for i in range(lo, hi):
            md = pods[i]["metadata"]
            free[i] = not any(md["namespace"] in (t.get("namespaces") or [ns]) and
                              label_selector_matches(t["labelSelector"], md["labels"]) for ns, t in seen)
    loose = in_batch & ~topo & (c.q["dpts"]["kind"] == SEL_EMPTY)
    planned = in_batch & topo & ~np.array([_t_add_refuses(p) for p in pods])
    return planned, loose, free & loose


@functools.lru_cache(maxsize=None)
def _topo_kinds(seed):
    """_topo_kinds_of the topo family's seed."""
    _, existing, pods, _, _ = gen_random.family("topo", seed)
    return _topo_kinds_of(existing, pods, _case("topo", seed, _cut_pct("topo")))


def _topo_counts(planned, loose, free, need):
    """What _topo_bounds holds the counters to; dicts of several batches add up field by field."""
    return {"planned": int(planned.sum()), "loose": int(loose.sum()), "loose_plain": int((loose & ~need).sum()),
            "loose_need": int((loose & need).sum()), "free_plain": int((free & ~need).sum()),
            "free_need": int((free & need).sum())}


def _topo_bounds(want, opts, cut, tot, n, batch_pods, refusal):
    """The topology family's bounds on the counter totals `tot` of batches whose pods count as `n` (_topo_counts)."""
    n_c, n_n = n["free_plain"], n["free_need"]  # certain to reach k_cbatch / k_nbatch
    nb = opts in ("norm1", "norm4")
    if cut:
        want(tot["cut_topo_persistent_pods"] > 0, "no cut-mode k_tbatch run", tot)
        want(tot["cut_topo_persistent_pods"] >= n["planned"], "topology pods outside k_tbatch", tot, n["planned"])
        if opts == "norm4":  # a k_nbatch run may absorb a constant-maxima pod
            both = tot["cut_persistent_pods"] + tot["norm_persistent_pods"]
            want(n_c + n_n <= both <= n["loose"], "k_cbatch + k_nbatch pods", tot, n_c, n_n)
        else:
            want(n_c <= tot["cut_persistent_pods"] <= n["loose_plain"], "k_cbatch pods", tot, n_c)
    if nb:
        most = n["loose_need"] if opts == "norm1" else n["loose"]
        want(n_n <= tot["norm_persistent_pods"] <= most, "k_nbatch pods", tot, n_n)
        if refusal:
            want(tot["persistent_pods"] < batch_pods, "no pod left the batch for the per-pod pipeline", tot, batch_pods)


# ---------------------------------------------------------------- CPU
def test_family_sizes_and_calls():
    """Sizes: at least two workgroups of every kernel and a real cut; calls: the split the module
    docstring describes, stable per seed."""
    assert gen_random.FAMILIES == {"generic_taints": (200, 50, 100), "generic_plain": (330, 31, 102), "topo": (400, 25, 100)}
    for fam, (n, pct, k) in gen_random.FAMILIES.items():
        assert _to_find(n, pct) == k < n and n >= 100
        assert (n + 62) // 63 >= 2 and (fam != "topo" or (n + 255) // 256 == 2)
        assert len(SEEDS[fam]) == 6 and len(set(SEEDS[fam])) == 6
    for seed in sorted(set(sum(SEEDS.values(), []))):
        calls = gen_random.family_calls(seed)
        assert calls == gen_random.family_calls(seed)
        lens = [c[2] - c[1] for c in calls if c[0] == "batch"]
        assert 4 <= len(lens) <= 6 and 1 in lens and 2 in lens, calls
        ones = [i for i, c in enumerate(calls) if c[0] == "one"]
        assert len(ones) == 2 and all(0 < i < len(calls) - 1 for i in ones), calls
        spans = [(c[1], c[2]) if c[0] == "batch" else (c[1], c[1] + 1) for c in calls]
        assert spans[0][0] == 0 and spans[-1][1] == PODS and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert len({tuple(gen_random.family_calls(s)) for s in range(6)}) == 6


CLUSTER0_DIGEST = "d677403d595a5ff6"  # sha256 of the sorted JSON of cluster(0) / topo_cluster(0), first 16 digits
TOPO0_DIGEST = "843a554f736ef49c"


def test_existing_generators_unchanged():
    """cluster() and topo_cluster() draw as before: the digests of the existing random-parity inputs."""
    import hashlib
    import json

    def digest(x):
        return hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()[:16]

    assert digest(gen_random.cluster(0)) == CLUSTER0_DIGEST
    assert digest(gen_random.topo_cluster(0)) == TOPO0_DIGEST
    # generic_plain: the same objects as cluster() but for the PreferNoSchedule taints
    nodes, ex, pods, _, _ = gen_random.family("generic_plain", 1)
    n0, ex0, pods0 = gen_random.cluster(1, 330, 165, PODS)
    assert (ex, pods) == (ex0, pods0)
    for a, b in zip(nodes, n0):
        assert all(t["effect"] != "PreferNoSchedule" for t in a["spec"].get("taints", []))
        assert a["spec"].get("taints", []) == [t for t in b["spec"].get("taints", []) if t["effect"] != "PreferNoSchedule"]
        assert a["metadata"] == b["metadata"] and a["status"] == b["status"]


@pytest.mark.parametrize("fam", sorted(SEEDS))
def test_seed_lists_produce_what_the_gpu_cases_need(fam):
    """Over the family's whole seed list at the cut percentage, from the C restatement's records and the
    compiled queries alone."""
    n, pct, k = gen_random.FAMILIES[fam]
    cut = fit = one = moved = nrm_pods = total = 0
    nrm_then_plain = nrm_then_nrm = notopo_nrm = 0
    for seed in SEEDS[fam]:
        c, c100 = _case(fam, seed, pct), _case(fam, seed, 100)
        w = c.want
        assert len(w) == PODS and c.n == n and (w["node"] >= -1).all()
        assert (c100.want["evaluated"] == n).all()
        total += PODS
        cut += int((w["evaluated"] < n).sum())
        fit += int((w["node"] == -1).sum())
        one += int((w["feasible"] == 1).sum())
        moved += int((w["node"] != c100.want["node"]).sum())
        assert (w["feasible"] <= k).all() and (w["scored"][w["feasible"] == 1] == 0).all()
        nrm, topo = _nrm(c), _topo(c)
        if fam == "generic_plain":
            # what makes its routing exact: no topology state, no PreferNoSchedule taint, no Q_SCORE_ERROR
            assert not topo.any() and not (c.q["flags"] & abi.Q_SCORE_ERROR).any()
            assert not c.fw.arrays["taint_prefer"].any() and (_needs_norm(c) == nrm).all()
            nrm_pods += int(nrm.sum())
            nrm_then_plain += int((nrm[:-1] & ~nrm[1:]).sum())
            nrm_then_nrm += int((nrm[:-1] & nrm[1:]).sum())
        if fam == "topo":
            assert int(topo.sum()) >= 25 and int((~topo).sum()) >= 5, (seed, int(topo.sum()))
            notopo_nrm += int((~topo & nrm).sum())
    assert 4 * cut >= total, (cut, total)
    assert 1 <= fit and 100 * fit <= 35 * total, (fit, total)
    assert one >= 3, one
    assert 10 * moved >= total, (moved, total)
    if fam == "generic_plain":
        assert 20 * total <= 100 * nrm_pods <= 60 * total, (nrm_pods, total)
        assert nrm_then_plain >= 1 and nrm_then_nrm >= 1
    if fam == "topo":
        assert notopo_nrm >= 3, notopo_nrm


def test_topo_refusal_seed_is_named_from_the_objects():
    """REFUSAL_SEED has a pod inside a batch of three or more that t_add refuses, between two topology pods
    it accepts: the per-pod topology pipeline runs in the middle of a batch."""
    _, _, pods, _, _ = gen_random.family("topo", REFUSAL_SEED)
    c = _case("topo", REFUSAL_SEED, _cut_pct("topo"))
    refused = np.array([_t_add_refuses(p) for p in pods])
    assert (_topo(c)[refused]).all()
    inside = [k for call in c.calls if call[0] == "batch" and call[2] - call[1] >= 3
              for k in range(call[1] + 1, call[2] - 1) if refused[k] and not refused[k - 1] and _topo(c)[k - 1]]
    assert inside, refused.nonzero()


def test_topo_family_reaches_every_kind_of_run():
    """In topo_cluster's output a Service or a ReplicaSet selects two thirds of the pods and the (anti-)affinity
    terms of existing and earlier pods match most of the others, so nearly every pod has a topology plan
    whether or not it has terms of its own.  From the objects alone: every seed has pods k_tbatch carries, and
    the list holds seeds with a pod inside a batch that certainly has no plan -- one with constant maxima
    (k_cbatch under a cut) and one with a normalize pass (k_nbatch under option 26)."""
    n_c = n_n = 0
    for seed in SEEDS["topo"]:
        c = _case("topo", seed, _cut_pct("topo"))
        planned, loose, free = _topo_kinds(seed)
        need = _needs_norm(c)
        assert planned.sum() >= 15 and (free <= loose).all() and not (planned & loose).any()
        n_c += int((free & ~need).sum())
        n_n += int((free & need).sum())
    assert n_c >= 1 and n_n >= 2, (n_c, n_n)


@pytest.mark.parametrize("fam,seed", [(f, s) for f in sorted(SEEDS) for s in SEEDS[f][:ORACLE_SEEDS]])
def test_c_restatement_matches_python_oracle_under_the_cut(fam, seed):
    """Node, feasible count, evaluated count and the winner's score against oracle.refsched at the cut
    percentage: neither existing random file does this above 20 nodes or below percentage 100."""
    nodes, existing, pods, services, rss = gen_random.family(fam, seed)
    pct = _cut_pct(fam)
    _cmp_oracle(_case(fam, seed, pct), TP.oracle_run(nodes, existing, pods, services, rss, pct))


# ---------------------------------------------------------------- GPU
def _run(case, options):
    """The case's calls on a fresh engine: (records, node rows, per-call deltas, counters).  A call's delta
    holds the three pod counters' increase and instantiation()["persistent_pods"]."""
    e = Engine(case.fw.config)
    try:
        e.upload(case.fw.snap, case.fw.arrays)
        for opt, v in options:
            e.set_option(opt, v)
        got, deltas, before = [], [], dict.fromkeys(COUNTERS, 0)
        for call in case.calls:
            if call[0] == "batch":
                got.append(e.schedule_batch(case.q[call[1]:call[2]], case.pc, first_seq=call[1])[0])
            else:
                res, _ = e.schedule_one(case.q[call[1]], case.pc, seq=call[1], assume=True)
                one = np.zeros(1, abi.RESULT)
                for f in FIELDS:
                    one[0][f] = res[f]
                got.append(one)
            cnt = e.counters()
            d = {k: cnt[k] - before[k] for k in COUNTERS}
            before = {k: cnt[k] for k in COUNTERS}
            d["persistent_pods"] = e.instantiation()["persistent_pods"]
            deltas.append(d)
        return np.concatenate(got), e.read_nodes(case.n), deltas, e.counters()
    finally:
        e.close()


def _describe(case, got, rows, what):
    """What is needed to read a mismatch without another run: the first differing pod, its kind, the call it
    lies in, and the rotation start of that pod and of its predecessor."""
    bad = [int(np.nonzero(case.want[f] != got[f])[0][0]) for f in FIELDS if (case.want[f] != got[f]).any()]
    if not bad:
        cols = [k for k in ROW_KEYS if not np.array_equal(case.rows[k], rows[k])]
        return "%s: every record equal, node rows differ in %s" % (what, cols)
    i = min(bad)
    call = next(c for c in case.calls if (c[1] <= i < c[2] if c[0] == "batch" else c[1] == i))
    rec = lambda r: {f: int(r[f][i]) for f in FIELDS}  # noqa: E731
    prev = "none" if i == 0 else "%s pod %d, start %d" % (_kind(case, i - 1), i - 1, int(case.start[i - 1]))
    return ("%s: first differing pod %d (%s, ports %d) in call %s, start %d (predecessor: %s)\n  want %s\n  got  %s" %
            (what, i, _kind(case, i), int(case.q["ports"]["count"][i]), call, int(case.start[i]), prev, rec(case.want),
             rec(got)))


def _check_records(case, got, rows, what):
    try:
        _equal(case.want, got, case.rows, rows)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (_describe(case, got, rows, what), e)) from None


def _routing(fam, seed, pct, opts, case, deltas, topo_sum=None):
    """The routing assertions, as a list of failures (reported after the records, which say more).
    topo_sum: a dict of a caller that holds the topology family's bounds over several _routing calls itself
    (_topo_bounds; test_delta_routing, one call per checkpoint): the counter totals are added to it instead."""
    bad = []

    def want(cond, *msg):
        if not cond:
            bad.append(msg)

    cut = pct < 100
    nrm, topo, need = _nrm(case), _topo(case), _needs_norm(case)
    tot = dict.fromkeys(COUNTERS + ("persistent_pods",), 0)
    batch_pods = 0
    in_batch = np.zeros(len(case.q), bool)
    for call, d in zip(case.calls, deltas):
        if call[0] == "one":
            if cut:
                want(d["persistent_pods"] == 0 and not any(d[k] for k in COUNTERS), call, d)
            continue
        lo, hi = call[1], call[2]
        batch_pods += hi - lo
        in_batch[lo:hi] = True
        for k in tot:
            tot[k] += d[k]
        counted = sum(d[k] for k in COUNTERS)
        if cut:
            want(counted == d["persistent_pods"], "cut + cut_topo + norm != persistent_pods", call, d)
        else:
            want(d["cut_persistent_pods"] == 0 and d["cut_topo_persistent_pods"] == 0, "cut counters at 100", call, d)
        if opts == "perpod":
            want(counted == 0 and d["persistent_pods"] == 0, "perpod ran persistently", call, d)
        if opts in ("default", "perpod"):
            want(d["norm_persistent_pods"] == 0, "k_nbatch with option 26 = 0", call, d)
        n_nrm = int(nrm[lo:hi].sum())
        if fam == "generic_plain":
            if opts in ("norm1", "norm4"):
                want(d["persistent_pods"] == hi - lo, "not every pod persistent", call, d)
            if opts == "norm1":
                want(d["norm_persistent_pods"] == n_nrm, "norm1: k_nbatch pods != normalize-pass pods", n_nrm, call, d)
            if opts == "norm4":
                want(d["norm_persistent_pods"] >= n_nrm, "norm4: fewer k_nbatch pods than at norm1", n_nrm, call, d)
            if opts == "default":
                want(d["persistent_pods"] == hi - lo - n_nrm, "default: persistent pods != plain pods", n_nrm, call, d)
        if fam == "generic_taints":
            # no topology state and no Q_SCORE_ERROR pod either: exact with needs_norm restated (_needs_norm)
            n_need = int(need[lo:hi].sum())
            if opts == "norm1":
                want(d["norm_persistent_pods"] >= n_nrm, "norm1: fewer k_nbatch pods than preferred-term pods", n_nrm, call, d)
                want(d["norm_persistent_pods"] == n_need, "norm1: k_nbatch pods != needs_norm pods", n_need, call, d)
            if opts in ("norm1", "norm4"):
                want(d["persistent_pods"] == hi - lo, "not every pod persistent", call, d)
            if opts == "default":
                want(d["persistent_pods"] == hi - lo - n_need, "default: persistent pods != constant-maxima pods", n_need, call, d)
    if fam == "topo" and opts != "perpod":
        if topo_sum is not None:
            for k in tot:
                topo_sum[k] = topo_sum.get(k, 0) + tot[k]
            topo_sum["batch_pods"] = topo_sum.get("batch_pods", 0) + batch_pods
        else:
            _topo_bounds(want, opts, cut, tot, _topo_counts(*_topo_kinds(seed), need), batch_pods, seed == REFUSAL_SEED)
    print("routing %s seed %d pct %d %s: %s of %d batch pods" % (fam, seed, pct, opts, tot, batch_pods))
    return bad


def _matrix():
    for fam in sorted(SEEDS):
        for seed in SEEDS[fam]:
            for pct in (_cut_pct(fam), 100):
                for opts in OPTION_SETS:
                    if opts == "perpod" and pct == 100:
                        continue  # the parity twin of the cut-mode kernels
                    yield pytest.param(fam, seed, pct, opts, id="%s-s%d-p%d-%s" % (fam, seed, pct, opts))


@pytest.mark.gpu
@pytest.mark.parametrize("fam,seed,pct,opts", list(_matrix()))
def test_gpu_random_routing(fam, seed, pct, opts):
    case = _case(fam, seed, pct)
    got, rows, deltas, counters = _run(case, OPTION_SETS[opts])
    what = "%s seed %d pct %d options %s %s" % (fam, seed, pct, opts, OPTION_SETS[opts])
    bad = _routing(fam, seed, pct, opts, case, deltas)
    _check_records(case, got, rows, what)
    assert not bad, "%s: records equal, routing differs: %s" % (what, bad)
    _equal(case.want, got, case.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(SEEDS))
def test_gpu_random_routing_cooperative(fam):
    """Percentage 100, option 26 = 1, every persistent launch through hipLaunchCooperativeKernel: nothing is
    issued again."""
    seed = SEEDS[fam][0]
    case = _case(fam, seed, 100)
    got, rows, deltas, counters = _run(case, OPTION_SETS["norm1"] + [(abi.OPT_COOPERATIVE, 1)])
    assert counters["coop_retries"] == 0 and counters["coop_launches"] >= 1, counters
    what = "%s seed %d pct 100 options norm1 + cooperative" % (fam, seed)
    bad = _routing(fam, seed, 100, "norm1", case, deltas)
    _check_records(case, got, rows, what)
    assert not bad, "%s: records equal, routing differs: %s" % (what, bad)
    _equal(case.want, got, case.rows, rows)
