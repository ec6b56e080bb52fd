"""kgpu_schedule_one cycles of topology pods under percentageOfNodesToScore below 100 inside ONE launch: a
one-pod run of k_tbatch's cut-mode instantiation (KGPU_OPT_CUT_TOPO_ONE, option 28, off by default; DESIGN.md
4.3.4) instead of the per-pod topology pipeline.

A diagnostic cycle must leave what kgpu_get_filter and kgpu_get_scores promise (include/kgpu.h) and oracle/c
restates (kgpu_ref_schedule's status_out / raw_out / norm_out).  With s the rotation before the pod, p the cut
position and pos = n >= s ? n - s : n + N - s:
  * a kept node (one of the first to_find feasible rows in rotated order) has word 0 and its raw / normalized
    rows;
  * a node that was not kept and lies at pos >= p -- the feasible rows beyond the cut and the failing rows
    nobody examined -- has KGPU_FS_NOT_EVALUATED and zero rows;
  * a node that failed a filter at pos < p has its own failing word and zero rows;
  * the one-feasible-node shortcut leaves every score row 0; a profile without filter plugins keeps n < to_find
    in non-rotated order.

Everything is exact.  The reference of cycle i is a fresh RefEngine that schedules q[:i + 1] with diag=True: its
last record, status words and score rows are that cycle's.  The GPU side is one engine with the option at 1 and
schedule_one(q[i], seq=i, assume=True) in order; after every cycle the record, all N status words and the whole
raw / normalized row of every score plugin of the profile are compared, and at the end the six node-row
columns.  Every case asserts what ran (the ninth counter of kgpu_debug_counters, the batch counter staying 0,
kgpu_debug_geometry), so a silent fall-back to the per-pod pipeline fails it.  The inputs are
test_percentage_topo_persistent.py's generators, which that file's CPU tests pin."""
import inspect
import os
import re

import numpy as np
import pytest

from kgpu import abi, native
from kgpu.compile import Profile
from kgpu.native import Engine

from test_percentage_persistent import FIELDS, ROW_KEYS, _equal, _to_find
from test_percentage_topo_persistent import (GEO_CASES, PROFILE_ROWS, RACKS, SEAM_PODS, TGEO, _TCase, _edge_case,
                                             _ipa, _nofilter_case, _rack, _rack_nodes, _rack_pod, _service_case,
                                             _split_pods, EDGE_PODS)
from kgpu import cluster

NOT_EVALUATED = abi.STATUS_NOT_EVALUATED
RACK_CYCLES, BIG_CYCLES = 24, 8

_REFS = {}


def _ref(c, i):
    """Cycle i of case c on the C restatement: (record, words, raw[12][N], norm[12][N], node rows after it)."""
    key = (id(c), i)
    if key not in _REFS:
        from oracle.cref import RefEngine
        ref = RefEngine(c.fw.config, c.fw.snap)
        try:
            res, st, raw, norm = ref.schedule(c.q[:i + 1], c.pc, diag=True)
            _REFS[key] = (res[-1].copy(), st, raw, norm, ref.read_nodes())
        finally:
            ref.close()
    return _REFS[key]


def _plugins(c):
    cfg = c.fw.config
    return [int(cfg.scores[k]) for k in range(cfg.n_scores)]


def _starts(c, n_cycles):
    """nextStartNodeIndex before every cycle, from the reference's evaluated counts."""
    p = np.array([int(_ref(c, i)[0]["evaluated"]) for i in range(n_cycles)], np.int64)
    return np.concatenate([[0], np.cumsum(p) % c.n])[:-1], p


# ---------------------------------------------------------------- CPU
def test_option_and_counter_are_mirrored():
    assert abi.OPT_CUT_TOPO_ONE == 28
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "kgpu.h")).read()
    assert re.search(r"#define KGPU_OPT_CUT_TOPO_ONE 28\b", hdr)
    assert "out[8]" in hdr
    src = inspect.getsource(native.Engine.counters)
    names = re.findall(r'"(\w+)"', src)
    assert len(names) == 9 and names[8] == "cut_topo_one_cycles" and names[6] == "cut_topo_persistent_pods", names


def test_rack_reference_words_hold_all_three_kinds():
    """The rack cluster at 600 nodes and percentage 30 (to_find 180): every third node has 1 CPU and fails
    NodeResourcesFit for the 2-CPU pods, about 400 nodes are feasible.  Every cycle's reference words hold a
    kept node, a failing word below the cut, and NOT_EVALUATED on both a feasible node (the one at the cut
    position, whose discovery cancelled the search) and a failing node (a 1-CPU node beyond it); the score rows
    are zero wherever the word is not 0."""
    c, _ = _rack(30)
    N, K = c.n, _to_find(600, 30)
    assert (N, K) == (600, 180)
    s_of, p_of = _starts(c, RACK_CYCLES)
    small = np.arange(N) % 3 == 0  # 1 CPU: fails Fit for every rack pod
    for i in range(RACK_CYCLES):
        rec, st, raw, norm, _ = _ref(c, i)
        s, p = int(s_of[i]), int(p_of[i])
        assert p < N and rec["feasible"] == K and rec["scored"] == 1, i
        pos = (np.arange(N) - s) % N
        kept = st == 0
        assert kept.sum() == K and (pos[kept] < p).all(), i
        failing = (st != 0) & (st != NOT_EVALUATED)
        assert failing.any() and (pos[failing] < p).all() and small[failing].sum() >= 1, i
        ne = st == NOT_EVALUATED
        assert (pos[ne] >= p).all() and ne.sum() == N - p, i
        assert ne[(s + p) % N] and not small[(s + p) % N], i        # the feasible node that cancelled the search
        assert (ne & small).any() and (ne & ~small).sum() >= 2, i    # failing and feasible nodes beyond it
        for plugin in _plugins(c):
            assert not raw[plugin][~kept].any() and not norm[plugin][~kept].any(), (i, plugin)
        assert any(raw[plugin][kept].any() for plugin in _plugins(c)), i


def test_rack_cycles_wrap_and_split_workgroups():
    """At least one cycle's window wraps past node N - 1, and at least one has s and the cut node in different
    workgroups, for every geometry case (from the reference's evaluated counts, as _split_pods)."""
    c, _ = _rack(30)
    s_of, p_of = _starts(c, RACK_CYCLES)
    assert ((s_of + p_of) > c.n).any()
    for geo, (n, pct) in GEO_CASES.items():
        cg, _ = _rack(pct, n_nodes=n)
        cycles = RACK_CYCLES if n == 600 else BIG_CYCLES
        s, p = _starts(cg, cycles)
        per = TGEO[geo][0] * TGEO[geo][1]
        cut = (s + p - 1) % cg.n
        assert ((p < cg.n) & (s // per != cut // per)).any(), geo
        assert (cg.start[:cycles] == s).all() and len(_split_pods(cg, per)) >= 1


def test_edge_reference_covers_the_boundaries():
    """_edge_case's nine pods in order, on the per-cycle reference: the shortcut pod has no NOT_EVALUATED word
    and zero rows, the FitError pod only failing words, and the no-filter profile keeps n < to_find."""
    e = _edge_case()
    idx = {name: i for i, (name, _) in enumerate(EDGE_PODS)}
    rec, st, raw, norm, _ = _ref(e, idx["one"])
    assert (rec["feasible"], rec["scored"], rec["evaluated"]) == (1, 0, e.n) and (st == 0).sum() == 1
    assert not (st == NOT_EVALUATED).any() and not raw.any() and not norm.any()
    rec, st, raw, norm, _ = _ref(e, idx["none"])
    assert rec["node"] < 0 and rec["evaluated"] == e.n and ((st != 0) & (st != NOT_EVALUATED)).all()
    rec, st, _, _, _ = _ref(e, idx["first_of_next"])
    assert st[256] == NOT_EVALUATED and (st[:200] == 0).all() and rec["evaluated"] == 256
    nf = _nofilter_case()
    K = _to_find(nf.n, 60)
    for i in (0, len(nf.q) - 1):
        rec, st, _, _, _ = _ref(nf, i)
        assert (st[:K] == 0).all() and (st[K:] == NOT_EVALUATED).all() and rec["evaluated"] == K


# ---------------------------------------------------------------- GPU
def _check_cycle(e, c, i, res, full=True):
    """Cycle i of the engine against the reference: the record, every word, every row of the profile."""
    rec, st, raw, norm, _ = _ref(c, i)
    for f in FIELDS:
        assert res[f] == rec[f], "cycle %d: %s %s vs oracle/c %s" % (i, f, res[f], rec[f])
    words = e.filter_words(c.n)
    np.testing.assert_array_equal(words, st, err_msg="cycle %d: status words" % i)
    for plugin in _plugins(c):
        r, nm = e.scores(plugin, c.n)
        if full:
            np.testing.assert_array_equal(r, raw[plugin], err_msg="cycle %d: raw scores of plugin %d" % (i, plugin))
            np.testing.assert_array_equal(nm, norm[plugin], err_msg="cycle %d: normalized scores of plugin %d" % (i, plugin))
        else:  # a cycle on the per-pod pipeline: held on the kept nodes
            k = st == 0
            np.testing.assert_array_equal(r[k], raw[plugin][k], err_msg="cycle %d: raw scores of plugin %d" % (i, plugin))
            np.testing.assert_array_equal(nm[k], norm[plugin][k], err_msg="cycle %d: normalized scores of plugin %d" % (i, plugin))


def _run_cycles(c, n_cycles, options=(), index=1, row=None, must=None):
    """n_cycles kgpu_schedule_one cycles with the option at 1, each compared; every cycle (or those `must`
    selects) has to be a one-pod k_tbatch run of geometry `index`; the rest count on whichever path they took."""
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
        e.set_option(abi.OPT_CUT_TOPO_ONE, 1)
        for opt, v in options:
            e.set_option(opt, v)
        ran = 0
        for i in range(n_cycles):
            res, _ = e.schedule_one(c.q[i], c.pc, seq=i, assume=True)
            g = e.geometry()
            inside = g["kernel"] == "k_tbatch"
            if must is None or must(i):
                assert inside and g["index"] == index, (i, g)
            if inside:
                inst = e.instantiation()
                assert inst["persistent_pods"] == 1 and (row is None or inst["row"] == row), (i, inst)
            ran += inside
            _check_cycle(e, c, i, res, full=inside)
        cnt = e.counters()
        assert cnt["cut_topo_one_cycles"] == ran and cnt["persistent_launches"] == ran, cnt
        assert cnt["cut_topo_persistent_pods"] == 0 and cnt["cut_persistent_pods"] == 0 and cnt["coop_retries"] == 0, cnt
        if must is None:
            assert ran == n_cycles
        rows = e.read_nodes(c.n)
        want_rows = _ref(c, n_cycles - 1)[4]
        for k in ROW_KEYS:
            np.testing.assert_array_equal(want_rows[k], rows[k], err_msg=k)
        return cnt
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geo", sorted(GEO_CASES))
def test_gpu_cut_one_geometry(geo):
    """256 x 1 and 512 x 1 (status word and rows held in registers until the pod resolves), 512 x 2 (resident
    rows, direct stores) and 512 x 4 / 512 x 8 (streamed rows)."""
    n, pct = GEO_CASES[geo]
    c, _ = _rack(pct, n_nodes=n)
    _run_cycles(c, RACK_CYCLES if n == 600 else BIG_CYCLES, [(abi.OPT_TBATCH_GEO, geo)], index=geo, row=2)


@pytest.mark.gpu
@pytest.mark.parametrize("prof", ["least21", "most", "autoscaler"])
def test_gpu_cut_one_profile_rows(prof):
    """The runtime rows store directly even at one row per lane."""
    c, _ = _rack(30, prof=prof)
    _run_cycles(c, RACK_CYCLES, row=PROFILE_ROWS[prof])


@pytest.mark.gpu
def test_gpu_cut_one_edge_pods():
    c = _edge_case()
    _run_cycles(c, len(c.q), [(abi.OPT_TBATCH_GEO, 0)], index=0)


@pytest.mark.gpu
def test_gpu_cut_one_no_filter_profile():
    c = _nofilter_case()
    _run_cycles(c, len(c.q), [(abi.OPT_TBATCH_GEO, 0)], index=0)


@pytest.mark.gpu
def test_gpu_cut_one_service_zone_sums():
    c = _service_case()
    _run_cycles(c, len(c.q))


@pytest.mark.gpu
def test_gpu_cut_one_pod_affinity():
    """cluster.pod_affinity: the pods with (anti-)affinity terms of their own are topology pods; every 16th pod
    has none and may take the per-pod pipeline, where it is held on the kept nodes."""
    c = _ipa(30)
    cnt = _run_cycles(c, len(c.q), must=lambda i: i % 16 != 0)
    assert cnt["cut_topo_one_cycles"] >= sum(1 for i in range(len(c.q)) if i % 16 != 0)


@pytest.mark.gpu
def test_gpu_cut_one_first_max_tie_mode():
    c, _ = _rack(30, tie=1)
    _run_cycles(c, RACK_CYCLES)


_SEAM = []


def _seam3_case():
    """_seam_case's pod mix with three cycles between the batches: a rack pod (the one-pod cut-mode run), a plain
    pod and a preferred-affinity pod (both on the per-pod pipeline)."""
    if not _SEAM:
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
        a = SEAM_PODS // 2
        assert a % 3 == 0
        calls = [("batch", 0, a), ("one", a), ("one", a + 1), ("one", a + 2), ("batch", a + 3, SEAM_PODS)]
        _SEAM.append(_TCase(Profile(percentage_of_nodes_to_score=30), _rack_nodes(600), [], pods, calls=calls))
    return _SEAM[0]


@pytest.mark.gpu
def test_gpu_cut_one_seams():
    """A cut-mode batch, three kgpu_schedule_one cycles, a batch, on one rotation; each counter counts its own."""
    c = _seam3_case()
    assert (c.want["node"] >= 0).all() and (c.want["evaluated"] < c.n).all()
    got, rows, insts, geos, counters = c.run_gpu([(abi.OPT_CUT_TOPO_ONE, 1)])
    a = SEAM_PODS // 2
    kinds = np.arange(SEAM_PODS) % 3
    in_batch = np.ones(SEAM_PODS, bool)
    in_batch[a:a + 3] = False
    t, p = int(((kinds == 0) & in_batch).sum()), int(((kinds == 1) & in_batch).sum())
    assert [i["persistent_pods"] for i in insts[1:4]] == [1, 0, 0], insts
    assert geos[1]["kernel"] == "k_tbatch" and geos[2]["kernel"] is None and geos[3]["kernel"] is None, geos
    assert counters["cut_topo_one_cycles"] == 1, counters
    assert counters["cut_topo_persistent_pods"] == t and counters["cut_persistent_pods"] == p, counters
    _equal(c.want, got, c.rows, rows)


@pytest.mark.gpu
def test_gpu_cut_one_without_assume():
    """assume=False: the cycle leaves every node row unchanged and still advances nextStartNodeIndex, as the
    reference does whether or not the pod is assumed; the next cycle's window starts where the reference's does."""
    from oracle.cref import RefEngine
    c, _ = _rack(30)
    rec0, st0, raw0, norm0, _ = _ref(c, 0)
    ref = RefEngine(c.fw.config, c.fw.snap)
    try:
        ref.next_start = int(rec0["evaluated"]) % c.n   # the same cluster, the rotation one cycle on
        res1, st1, raw1, norm1 = ref.schedule(c.q[1:2], c.pc, first_seq=1, diag=True)
        rows1 = ref.read_nodes()
    finally:
        ref.close()
    assert res1[0]["evaluated"] < c.n and st1[int(rec0["evaluated"]) % c.n] == 0
    e = Engine(c.fw.config)
    try:
        e.upload(c.fw.snap, c.fw.arrays)
        e.set_option(abi.OPT_CUT_TOPO_ONE, 1)
        before = e.read_nodes(c.n)
        res, slot = e.schedule_one(c.q[0], c.pc, seq=0, assume=False)
        _check_cycle(e, c, 0, res)
        after = e.read_nodes(c.n)
        for k in ROW_KEYS:
            np.testing.assert_array_equal(before[k], after[k], err_msg=k)
        res, _ = e.schedule_one(c.q[1], c.pc, seq=1, assume=True)
        for f in FIELDS:
            assert res[f] == res1[0][f], (f, res[f], res1[0][f])
        np.testing.assert_array_equal(e.filter_words(c.n), st1)
        for plugin in _plugins(c):
            r, nm = e.scores(plugin, c.n)
            np.testing.assert_array_equal(r, raw1[plugin], err_msg="raw %d" % plugin)
            np.testing.assert_array_equal(nm, norm1[plugin], err_msg="norm %d" % plugin)
        rows = e.read_nodes(c.n)
        for k in ROW_KEYS:
            np.testing.assert_array_equal(rows1[k], rows[k], err_msg=k)
        cnt = e.counters()
        assert cnt["cut_topo_one_cycles"] == 2 and cnt["cut_topo_persistent_pods"] == 0, cnt
        assert e.geometry()["kernel"] == "k_tbatch"
    finally:
        e.close()


@pytest.mark.gpu
def test_gpu_cut_one_twin():
    """Two engines, option 0 (the per-pod topology pipeline) and 1, the same 24 rack cycles: records and words
    identical, score rows identical on the nodes whose word is 0, final rows identical; only the option-1 engine
    starts runs from the resident topology state."""
    c, _ = _rack(30)

    def run(v):
        e = Engine(c.fw.config)
        try:
            e.upload(c.fw.snap, c.fw.arrays)
            e.set_option(abi.OPT_CUT_TOPO_ONE, v)
            out = []
            for i in range(RACK_CYCLES):
                res, _ = e.schedule_one(c.q[i], c.pc, seq=i, assume=True)
                out.append((tuple(int(res[f]) for f in FIELDS), e.filter_words(c.n),
                            [e.scores(s, c.n) for s in _plugins(c)], e.geometry()["kernel"]))
            return out, e.read_nodes(c.n), e.topo_resident(), e.counters()
        finally:
            e.close()

    out1, rows1, res1, cnt1 = run(1)
    out0, rows0, res0, cnt0 = run(0)
    assert cnt1["cut_topo_one_cycles"] == RACK_CYCLES and cnt0["cut_topo_one_cycles"] == 0, (cnt1, cnt0)
    assert cnt0["persistent_launches"] == 0 and all(o[3] is None for o in out0) and all(o[3] == "k_tbatch" for o in out1)
    stray = 0
    for i in range(RACK_CYCLES):
        assert out1[i][0] == out0[i][0], i
        np.testing.assert_array_equal(out1[i][1], out0[i][1], err_msg="cycle %d: words" % i)
        k = out1[i][1] == 0
        for (r1, n1), (r0, n0) in zip(out1[i][2], out0[i][2]):
            np.testing.assert_array_equal(r1[k], r0[k], err_msg="cycle %d: raw" % i)
            np.testing.assert_array_equal(n1[k], n0[k], err_msg="cycle %d: normalized" % i)
            assert not r1[~k].any() and not n1[~k].any(), i
            stray += int(r0[~k].any() or n0[~k].any())
    print("per-pod pipeline: score rows with non-zero values on nodes whose word is non-zero: %d" % stray)
    for k in ROW_KEYS:
        np.testing.assert_array_equal(rows1[k], rows0[k], err_msg=k)
    assert res1[0] >= 1 and res0[0] == 0, (res1, res0)
