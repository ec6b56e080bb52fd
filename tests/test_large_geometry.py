"""The streamed persistent geometries: k_tbatch at 512 threads x 4 and x 8 rows per lane
(KGPU_OPT_TBATCH_GEO 3 and 4) and k_batch at 512 x 8 (KGPU_OPT_BATCH_GEO 6), which hold clusters of up
to one million nodes on one GPU.  The geometry choice is pure host code (kgpu_geometry_for); the GPU
runs use the smallest clusters at which a row above the old rows per lane holds a node -- a capped grid
(KGPU_OPT_PERSIST_GROUPS) gives each lane more rows -- and compare placements, feasible counts, scores
and every node row with the C restatement (oracle/c).  Each GPU test also asks the engine which kernel
and rows per lane its last persistent launch used (kgpu_debug_geometry): without the new geometries a
forced index clamps to 512 x 2 and a capped grid falls back to one launch per pod.

Seeds: chosen by running the C restatement on the CPU (no GPU involved) so that at least one pod of the
batch lands in the upper half of the rows (see _upper_rows_hit)."""
import numpy as np
import pytest

import gen_random
from kgpu import abi, cluster
from kgpu.compile import Cluster, Profile
from kgpu.framework import GpuFramework
from kgpu.native import KERNEL_BATCH, KERNEL_TBATCH, KgpuError, geometry_for

# ---- the geometry tables and the first-fit rule, restated
# (threads per workgroup, rows per lane); k_batch keeps the last slot of the last lane as a spare
OLD_TGEO = [(256, 1), (512, 1), (512, 2)]
OLD_GEO = [(64, 1), (128, 1), (192, 1), (448, 1), (960, 1), (512, 4)]
NEW_TGEO = OLD_TGEO + [(512, 4), (512, 8)]
NEW_GEO = OLD_GEO + [(512, 8)]


def _first_fit(table, spare, n, max_groups, first):
    for gi in range(first, len(table)):
        per = table[gi][0] * table[gi][1] - spare
        g = (n + per - 1) // per
        if g <= max_groups:
            return gi, max(g, 1), per
    return None


@pytest.mark.parametrize("kernel", [KERNEL_BATCH, KERNEL_TBATCH])
def test_old_geometry_choices_unchanged(kernel):
    old, new, spare, default = ((OLD_GEO, NEW_GEO, 1, 0) if kernel == KERNEL_BATCH else (OLD_TGEO, NEW_TGEO, 0, 1))
    sizes = [1, 63, 64, 5000, 65536, 125000, 262144] + ([262145, 524032] if kernel == KERNEL_BATCH else [])
    grown = 0
    for first in sorted({0, default}):
        for max_groups in (1, 2, 3, 80, 256):
            for n in sizes:
                was = _first_fit(old, spare, n, max_groups, first)
                now = _first_fit(new, spare, n, max_groups, first)
                if was is not None:
                    assert now == was
                if now is None:
                    with pytest.raises(KgpuError) as ex:
                        geometry_for(kernel, n, max_groups, first)
                    assert ex.value.code == abi.E_CAPACITY
                    continue
                grown += was is None
                got = geometry_for(kernel, n, max_groups, first)
                assert (got["index"], got["groups"], got["per"]) == now, (first, max_groups, n, got)
                assert (got["threads"], got["rows_per_lane"]) == new[now[0]]
    assert grown > 0  # some of the cases the old tables refused now have a geometry
    # first=None is the option's default
    assert geometry_for(kernel, 5000, 80) == geometry_for(kernel, 5000, 80, default)


def test_one_million_nodes_fit():
    t = geometry_for(KERNEL_TBATCH, 1_000_000, 256, 1)
    assert t == {"index": 4, "threads": 512, "rows_per_lane": 8, "groups": 245, "per": 4096}
    b = geometry_for(KERNEL_BATCH, 1_000_000, 256, 0)
    assert b == {"index": 6, "threads": 512, "rows_per_lane": 8, "groups": 245, "per": 4095}
    for kernel in (KERNEL_BATCH, KERNEL_TBATCH):
        with pytest.raises(KgpuError) as ex:
            geometry_for(kernel, 1_048_577, 256, 0)
        assert ex.value.code == abi.E_CAPACITY


# ---- GPU runs
ROW_KEYS = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "num_pods")


def _check(w, got, rows_w, rows_g):
    for f in ("node", "feasible", "scored", "score"):
        bad = np.nonzero(w[f] != got[f])[0]
        assert len(bad) == 0, "%s differs at pods %s: want %s got %s" % (f, bad[:5], w[f][bad[:5]], got[f][bad[:5]])
    for k in rows_w:
        np.testing.assert_array_equal(rows_w[k], rows_g[k], err_msg=k)


def _upper_rows_hit(nodes, n_nodes, per, rows, threads=512):
    """Did a pod of the reference's own placements land in a row j >= rows / 2 of its workgroup
    (j = (node mod per) // threads)?  Then the upper rows' assume path ran.  Where the cluster is too
    small for any node to sit that high (a k_batch grid of 2048 nodes at 4095 per workgroup fills rows
    0-3 only; a forced geometry on 300 nodes fills row 0) the highest row that holds a node stands in."""
    top = min(rows // 2, (min(n_nodes, per) - 1) // threads)
    placed = nodes[nodes >= 0]
    return bool((((placed % per) // threads) >= top).any())


def _topo_run(args, groups=0, geo=None, threads=4):
    from oracle.cref import RefEngine
    nodes, ex, pods, services, rss = args
    fw = GpuFramework(Profile(), nodes, ex, cluster=Cluster(services=services, rss=rss), pods_hint=pods)
    q, pc, pnp, errs = fw.compile_pods(pods)
    assert not errs
    want = RefEngine(fw.config, fw.snap, threads=threads)
    w = want.schedule(q, pc)
    fw.engine.set_option(abi.OPT_TOPO_PERSISTENT, 1)
    if groups:
        fw.engine.set_option(abi.OPT_PERSIST_GROUPS, groups)
    if geo is not None:
        fw.engine.set_option(abi.OPT_TBATCH_GEO, geo)
    got, _ = fw.engine.schedule_batch(q, pc)
    used = fw.engine.geometry()
    rows = want.read_nodes(), fw.engine.read_nodes(fw.snap.n_nodes)
    fw.engine.close()
    return w, got, rows, used


@pytest.mark.gpu
@pytest.mark.parametrize("geo,rows", [(3, 4), (4, 8)])
@pytest.mark.parametrize("seed", [1, 4])
def test_gpu_tbatch_forced_geometry(seed, geo, rows):
    """KGPU_OPT_TBATCH_GEO 3 / 4 on 1,500 nodes: one workgroup whose rows 3 and up hold no node."""
    args = gen_random.topo_cluster(seed, n_nodes=1500, n_existing=600, n_pods=80)
    w, got, (rw, rg), used = _topo_run(args, geo=geo)
    _check(w, got, rw, rg)
    assert (used["kernel"], used["index"], used["threads"], used["rows_per_lane"]) == ("k_tbatch", geo, 512, rows)


# (workgroup cap, nodes, rows per lane, seed); seed 276 is the first whose reference run places a pod on
# node 2048, the only node of row 4
TBATCH_CAPPED = [(1, 2048, 4, 0), (1, 2049, 8, 276), (2, 6000, 8, 0),
                 (2, 3000, 4, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("groups,n_nodes,rows,seed", TBATCH_CAPPED)
def test_gpu_tbatch_capped_grid_fills_rows(groups, n_nodes, rows, seed):
    """A capped grid: 2,048 nodes on one workgroup fill every slot of 512 x 4; 2,049 put one node into
    row 4 of 512 x 8; 6,000 on two workgroups of 512 x 8 leave the last partly filled; 3,000 on two of
    512 x 4."""
    args = gen_random.topo_cluster(seed, n_nodes=n_nodes, n_existing=800, n_pods=80)
    w, got, (rw, rg), used = _topo_run(args, groups=groups)
    assert _upper_rows_hit(w["node"], n_nodes, 512 * rows, rows), "no placement in the upper rows: pick another seed"
    _check(w, got, rw, rg)
    assert (used["kernel"], used["threads"], used["rows_per_lane"], used["per"]) == ("k_tbatch", 512, rows, 512 * rows)
    assert used["groups"] == (n_nodes + 512 * rows - 1) // (512 * rows)


@pytest.mark.gpu
def test_gpu_tbatch_pod_affinity_one_workgroup():
    """The benchmark's config (d) shape at 3,000 nodes on one workgroup of 512 x 8."""
    nodes, ex, pods, _ = cluster.pod_affinity(n_nodes=3000, n_existing=3000, n_pods=160)
    w, got, (rw, rg), used = _topo_run((nodes, ex, pods, [], []), groups=1, threads=8)
    assert _upper_rows_hit(w["node"], 3000, 4096, 8)
    _check(w, got, rw, rg)
    assert (used["kernel"], used["index"], used["rows_per_lane"], used["groups"]) == ("k_tbatch", 4, 8, 1)


# (workgroup cap, KGPU_OPT_BATCH_GEO, nodes, seed): 2,048 nodes are one more than 512 x 4 holds on one
# workgroup; 4,095 fill 512 x 8 up to the spare slot; 4,096 put one node on a second workgroup; the
# forced geometry runs with every row but the first empty
BATCH_K8 = [(1, 0, 2048, 0), (1, 0, 4095, 0), (2, 0, 4096, 0), (0, 6, 300, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("groups,geo,n_nodes,seed", BATCH_K8)
def test_gpu_batch_eight_rows_per_lane(groups, geo, n_nodes, seed):
    """k_batch at 512 x 8 on the generic random clusters (pods with extended resources and host ports
    take the slow re-evaluation of the winning row)."""
    from oracle.cref import RefEngine
    nodes, existing, pods = gen_random.cluster(seed, n_nodes=n_nodes, n_existing=400, n_pods=120)
    fw = GpuFramework(Profile(), nodes, existing, pods_hint=pods)
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    ref = RefEngine(fw.config, fw.snap, threads=4)
    w = ref.schedule(q, pc)
    assert _upper_rows_hit(w["node"], n_nodes, 4095, 8), "no placement in the upper rows: pick another seed"
    fw.engine.set_option(abi.OPT_PERSISTENT, 1)
    fw.engine.set_option(abi.OPT_PERSIST_GROUPS, groups)
    fw.engine.set_option(abi.OPT_BATCH_GEO, geo)
    got, _ = fw.engine.schedule_batch(q, pc)
    used = fw.engine.geometry()
    _check(w, got, ref.read_nodes(), fw.engine.read_nodes(fw.snap.n_nodes))
    fw.engine.close()
    assert (used["kernel"], used["index"], used["threads"], used["rows_per_lane"], used["per"]) == ("k_batch", 6, 512, 8, 4095)
    assert used["groups"] == (n_nodes + 4094) // 4095


@pytest.mark.gpu
def test_gpu_pipelined_submit_on_one_workgroup():
    """kgpu_schedule_batch_submit / _wait with 3,000 nodes on one workgroup (512 x 8): two batches in
    flight, results equal to the C restatement (the old tables had no geometry: KGPU_E_UNSUPPORTED)."""
    from oracle.cref import RefEngine
    nodes, existing, pods, prof = cluster.fit_least_balanced(n_nodes=3000, n_pods=300)
    fw = GpuFramework(prof, nodes, existing, pods_hint=pods[:16])
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    ref = RefEngine(fw.config, fw.snap, threads=8)
    w = ref.schedule(q, pc)
    e = fw.engine
    e.set_option(abi.OPT_PERSIST_GROUPS, 1)
    e.schedule_batch_submit(q[:150], pc, first_seq=0)  # raises KgpuError unless KGPU_OK
    first_geo = e.geometry()
    e.schedule_batch_submit(q[150:], pc, first_seq=150)
    assert e.pipelined() == 2
    got = np.concatenate([e.schedule_batch_wait()[0], e.schedule_batch_wait()[0]])
    used = e.geometry()
    _check(w, got, ref.read_nodes(), e.read_nodes(fw.snap.n_nodes))
    e.close()
    for u in (first_geo, used):
        assert (u["kernel"], u["index"], u["rows_per_lane"], u["groups"]) == ("k_batch", 6, 8, 1)


def _shard_rank(rank, world, rdv, out):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://" + rdv, rank=rank, world_size=world)
    try:
        nodes, existing, pods, prof = cluster.fit_least_balanced(n_nodes=3000, n_pods=300)
        fw = GpuFramework(prof, nodes, existing, pods_hint=pods[:16], device=0, shard=(rank, world))
        # before the communicator: the sharded geometry is fixed when the ranks join
        fw.engine.set_option(abi.OPT_BATCH_GEO, 6)
        h = fw.engine.xgmi_handle(world)
        hs = [None] * world
        dist.all_gather_object(hs, h)
        fw.engine.xgmi_init(world, rank, b"".join(hs))
        assert fw.engine.xgmi_active()
        q, pc, _, errs = fw.compile_pods(pods)
        assert not errs
        res = []
        for b in range(0, len(pods), 100):
            res.append(fw.engine.schedule_batch(q[b:b + 100], pc, first_seq=b)[0])
        res = np.concatenate(res)
        used = fw.engine.geometry()
        rows = fw.engine.read_nodes(fw.snap.n_nodes)
        np.savez(out, node=res["node"], feasible=res["feasible"], score=res["score"], scored=res["scored"],
                 base=fw.snap.node_base, kernel=used["kernel"] or "", index=used["index"], rows_per_lane=used["rows_per_lane"],
                 **rows)
        fw.engine.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_sharded_eight_rows_per_lane(tmp_path):
    """The node-sharded (xGMI mailbox) instantiation of k_batch at 512 x 8: two ranks on one GPU, 1,500
    nodes each, against the C restatement of the unsharded cluster."""
    import os
    import tempfile

    import torch.multiprocessing as mp
    from oracle.cref import RefEngine
    nodes, existing, pods, prof = cluster.fit_least_balanced(n_nodes=3000, n_pods=300)
    world = 2
    ctx = mp.get_context("spawn")
    rdv = os.path.join(tempfile.mkdtemp(prefix="kgpu_rdv_"), "store")
    outs = [str(tmp_path / ("r%d.npz" % r)) for r in range(world)]
    procs = [ctx.Process(target=_shard_rank, args=(r, world, rdv, outs[r])) for r in range(world)]
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
    assert failed is None, failed  # nothing more runs after a failed child
    fw = GpuFramework(prof, nodes, existing, pods_hint=pods[:16], create_engine=False)
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    ref = RefEngine(fw.config, fw.snap, threads=8)
    want = ref.schedule(q, pc)
    rows = ref.read_nodes()
    assert (want["node"] >= 0).sum() > 0
    for r in range(world):
        got = np.load(outs[r])
        assert (str(got["kernel"]), int(got["index"]), int(got["rows_per_lane"])) == ("k_batch", 6, 8)
        for f in ("node", "feasible", "score", "scored"):
            assert np.array_equal(got[f], want[f]), (r, f, np.nonzero(got[f] != want[f])[0][:5])
        base = int(got["base"])
        n = len(got["num_pods"])
        for c in ROW_KEYS:
            assert np.array_equal(got[c], rows[c][base:base + n]), (r, c)
