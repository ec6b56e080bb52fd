#!/usr/bin/env python3
"""percentageOfNodesToScore = 0 (the reference's adaptive default) on config (b), (c) or (d), through
kgpu_schedule_batch: the cut-mode persistent kernel (option 1) against the per-pod cut pipeline (0, the path
before the option existed), alternated inside one job, and the pct = 100 persistent run of the same job for
scale.  Config b alternates KGPU_OPT_CUT_PERSISTENT (k_cbatch, pct = 100: k_batch); c and d -- the topology
configs, cluster.taints_affinity_spread and cluster.pod_affinity at full node count -- alternate
KGPU_OPT_CUT_TOPO_PERSISTENT (k_tbatch's cut mode, pct = 100: k_tbatch).

  python tools/pct_bench.py --tag r10                 # 5,000 and 100,000 nodes, three alternated pairs
  python tools/pct_bench.py --config c --tag r11      # the same for config (c): profiles/r11_pct_topo_bench.jsonl
  python tools/pct_bench.py --nodes 5000 --only 1     # one mode, one size: the run to put under a
                                                      # kernel trace (rocprofv3 --kernel-trace --stats -- ...)

Every run starts from a fresh engine on the same compiled snapshot and schedules the same pods, so the
placements of the two modes must be equal; the tool fails when they are not.  One JSON line per run goes
to profiles/<tag>_pct_bench.jsonl (c, d: <tag>_pct_topo_bench.jsonl, appended per config), and a summary line per size: every pair's gap, the spread among the
option-0 runs, and microseconds per pod against pct = 100."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kubernetes-1_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _inputs(config, n_nodes, n_pods):
    from kgpu import cluster
    if config == "b":
        return cluster.fit_least_balanced(n_nodes=n_nodes, n_pods=n_pods)
    if config == "c":
        return cluster.taints_affinity_spread(n_nodes=n_nodes, n_pods=n_pods)
    return cluster.pod_affinity(n_nodes=n_nodes, n_existing=n_nodes, n_pods=n_pods)


def one_run(fw, q, pc, batch, option, warm, config="b"):
    """A fresh engine, `warm` untimed pods, then the rest in batches of `batch`: (seconds, device ms,
    records, persistent pods, cut-mode pods of the config's kernel)."""
    from kgpu import abi
    from kgpu.native import Engine
    e = Engine(fw.config)
    try:
        e.upload(fw.snap, fw.arrays)
        if option is not None:
            e.set_option(abi.OPT_CUT_PERSISTENT if config == "b" else abi.OPT_CUT_TOPO_PERSISTENT, option)
        e.schedule_batch(q[:warm], pc, first_seq=0)
        out, inside, dev = [], 0, 0.0
        t0 = time.perf_counter()
        for k in range(warm, len(q), batch):
            res, st = e.schedule_batch(q[k:k + batch], pc, first_seq=k)
            out.append(res)
            dev += st.device_ms
            inside += e.instantiation()["persistent_pods"]
        dt = time.perf_counter() - t0
        return dt, dev, np.concatenate(out), inside, e.counters()["cut_persistent_pods" if config == "b"
                                                                  else "cut_topo_persistent_pods"]
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--config", choices=["b", "c", "d"], default="b")
    ap.add_argument("--nodes", type=int, nargs="*", default=[5000, 100000])
    ap.add_argument("--pods", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", type=int, choices=[0, 1], default=None, help="one run of this option value, no file")
    args = ap.parse_args()
    from kgpu.framework import GpuFramework
    cfg, topo = args.config, args.config != "b"
    tagc = {"config": cfg} if topo else {}  # config b keeps its records as they were
    path = os.path.join(ROOT, "profiles", "%s_pct_%sbench.jsonl" % (args.tag, "topo_" if topo else ""))
    lines, ok = [], True
    for n_nodes in args.nodes:
        nodes, ex, pods, prof = _inputs(cfg, n_nodes, args.pods + args.warmup)
        prof.percentage_of_nodes_to_score = 0
        fw = GpuFramework(prof, nodes, ex, pods_hint=pods, create_engine=False)
        q, pc, _, errs = fw.compile_pods(pods)
        assert not errs
        n_timed = len(q) - args.warmup
        if args.only is not None:
            dt, dev, _, inside, cutp = one_run(fw, q, pc, args.batch, args.only, args.warmup, cfg)
            print(json.dumps({**tagc, "nodes": n_nodes, "option": args.only, "us_per_pod": dt / n_timed * 1e6,
                              "persistent_pods": inside}))
            continue
        prof100 = _inputs(cfg, 1, 1)[3]
        prof100.percentage_of_nodes_to_score = 100
        fw100 = GpuFramework(prof100, nodes, ex, pods_hint=pods, create_engine=False)
        q100, pc100, _, errs = fw100.compile_pods(pods)
        assert not errs
        runs = {0: [], 1: []}
        ref = None
        for pair in range(args.pairs):
            for option in (1, 0):
                dt, dev, res, inside, cutp = one_run(fw, q, pc, args.batch, option, args.warmup, cfg)
                if ref is None:
                    ref = res
                same = all(np.array_equal(ref[f], res[f]) for f in ("node", "feasible", "evaluated", "scored", "score"))
                # (c, d: a pod without topology state runs in k_cbatch under either value; the counter of the
                # config's own kernel must cover every other pod, and none with the option off)
                ok &= same and ((inside == (n_timed if option else 0)) if not topo else
                                (cutp > 0 and inside == n_timed) if option else cutp == 0)
                rec = {**tagc, "kind": "run", "nodes": n_nodes, "pods": n_timed, "batch": args.batch, "pct": 0, "pair": pair,
                       "cut_persistent": option, "seconds": dt, "us_per_pod": dt / n_timed * 1e6,
                       "device_us_per_pod": dev * 1e3 / n_timed, "persistent_pods": inside,
                       "cut_topo_persistent_pods" if topo else "cut_persistent_pods": cutp,
                       "placements_equal": bool(same)}
                runs[option].append(rec["us_per_pod"])
                lines.append(rec)
                print(json.dumps(rec), flush=True)
        full = []
        for _ in range(2):
            dt, dev, _, inside, _ = one_run(fw100, q100, pc100, args.batch, None, args.warmup, cfg)
            full.append(dt / n_timed * 1e6)
            lines.append({**tagc, "kind": "run", "nodes": n_nodes, "pods": n_timed, "batch": args.batch, "pct": 100,
                          "us_per_pod": full[-1], "device_us_per_pod": dev * 1e3 / n_timed, "persistent_pods": inside})
            print(json.dumps(lines[-1]), flush=True)
        gaps = [b - a for a, b in zip(runs[1], runs[0])]
        spread0 = max(runs[0]) - min(runs[0])
        summ = {**tagc, "kind": "summary", "nodes": n_nodes, "us_per_pod_persistent": runs[1], "us_per_pod_per_pod": runs[0],
                "gap_us_per_pod": gaps, "option0_spread_us": spread0, "us_per_pod_pct100": full,
                "every_pair_faster": bool(all(g > 0 for g in gaps)),
                "gap_exceeds_option0_spread": bool(min(gaps) > spread0)}
        lines.append(summ)
        print(json.dumps(summ), flush=True)
    if args.only is None:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a" if topo else "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
        print("wrote", path)
    if not ok:
        raise SystemExit("placements differ between the two modes, or a run left the expected path")


if __name__ == "__main__":
    main()
