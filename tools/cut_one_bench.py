#!/usr/bin/env python3
"""Latency of a kgpu_schedule_one cycle of a topology pod under percentageOfNodesToScore = 0 (the reference's
adaptive default), configs (c) and (d): the one-pod cut-mode run of k_tbatch (KGPU_OPT_CUT_TOPO_ONE 1) against the
per-pod topology pipeline (0, the default), alternated inside one job with a fresh engine per run, and the
pct = 100 one-pod cycle of the same job for scale.

  python tools/cut_one_bench.py --tag r14                 # c and d, 5,000 and 100,000 nodes, three alternated pairs
  python tools/cut_one_bench.py --configs c --nodes 5000 --only 1   # one mode, one size, no file

Every run schedules the same pods from the same compiled snapshot (classes prepared first, as the drop-in does
at upload), so the records of the two modes must be equal; the tool fails when they are not, or when a run left
the path its option names (kgpu_debug_counters out[8]).  One JSON line per run goes to
profiles/<tag>_cut_one_latency.jsonl (or --out), and a summary line per config and size: every pair's p50 gap,
the spread among the option-0 runs, and whether the smallest gap exceeds that spread."""
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

FIELDS = ("node", "feasible", "evaluated", "scored", "score")


def _inputs(config, n_nodes, n_pods):
    from kgpu import cluster
    if config == "c":
        return cluster.taints_affinity_spread(n_nodes=n_nodes, n_pods=n_pods)
    return cluster.pod_affinity(n_nodes=n_nodes, n_existing=n_nodes, n_pods=n_pods)


def one_run(fw, q, pc, option, warm):
    """A fresh engine, `warm` untimed cycles, then one timed cycle per remaining pod: (latencies in us, records,
    counters)."""
    from kgpu import abi
    from kgpu.native import Engine
    e = Engine(fw.config)
    try:
        e.upload(fw.snap, fw.arrays)
        if option is not None:
            e.set_option(abi.OPT_CUT_TOPO_ONE, option)
        e.prepare_pods(q, pc)
        for i in range(warm):
            e.schedule_one(q[i], pc, seq=i, assume=True)
        lat, out = [], []
        for i in range(warm, len(q)):
            t = time.perf_counter()
            res, _ = e.schedule_one(q[i], pc, seq=i, assume=True)
            lat.append((time.perf_counter() - t) * 1e6)
            out.append(tuple(int(res[f]) for f in FIELDS))
        return np.array(lat), out, e.counters()
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--configs", nargs="*", choices=["c", "d"], default=["c", "d"])
    ap.add_argument("--nodes", type=int, nargs="*", default=[5000, 100000])
    ap.add_argument("--pods", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", type=int, choices=[0, 1], default=None, help="one run of this option value, no file")
    ap.add_argument("--out", default=None, help="the JSON-lines file (default profiles/<tag>_cut_one_latency.jsonl)")
    args = ap.parse_args()
    from kgpu.framework import GpuFramework
    path = args.out or os.path.join(ROOT, "profiles", "%s_cut_one_latency.jsonl" % args.tag)
    lines, ok = [], True

    def stat(la):
        return {"p50_us": float(np.percentile(la, 50)), "p99_us": float(np.percentile(la, 99)), "mean_us": float(la.mean())}

    for cfg in args.configs:
        for n_nodes in args.nodes:
            nodes, ex, pods, prof = _inputs(cfg, n_nodes, args.pods + args.warmup)
            prof.percentage_of_nodes_to_score = 0
            fw = GpuFramework(prof, nodes, ex, pods_hint=pods, create_engine=False)
            q, pc, _, errs = fw.compile_pods(pods)
            assert not errs
            if args.only is not None:
                la, _, cnt = one_run(fw, q, pc, args.only, args.warmup)
                print(json.dumps({"config": cfg, "nodes": n_nodes, "option": args.only, **stat(la),
                                  "cut_topo_one_cycles": cnt["cut_topo_one_cycles"]}))
                continue
            runs = {0: [], 1: []}
            ref = None
            for pair in range(args.pairs):
                for option in (1, 0):
                    la, out, cnt = one_run(fw, q, pc, option, args.warmup)
                    if ref is None:
                        ref = out
                    same = ref == out
                    inside = cnt["cut_topo_one_cycles"]
                    ok &= same and (inside > 0 if option else inside == 0)
                    rec = {"kind": "run", "config": cfg, "nodes": n_nodes, "pods": len(la), "pct": 0, "pair": pair,
                           "cut_topo_one": option, **stat(la), "cut_topo_one_cycles": inside,
                           "persistent_launches": cnt["persistent_launches"], "records_equal": bool(same)}
                    runs[option].append(rec["p50_us"])
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
            prof100 = _inputs(cfg, 1, 1)[3]
            prof100.percentage_of_nodes_to_score = 100
            fw100 = GpuFramework(prof100, nodes, ex, pods_hint=pods, create_engine=False)
            q100, pc100, _, errs = fw100.compile_pods(pods)
            assert not errs
            la, _, cnt = one_run(fw100, q100, pc100, None, args.warmup)
            lines.append({"kind": "run", "config": cfg, "nodes": n_nodes, "pods": len(la), "pct": 100, **stat(la),
                          "persistent_launches": cnt["persistent_launches"]})
            print(json.dumps(lines[-1]), flush=True)
            gaps = [b - a for a, b in zip(runs[1], runs[0])]
            spread0 = max(runs[0]) - min(runs[0])
            summ = {"kind": "summary", "config": cfg, "nodes": n_nodes, "p50_us_one_pod_run": runs[1],
                    "p50_us_per_pod_pipeline": runs[0], "gap_p50_us": gaps, "option0_spread_p50_us": spread0,
                    "p50_us_pct100": lines[-1]["p50_us"], "every_pair_faster": bool(all(g > 0 for g in gaps)),
                    "gap_exceeds_option0_spread": bool(min(gaps) > spread0)}
            lines.append(summ)
            print(json.dumps(summ), flush=True)
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
        print("wrote", path)
    if not ok:
        raise SystemExit("records differ between the two modes, or a run left the expected path")


if __name__ == "__main__":
    main()
