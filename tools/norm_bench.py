#!/usr/bin/env python3
"""Pods that need a normalize pass, through kgpu_schedule_batch: one persistent launch of k_nbatch
(KGPU_OPT_NORM_PERSISTENT 1) against the per-pod pipeline (0: k_eval + k_final, under a cut k_eval + k_cut +
k_final), alternated inside one job on fresh engines.

Workload: the nodes and requests of cluster.fit_least_balanced plus zone labels, spot=true:PreferNoSchedule on
a fifth of the nodes; filters Fit, NodeAffinity, TaintToleration; scores Balanced, Least, NodeAffinity,
TaintToleration; every pod carries one preferred zone term, so every pod needs the normalize pass.  A second
mode (--mixed) gives the term -- and a toleration of the taint to all the others -- to every 8th pod only and
records option values 1, 4 and 16 with no threshold.

  python tools/norm_bench.py --tag r12               # 5,000 and 100,000 nodes, pct 100 and 0, three pairs
  python tools/norm_bench.py --tag r12 --mixed       # every 8th pod, option values 1, 4, 16 (and 0)
  python tools/norm_bench.py --nodes 5000 --pct 0 --only 1   # one run: the one to put under a kernel trace

Every run schedules the same pods on the same compiled snapshot, so the records of the two modes must be equal;
the tool fails when they are not.  One JSON line per run and a summary per point (every pair's gap, the spread
among the option-0 runs, gap_exceeds_option0_spread) go to profiles/<tag>_norm_bench.jsonl."""
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

ZONES = 8
FIELDS = ("node", "feasible", "evaluated", "scored", "score")


def workload(n_nodes, n_pods, pct, every=1):
    """(framework without an engine, queries, pools).  every > 1: only every `every`-th pod carries the
    preferred term and lacks the toleration; the others have constant maxima."""
    from kgpu import cluster
    from kgpu.compile import Profile
    from kgpu.framework import GpuFramework
    nodes, ex, pods, _ = cluster.fit_least_balanced(n_nodes=n_nodes, n_pods=n_pods, zones=ZONES)
    for i, n in enumerate(nodes):
        if i % 5 == 0:
            n["spec"]["taints"] = [{"key": "spot", "value": "true", "effect": "PreferNoSchedule"}]
    for i, p in enumerate(pods):
        if i % every == every - 1:
            p["spec"]["affinity"] = {"nodeAffinity": {"preferredDuringSchedulingIgnoredDuringExecution": [
                {"weight": 10, "preference": {"matchExpressions": [
                    {"key": cluster.ZONE, "operator": "In", "values": ["zone%d" % (i % ZONES)]}]}}]}}
        else:
            p["spec"]["tolerations"] = [{"key": "spot", "operator": "Exists", "effect": "PreferNoSchedule"}]
    prof = Profile(filters=["NodeResourcesFit", "NodeAffinity", "TaintToleration"],
                   scores=[("NodeResourcesBalancedAllocation", 1), ("NodeResourcesLeastAllocated", 1),
                           ("NodeAffinity", 1), ("TaintToleration", 1)],
                   percentage_of_nodes_to_score=pct)
    fw = GpuFramework(prof, nodes, ex, pods_hint=pods, create_engine=False)
    q, pc, _, errs = fw.compile_pods(pods)
    assert not errs
    return fw, q, pc


def one_run(fw, q, pc, batch, option, warm):
    """A fresh engine, `warm` untimed pods, then the rest in batches of `batch`: (seconds, device ms, records,
    persistent pods, k_nbatch pods)."""
    from kgpu import abi
    from kgpu.native import Engine
    e = Engine(fw.config)
    try:
        e.upload(fw.snap, fw.arrays)
        e.set_option(abi.OPT_NORM_PERSISTENT, option)
        e.schedule_batch(q[:warm], pc, first_seq=0)
        n0 = e.counters()["norm_persistent_pods"]
        out, inside, dev = [], 0, 0.0
        t0 = time.perf_counter()
        for k in range(warm, len(q), batch):
            res, st = e.schedule_batch(q[k:k + batch], pc, first_seq=k)
            out.append(res)
            dev += st.device_ms
            inside += e.instantiation()["persistent_pods"]
        dt = time.perf_counter() - t0
        return dt, dev, np.concatenate(out), inside, e.counters()["norm_persistent_pods"] - n0
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--nodes", type=int, nargs="*", default=[5000, 100000])
    ap.add_argument("--pct", type=int, nargs="*", default=[100, 0])
    ap.add_argument("--pods", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--mixed", action="store_true", help="every 8th pod needs the pass; option values 1, 4, 16, 0")
    ap.add_argument("--only", type=int, default=None, help="one run of this option value, no file")
    args = ap.parse_args()
    path = os.path.join(ROOT, "profiles", "%s_norm_bench.jsonl" % args.tag)
    every = 8 if args.mixed else 1
    lines, ok = [], True
    for n_nodes in args.nodes:
        for pct in args.pct:
            fw, q, pc = workload(n_nodes, args.pods + args.warmup, pct, every)
            n_timed = len(q) - args.warmup
            point = {"nodes": n_nodes, "pct": pct, "pods": n_timed, "batch": args.batch, "norm_every": every}
            if args.only is not None:
                dt, dev, _, inside, normp = one_run(fw, q, pc, args.batch, args.only, args.warmup)
                print(json.dumps({**point, "option": args.only, "us_per_pod": dt / n_timed * 1e6,
                                  "device_us_per_pod": dev * 1e3 / n_timed, "persistent_pods": inside,
                                  "norm_persistent_pods": normp}))
                continue
            values = (1, 4, 16, 0) if args.mixed else (1, 0)
            runs = {v: [] for v in values}
            devs = {v: [] for v in values}
            ref = None
            for pair in range(args.pairs):
                for option in values:
                    dt, dev, res, inside, normp = one_run(fw, q, pc, args.batch, option, args.warmup)
                    if ref is None:
                        ref = res
                    same = all(np.array_equal(ref[f], res[f]) for f in FIELDS)
                    ok &= same
                    if not args.mixed:  # every pod inside k_nbatch, or none
                        ok &= normp == (n_timed if option else 0)
                    rec = {**point, "kind": "run", "pair": pair, "norm_persistent": option, "seconds": dt,
                           "us_per_pod": dt / n_timed * 1e6, "device_us_per_pod": dev * 1e3 / n_timed,
                           "persistent_pods": inside, "norm_persistent_pods": normp, "records_equal": bool(same)}
                    runs[option].append(rec["us_per_pod"])
                    devs[option].append(rec["device_us_per_pod"])
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
            summ = {**point, "kind": "summary", "us_per_pod": {str(v): runs[v] for v in values},
                    "device_us_per_pod": {str(v): devs[v] for v in values}}
            if not args.mixed:
                gaps = [b - a for a, b in zip(runs[1], runs[0])]
                spread0 = max(runs[0]) - min(runs[0])
                summ.update({"gap_us_per_pod": gaps, "option0_spread_us": spread0,
                             "every_pair_faster": bool(all(g > 0 for g in gaps)),
                             "gap_exceeds_option0_spread": bool(min(gaps) > spread0)})
            lines.append(summ)
            print(json.dumps(summ), flush=True)
    if args.only is None:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a" if args.mixed else "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
        print("wrote", path)
    if not ok:
        raise SystemExit("records differ between the modes, or a run left the expected path")


if __name__ == "__main__":
    main()
