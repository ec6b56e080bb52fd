"""A seeded stream of informer / scheduler events over a kgpu.cache.SchedulerCache (test infrastructure).

Stream.step() draws one event (schedule + assume, confirm, forget, expire, pod add / update / delete, node
add / update / delete, pods on not-yet-known nodes) and records the node events for a nodeTree replay;
tests/test_delta.py drives it event by event.  tests/test_delta_routing.py steers it: force() applies one
named node event, and generic=True draws gen_random.rpod pods without topology terms on cluster() nodes.

What steering is for: UpdateSnapshot rebuilds Snapshot.List() from numNodes calls of nodeTree.next(), and
after a node ADD that pass starts mid-round, so the list holds one node twice (and skips another) until the
next node-set change; a node REMOVE resets the tree's round and gives a list without duplicates.
"""
import copy
import random

import gen_random
from oracle.refsched import framework as F
from oracle.refsched import nodeinfo as NI
from kgpu.cache import CacheError

NEW_LABEL_KEY = "delta-stream/rack"  # no node of gen_random carries it: SET_NODE cannot absorb it (NeedsUpload)


class Stream:
    """Random cache events over a SchedulerCache, recording the node events for a nodeTree replay."""

    def __init__(self, seed, cache, nodes, services, rss, gpu, generic=False):
        self.r = random.Random(seed)
        self.c = cache
        self.gpu = gpu
        self.generic = generic  # rpod pods without topology terms, node adds keep rnode's allocatable
        self.services, self.rss = services, rss
        self.assumed = {}     # uid -> pod
        self.added = {}       # uid -> pod
        self.node_events = [("add", n) for n in nodes]
        self.next_pod = 0
        self.next_node = len(nodes)
        self.t = 0.0
        self.seq = 0

    def fresh_pod(self, bound_to=None):
        r = self.r
        names = list(self.c.nodes)
        p = gen_random.rpod(r, 50000 + self.next_pod, names, allow_node_name=False)
        if not self.generic:
            gen_random._topo_spec(r, p["spec"], p["metadata"], p_tsc=0.4, p_aff=0.4)
        p["metadata"]["uid"] = "s%d" % self.next_pod
        p["metadata"]["name"] = "s%d" % self.next_pod
        self.next_pod += 1
        if bound_to is not None:
            p["spec"]["nodeName"] = bound_to
        return p

    def step(self):
        r, c = self.r, self.c
        op = r.choices(["sched", "confirm", "forget", "expire", "add", "remove", "update", "node_update",
                        "node_add", "node_remove", "ghost"],
                       weights=[6, 3, 2, 1, 3, 3, 2, 3, 1, 1, 1])[0]
        if op == "sched":
            p = self.fresh_pod()
            host = self.schedule_probe(p) if self.gpu else r.choice(list(c.nodes))
            if host is None:
                return op
            p["spec"]["nodeName"] = host
            c.assume_pod(p)
            self.assumed[p["metadata"]["uid"]] = p
        elif op == "confirm" and self.assumed:
            uid = r.choice(sorted(self.assumed))
            p = self.assumed.pop(uid)
            if r.random() < 0.2 and c.nodes:
                p = copy.deepcopy(p)
                p["spec"]["nodeName"] = r.choice(sorted(c.nodes))   # bound elsewhere (cache.go:470-477)
            c.add_pod(p)
            self.added[uid] = p
        elif op == "forget" and self.assumed:
            uid = r.choice(sorted(self.assumed))
            c.forget_pod(self.assumed.pop(uid))
        elif op == "expire" and self.assumed:
            uid = r.choice(sorted(self.assumed))
            c.finish_binding(self.assumed[uid], self.t)
            self.t += c.ttl + 1
            c.cleanup_assumed(self.t)
            self.assumed = {u: p for u, p in self.assumed.items() if u in c.states}
        elif op == "add" and c.nodes:
            p = self.fresh_pod(bound_to=r.choice(sorted(c.nodes)))
            c.add_pod(p)
            self.added[p["metadata"]["uid"]] = p
        elif op == "ghost":
            p = self.fresh_pod(bound_to="ghost%d" % r.randrange(3))
            c.add_pod(p)
            self.added[p["metadata"]["uid"]] = p
        elif op == "remove" and self.added:
            uid = r.choice(sorted(self.added))
            p = self.added.pop(uid)
            try:
                c.remove_pod(p)
            except CacheError:
                pass  # the pod's node was deleted and re-added: NodeInfo.RemovePod fails, as in the reference
        elif op == "update" and self.added:
            uid = r.choice(sorted(self.added))
            old = self.added[uid]
            new = copy.deepcopy(old)
            new["metadata"]["labels"] = {"app": r.choice(gen_random.APPS)}
            cont = new["spec"]["containers"][0]
            cont.setdefault("resources", {}).setdefault("requests", {})["cpu"] = "%dm" % r.choice([10, 700])
            try:
                c.update_pod(old, new)
                self.added[uid] = new
            except CacheError:
                pass
        elif op == "node_update" and c.nodes:
            nm = r.choice(sorted(c.nodes))
            old = c.nodes[nm]
            new = copy.deepcopy(old)
            lab = new["metadata"]["labels"]
            if r.random() < 0.5:
                lab[gen_random.ZONE] = "z%d" % r.randrange(4)          # may be a new value (dictionary growth)
            if r.random() < 0.3:
                lab["disk"] = r.choice(["ssd", "hdd", "nvme"])
            if r.random() < 0.3 and "disk" in lab:
                del lab["disk"]
            new["status"]["allocatable"]["cpu"] = "%dm" % r.choice([500, 4000, 64000])
            new["spec"]["unschedulable"] = r.random() < 0.1
            if r.random() < 0.3:
                new["spec"]["taints"] = [{"key": "spot", "value": "true", "effect": "PreferNoSchedule"}]
            c.update_node(old, new)
            self.node_events.append(("update", old, new))
        elif op == "node_add":
            if r.random() < 0.5:
                nm = "ghost%d" % r.randrange(3)
                if nm in c.nodes:
                    return op
                n = gen_random.rnode(r, 0)
                n["metadata"]["name"] = nm
                n["metadata"]["labels"][gen_random.HOST] = nm
            else:
                n = gen_random.rnode(r, self.next_node)
                self.next_node += 1
            if not self.generic:
                n["status"]["allocatable"].update({"cpu": "64", "memory": "256Gi", "pods": "110"})
            c.add_node(n)
            self.node_events.append(("add", n))
        elif op == "node_remove" and len(c.nodes) > 4:
            nm = r.choice(sorted(c.nodes))
            n = c.nodes[nm]
            c.remove_node(n)
            self.node_events.append(("remove", n))
        return op

    def force(self, op):
        """One steered node event: "node_remove" (a random node), "node_add" (a new node, never a ghost
        name) or "node_new_label_key" (a node update that introduces NEW_LABEL_KEY)."""
        r, c = self.r, self.c
        if op == "node_remove":
            n = c.nodes[r.choice(sorted(c.nodes))]
            c.remove_node(n)
            self.node_events.append(("remove", n))
        elif op == "node_add":
            n = gen_random.rnode(r, self.next_node)
            self.next_node += 1
            if not self.generic:
                n["status"]["allocatable"].update({"cpu": "64", "memory": "256Gi", "pods": "110"})
            c.add_node(n)
            self.node_events.append(("add", n))
        elif op == "node_new_label_key":
            old = c.nodes[r.choice(sorted(c.nodes))]
            new = copy.deepcopy(old)
            new["metadata"]["labels"][NEW_LABEL_KEY] = "r%d" % r.randrange(3)
            c.update_node(old, new)
            self.node_events.append(("update", old, new))
        else:
            raise ValueError(op)
        return op

    def schedule_probe(self, pod):
        host, res = self.c.schedule(pod, seq=self.seq)
        want = F.schedule_sequence(self.c.ordered_nodes(), self.c.listed_pods(), [pod], F.Profile(),
                                   services=self.services, rss=self.rss, first_seq=self.seq, order="given",
                                   image_nodes=list(self.c.nodes.values()))[0]
        self.seq += 1
        if isinstance(want, F.ScheduleError):
            assert int(res["node"]) < 0, "oracle: %s, device placed on %s" % (want, host)
            return None
        assert host == want.host, "device %s vs oracle %s" % (host, want.host)
        assert int(res["feasible"]) == want.feasible
        if want.feasible > 1:
            assert int(res["score"]) == dict(want.totals)[want.host]
        return host

    def check_rows(self):
        c = self.c
        snap = NI.Snapshot(c.ordered_nodes(), c.listed_pods(), order="given")
        rows = c.engine.read_nodes(len(c.list))
        for i, ni in enumerate(snap.list):
            got = (int(rows["req_cpu"][i]), int(rows["req_mem"][i]), int(rows["nz_cpu"][i]), int(rows["nz_mem"][i]),
                   int(rows["num_pods"][i]))
            want = (ni.requested.milli_cpu, ni.requested.memory, ni.non_zero.milli_cpu, ni.non_zero.memory,
                    len(ni.pods))
            assert got == want, "node %s row %r vs oracle %r" % (c.list[i], got, want)
