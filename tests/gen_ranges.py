"""Value-range variants of gen_random's clusters (test infrastructure): node capacities and pod requests
on both sides of every threshold of the score arithmetic (2^24, 2^31 / 100, 2^52 / 100, 2^52, 2^53 and
the largest that keep 100 * quantity inside int64), and soft maxSkew values on both sides of 2^24.
gen_random's functions are untouched (other tests' seeds depend on their draw order): the values are
rewritten afterwards from a random.Random of their own."""
import random

import gen_random

# (cpu, memory) allocatable by class; classes 3|4 put 100 * cpu around 2^31, 5|6 100 * cap around 2^52,
# 7|8|9 the cap around 2^52, 10 = 2^56 (100 * cap < 2^63)
NODE_CLASSES = [
    ("0", "0"),
    ("40m", "64Mi"),  # below the default non-zero request (100m / 200Mi)
    ("2", "2Gi"),
    ("21474836m", "4Gi"),
    ("21474837m", "4294967297"),
    ("45035996273704m", "45035996273704"),
    ("45035996273705m", "45035996273705"),
    ("4503599627370495m", "4503599627370495"),
    ("4503599627370496m", "4503599627370496"),
    ("4503599627370497m", "4503599627370497"),
    ("72057594037927936m", "64Pi"),
]
POD_CPU = ["0", "1m", "10m", "500m", "21474m", "214748m", "45035996273m", "450359962737m", "45035996273704m",
           "720575940379279m"]
POD_MEM = ["0", "1", "1Mi", "1Gi", "42949673", "1Ti", "40Ti", "450359962737", "45035996273704", "640Ti"]
P_REQUEST = 0.85
SOFT_SKEWS = [1 << 22, 1 << 24, (1 << 25) + 1, (1 << 31) - 1]
P_SKEW = 0.7


def _requests(r, pod):
    c = pod["spec"]["containers"][0]
    req = c.setdefault("resources", {}).setdefault("requests", {})
    for res, values in (("cpu", POD_CPU), ("memory", POD_MEM)):
        req.pop(res, None)
        v = r.choice(values)
        if r.random() < P_REQUEST:
            req[res] = v
    pod["spec"].pop("initContainers", None)


def apply_value_classes(seed, nodes, existing, pods):
    """Rewrites the nodes' cpu / memory / pods allocatable to one of NODE_CLASSES and every pod's cpu and
    memory requests (existing pods too) in place; returns the class of each node, in `nodes` order."""
    r = random.Random(7000 + seed)
    classes = []
    for n in nodes:
        k = r.randrange(len(NODE_CLASSES))
        classes.append(k)
        n["status"]["allocatable"].update({"cpu": NODE_CLASSES[k][0], "memory": NODE_CLASSES[k][1], "pods": "110"})
    for p in list(existing) + list(pods):
        _requests(r, p)
    return classes


# Capacities c whose reciprocal products k * c * (1 / c) fall just below k for most k in 1..100 (1 / 17,
# 1 / 29 and 1 / 149 round down; the power-of-two factors change nothing): an exact multiple is then
# truncated to k - 1 and only ratio100's remainder step restores k.  Requests are multiples of c / 100, so
# the sums on a node keep landing on exact multiples.
STEP_CPU = ["1700m", "2900m", "14900m", "3400m"]
STEP_MEM = ["1700Mi", "2900Mi", "14900Mi", "6800Mi"]
STEP_POD_CPU = ["0", "17m", "29m", "149m", "170m", "290m", "34m"]
STEP_POD_MEM = ["0", "17Mi", "29Mi", "149Mi", "170Mi", "290Mi", "68Mi"]


def apply_step_values(seed, nodes, existing, pods):
    """Rewrites capacities and requests (as apply_value_classes does) to STEP_* values, in place."""
    r = random.Random(8000 + seed)
    for n in nodes:
        k = r.randrange(len(STEP_CPU))
        n["status"]["allocatable"].update({"cpu": STEP_CPU[k], "memory": STEP_MEM[r.randrange(len(STEP_MEM))], "pods": "110"})
    for p in list(existing) + list(pods):
        req = p["spec"]["containers"][0].setdefault("resources", {}).setdefault("requests", {})
        req["cpu"] = r.choice(STEP_POD_CPU)
        req["memory"] = r.choice(STEP_POD_MEM)
        p["spec"].pop("initContainers", None)
        p["spec"].pop("overhead", None)


def apply_soft_skews(seed, pods):
    """Rewrites the maxSkew of ScheduleAnyway constraints to one of SOFT_SKEWS with probability P_SKEW, in
    place (DoNotSchedule constraints keep theirs)."""
    r = random.Random(9000 + seed)
    for p in pods:
        for c in p["spec"].get("topologySpreadConstraints", []):
            if c["whenUnsatisfiable"] == "ScheduleAnyway":
                v = r.choice(SOFT_SKEWS)
                if r.random() < P_SKEW:
                    c["maxSkew"] = v


def topo_cluster(seed, n_nodes, n_existing, n_pods):
    nodes, existing, pods, services, rss = gen_random.topo_cluster(seed, n_nodes=n_nodes, n_existing=n_existing,
                                                                   n_pods=n_pods)
    apply_soft_skews(seed, pods)
    return nodes, existing, pods, services, rss
