"""ksched_schedule_affinity without a GPU: the CPU restatement (affinity_ref) on the worked example of include/ksched.h's
rules, the entry points' argument check and the binding's constant, and ksched.host's parsing and affinity_tables."""
import ctypes as C
import json

import numpy as np
import pytest

import affinity_ref as AR

ZONE = "topology.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"


def test_worked_example_reference(oracle_mod):
    c = AR.worked_example()
    idx, score, feas, nm, nah, naz, state, info = AR.schedule_affinity(oracle_mod, c)
    assert idx.tolist() == [0, 1, 0, 1, -1, 2, 3, 0, 0]
    assert feas.tolist() == [4, 3, 3, 1, 0, 2, 1, 4, 2]
    assert nm.tolist() == [7, 3, 1, 1] and nah.tolist() == [1, 1, 1, 0] and naz.tolist() == [2, 2, 0, 0]
    price = [float(np.float32(x)) for x in (0.1, 0.2, 0.3, 0.4)]
    assert score.tolist() == [price[0], price[1], price[0], price[1], 0.0, price[2], price[3], price[0], price[0]]
    assert state[0].tolist() == [64000 - 400, 64000 - 200, 64000 - 100, 64000 - 100] and state[2].tolist() == [106, 108, 109, 109]
    # p1 p2 p3 p5 lose nodes to their own terms, p6 to the bound pods' (the symmetric half); p2 p3 p8 need web / db
    # nearby; p7 is waived; p4 fits everywhere and is eligible nowhere; p0-p3 and p7 add bits to a zone word; p6 lands on
    # the node without the key
    assert info.pop("zone_moved_at") == [0, 1, 2, 3, 7]
    assert info == dict(own_anti=4, symmetric=1, aff_narrowed=4, waived=1, aff_nofit=1, zone_moved=5, off_domain=1, moved=5)
    assert oracle_mod.schedule(c.cl)[0].tolist() == [0] * 9


@pytest.mark.parametrize("labels", [False, True])
def test_empty_pods_are_the_plain_schedule(labels, oracle_mod):
    c = AR.adversarial(9, 64, 256, 4, 3, domain=1, labels=labels)
    p = c.cl.n_pods
    want = oracle_mod.schedule(c.cl)
    z = np.zeros(p, np.uint64)
    empty = AR.dataclasses.replace(c, member=z, anti_host=z, anti_zone=z, aff_group=np.full(p, -1, np.int32))
    got = AR.schedule_affinity(oracle_mod, empty)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert np.array_equal(got[2], want[2]) and all(np.array_equal(a, b) for a, b in zip(got[6], want[3]))
    assert all(np.array_equal(a, b) for a, b in zip(got[3:6], c.table()[1:])) and (got[0] >= 0).any()
    assert c.node_member.any() and c.node_anti_host.any()  # (a table that would bar pods with words)


def test_null_context_is_invalid_and_constant():
    from ksched import _lib as L
    assert L.AFF_MAX_GROUPS == 64
    lb = L.lib()
    assert lb.ksched_schedule_affinity(None, 0, *([None] * 12)) == L.E_INVALID
    one = np.zeros(1, np.uint64)
    assert lb.ksched_load_affinity(None, 0, None, L.ptr(one, C.c_uint64), None, None) == L.E_INVALID
    assert lb.ksched_read_affinity(None, L.ptr(one, C.c_uint64), None, None) == L.E_INVALID
    header = open(L.HEADER_PATH).read()
    assert any(ln.split()[:3] == ["#define", "KSCHED_AFF_MAX_GROUPS", "64"] for ln in header.splitlines())


def kube_json():
    """Five nodes -- n0 n1 in zone a, n2 n3 in zone b, n4 without the zone label -- priced n0 < n1 < ... < n4.  Bound: a
    web replica on n0 that carries the Deployment's hostname anti-affinity, and a `solo` pod on n2 that refuses app=cache
    in its whole zone.  Pending: three more web replicas (one per node), two caches (zone affinity to web, one per
    zone), a third cache, and a plain pod."""
    from ksched.host import PRICE_ANNOTATION, SCHEDULER_ANNOTATION

    def node(name, zone):
        return {"metadata": {"name": name, "labels": {HOST: name, **({ZONE: zone} if zone else {})},
                             "annotations": {PRICE_ANNOTATION: f"0.{int(name[1]) + 1}0"}},
                "status": {"capacity": {"cpu": "8", "memory": "16777216Ki", "pods": "110"}}}

    def term(app, key):
        return {"labelSelector": {"matchLabels": {"app": app}}, "topologyKey": key}

    def pod(name, app, node_name="", affinity=None, anti=None):
        spec = {"nodeName": node_name, "containers": [{"name": "c", "resources": {"requests": {"cpu": "100m"}}}]}
        aff = {}
        if affinity:
            aff["podAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": affinity,
                                  "preferredDuringSchedulingIgnoredDuringExecution": [
                                      {"weight": 1, "podAffinityTerm": term("ignored", "rack")}]}
        if anti:
            aff["podAntiAffinity"] = {"requiredDuringSchedulingIgnoredDuringExecution": anti}
        if aff:
            spec["affinity"] = aff
        return {"metadata": {"name": name, "labels": {"app": app}, "annotations": {SCHEDULER_ANNOTATION: "hightower"}},
                "spec": spec}

    web = dict(anti=[term("web", HOST)])
    cache = dict(affinity=[term("web", ZONE)], anti=[term("cache", ZONE)])
    nodes = {"items": [node("n0", "a"), node("n1", "a"), node("n2", "b"), node("n3", "b"), node("n4", None)]}
    pods = {"items": [pod("web-0", "web", "n0", **web), pod("solo", "solo", "n2", anti=[term("cache", ZONE)])] +
                     [pod(f"web-{i}", "web", **web) for i in (1, 2, 3)] +
                     [pod(f"cache-{i}", "cache", **cache) for i in (0, 1, 2)] + [pod("plain", "other")]}
    return nodes, pods


def test_pod_from_kube_affinity():
    from ksched.host import AffinityTerm, pod_from_kube
    _, pods = kube_json()
    w = pod_from_kube(pods["items"][2])
    assert w.name == "web-1" and w.affinity == ()
    assert w.anti_affinity == (AffinityTerm(topology_key=HOST, match_labels=(("app", "web"),)),)
    c = pod_from_kube(pods["items"][5])
    assert c.affinity == (AffinityTerm(topology_key=ZONE, match_labels=(("app", "web"),)),)  # the preferred term is ignored
    assert c.anti_affinity == (AffinityTerm(topology_key=ZONE, match_labels=(("app", "cache"),)),)
    assert c.affinity[0].matches(w.labels) and not c.affinity[0].matches(c.labels)
    assert pod_from_kube({}).affinity == () and pod_from_kube({"spec": {"affinity": {}}}).anti_affinity == ()
    assert pod_from_kube(json.loads(json.dumps(pods["items"][5]))) == c
    bad = json.loads(json.dumps(pods["items"][5]))
    bad["spec"]["affinity"]["podAffinity"]["requiredDuringSchedulingIgnoredDuringExecution"][0]["labelSelector"] = {
        "matchExpressions": [{"key": "app", "operator": "In", "values": ["web"]}]}
    with pytest.raises(ValueError, match="matchLabels only"):
        pod_from_kube(bad)


def tables():
    from ksched.host import node_from_kube, pod_from_kube
    nl, pl = kube_json()
    nodes = [node_from_kube(x) for x in nl["items"]]
    pods = [pod_from_kube(x) for x in pl["items"]]
    return nodes, [p for p in pods if p.node_name], [p for p in pods if not p.node_name]


def kube_case():
    """affinity_tables on kube_json(), as a reference case (the cluster restates the nodes' capacity and price)."""
    from ksched import cluster
    from ksched.host import affinity_tables
    nodes, bound, pending = tables()
    cl = cluster.Cluster(name="kube", alloc_cpu=np.full(5, 8000, np.int64), alloc_mem=np.full(5, 1 << 24, np.int64),
                         alloc_pods=np.full(5, 110, np.int64), req_cpu=np.full(7, 100, np.int64),
                         req_mem=np.zeros(7, np.int64), req_pods=np.ones(7, np.int64),
                         price=np.array([0.1, 0.2, 0.3, 0.4, 0.5], np.float32), priority=cluster.PRIORITY_BEST_PRICE,
                         domain=cluster.DOMAIN_FEASIBLE)
    cl.alloc_cpu[[0, 2]] -= 100  # the bound pods
    cl.alloc_pods[[0, 2]] -= 1
    return AR.Case(cl, 2, *affinity_tables(nodes, bound, pending))


def test_affinity_tables():
    c = kube_case()
    dom, nm, nah, naz, member, ah, az, ag, azs = c.table() + c.pods()
    WEB, CACHE = 1, 2  # the vocabulary, in the pending pods' order: app=web, app=cache
    assert dom.tolist() == [0, 0, 1, 1, -1] and dom.dtype == np.int32
    assert nm.tolist() == [WEB, 0, 0, 0, 0] and nm.dtype == np.uint64          # web-0 on n0; `solo` is in no group
    assert nah.tolist() == [WEB, 0, 0, 0, 0] and naz.tolist() == [0, 0, CACHE, 0, 0]
    assert member.tolist() == [WEB] * 3 + [CACHE] * 3 + [0] and member.dtype == np.uint64
    assert ah.tolist() == [WEB] * 3 + [0] * 4 and az.tolist() == [0] * 3 + [CACHE] * 3 + [0]
    assert ag.tolist() == [-1] * 3 + [0] * 3 + [-1] and ag.dtype == np.int32
    assert azs.tolist() == [0] * 3 + [1] * 3 + [0] and azs.dtype == np.uint8


def test_affinity_tables_reference(oracle_mod):
    # web one per node, cheapest first (n0 is taken); zone b refuses caches (`solo`), so one cache goes to zone a and the
    # others fit nowhere; `plain` takes the cheapest node
    c = kube_case()
    idx, _, feas = AR.schedule_affinity(oracle_mod, c)[:3]
    assert idx.tolist() == [1, 2, 3, 0, -1, -1, 0] and feas.tolist() == [4, 3, 2, 2, 0, 0, 5]


def test_affinity_tables_errors():
    from ksched import _lib as L
    from ksched.host import AffinityTerm, affinity_tables
    nodes, bound, pending = tables()
    # no zone key among the terms: every node -1, no domain
    dom = affinity_tables(nodes, bound[:1], pending[:3])[0]
    assert dom.tolist() == [-1] * 5
    rack = AffinityTerm(topology_key="rack", match_labels=(("app", "web"),))
    pending[0].anti_affinity += (rack,)
    with pytest.raises(ValueError, match="one zone key"):
        affinity_tables(nodes, bound, pending)
    nodes, bound, pending = tables()
    pending[3].affinity += (AffinityTerm(topology_key=ZONE, match_labels=(("app", "db"),)),)
    with pytest.raises(ValueError, match="one is supported"):
        affinity_tables(nodes, bound, pending)
    nodes, bound, pending = tables()
    many = tuple(AffinityTerm(topology_key=HOST, match_labels=(("app", f"a{k}"),)) for k in range(L.AFF_MAX_GROUPS - 2))
    pending[-1].anti_affinity = many
    assert int(affinity_tables(nodes, bound, pending)[5][-1]) == (1 << 64) - 4  # 64 groups: bits 2-63
    pending[-1].anti_affinity = many + (AffinityTerm(topology_key=HOST, match_labels=(("app", "one-more"),)),)
    with pytest.raises(ValueError, match="at most 64"):
        affinity_tables(nodes, bound, pending)
