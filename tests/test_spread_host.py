"""ksched_schedule_spread without a GPU: the CPU restatement (spread_ref) on the worked example of include/ksched.h's
rules, the entry points' argument check and the binding's constants, and ksched.host's parsing and spread_tables."""
import ctypes as C
import json

import numpy as np
import pytest

import spread_ref as SR

ZONE = "topology.kubernetes.io/zone"


def test_worked_example_reference(oracle_mod):
    cl, dom, skew, counts, group, enforce = SR.worked_example()
    idx, score, feas, cnt, state, info = SR.schedule_spread(oracle_mod, cl, dom, skew, counts, group, enforce)
    assert idx.tolist() == [0, 2, 0, 2]
    assert feas.tolist() == [3, 1, 3, 1]
    assert cnt.tolist() == [[2, 2]]
    assert score.tolist() == [float(np.float32(0.1)), 0.5, float(np.float32(0.1)), 0.5]
    assert state[0].tolist() == [64000 - 200, 64000, 64000 - 200] and state[2].tolist() == [108, 110, 108]
    assert info == dict(narrowed=2, moved=2, spread_nofit=0, min_rose=2, count_only=0, off_domain=0)
    assert oracle_mod.schedule(cl)[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("labels", [False, True])
def test_no_groups_is_the_plain_schedule(labels, oracle_mod):
    cl, dom, skew, counts, group, enforce = SR.adversarial(7, 64, 256, 4, 3, domain=1, labels=labels)
    want = oracle_mod.schedule(cl)
    got = SR.schedule_spread(oracle_mod, cl, dom, skew, counts, np.full(cl.n_pods, -1), enforce)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert np.array_equal(got[2], want[2]) and all(np.array_equal(a, b) for a, b in zip(got[4], want[3]))
    assert np.array_equal(got[3], counts) and (got[0] >= 0).any()


def test_null_context_is_invalid_and_constants():
    from ksched import _lib as L
    assert (L.SPREAD_MAX_DOMAINS, L.SPREAD_MAX_GROUPS, L.SPREAD_MAX_CELLS) == (1024, 64, 4096)
    lb = L.lib()
    assert lb.ksched_schedule_spread(None, 0, None, None, None, None, None, None, None, None, None) == L.E_INVALID
    one = np.zeros(1, np.int32)
    assert lb.ksched_load_spread(None, 1, L.ptr(one, C.c_int32), 1, L.ptr(one, C.c_int32), None) == L.E_INVALID
    assert lb.ksched_read_spread(None, L.ptr(one, C.c_int32)) == L.E_INVALID
    header = open(L.HEADER_PATH).read()
    for name, value in (("KSCHED_SPREAD_MAX_DOMAINS", 1024), ("KSCHED_SPREAD_MAX_GROUPS", 64), ("KSCHED_SPREAD_MAX_CELLS", 4096)):
        assert any(ln.split()[:3] == ["#define", name, str(value)] for ln in header.splitlines()), name


def kube_json():
    """6 nodes in 3 zones (a: n0 n1 n5, b: n2 n3, c: n4) and n6 without the zone label, priced n6 < n0 < ... < n5; two
    bound replicas of app=web (on n0 in a, n2 in b) and a bound pod of another app; 7 pending replicas with maxSkew 1
    over the zone, one pending pod that matches the selector without a constraint, one pending pod of another app."""
    from ksched.host import PRICE_ANNOTATION, SCHEDULER_ANNOTATION

    def node(name, zone):
        price = "0.05" if zone is None else f"0.{int(name[1]) + 1}0"
        return {"metadata": {"name": name, "labels": {"kubernetes.io/hostname": name, **({ZONE: zone} if zone else {})},
                             "annotations": {PRICE_ANNOTATION: price}},
                "status": {"capacity": {"cpu": "8", "memory": "16777216Ki", "pods": "110"}}}

    def pod(name, app, node_name="", spread=True):
        spec = {"nodeName": node_name, "containers": [{"name": "c", "resources": {"requests": {"cpu": "100m"}}}]}
        if spread:
            spec["topologySpreadConstraints"] = [
                {"maxSkew": 2, "topologyKey": ZONE, "whenUnsatisfiable": "ScheduleAnyway",
                 "labelSelector": {"matchLabels": {"app": app}}},
                {"maxSkew": 1, "topologyKey": ZONE, "whenUnsatisfiable": "DoNotSchedule",
                 "labelSelector": {"matchLabels": {"app": app}}}]
        return {"metadata": {"name": name, "labels": {"app": app, "rev": "1"},
                             "annotations": {SCHEDULER_ANNOTATION: "hightower"}}, "spec": spec}

    nodes = {"items": [node("n0", "a"), node("n1", "a"), node("n2", "b"), node("n3", "b"), node("n4", "c"),
                       node("n5", "a"), node("n6", None)]}
    pods = {"items": [pod("b0", "web", "n0"), pod("b1", "web", "n2"), pod("b2", "db", "n4", spread=False)] +
                     [pod(f"w{i}", "web") for i in range(7)] + [pod("plain", "web", spread=False),
                                                                pod("other", "db", spread=False)]}
    return nodes, pods


def test_pod_from_kube_spread():
    from ksched.host import SpreadConstraint, pod_from_kube
    _, pods = kube_json()
    w0 = pod_from_kube(pods["items"][3])
    assert w0.name == "w0" and w0.labels == {"app": "web", "rev": "1"}
    # the first DoNotSchedule entry; the ScheduleAnyway one before it is skipped
    assert w0.spread == SpreadConstraint(max_skew=1, topology_key=ZONE, match_labels=(("app", "web"),))
    assert w0.spread.matches(w0.labels) and not w0.spread.matches({"app": "db"})
    plain = pod_from_kube(pods["items"][-2])
    assert plain.spread is None and plain.labels["app"] == "web"
    assert pod_from_kube({"metadata": {"name": "x"}}).labels == {} and pod_from_kube({}).spread is None
    # through JSON text, as the apiserver sends it
    assert pod_from_kube(json.loads(json.dumps(pods["items"][3]))) == w0


def test_spread_tables():
    from ksched.host import node_from_kube, pod_from_kube, spread_tables
    nl, pl = kube_json()
    nodes = [node_from_kube(x) for x in nl["items"]]
    pods = [pod_from_kube(x) for x in pl["items"]]
    bound, pending = [p for p in pods if p.node_name], [p for p in pods if not p.node_name]
    dom, skew, counts, group, enforce = spread_tables(nodes, bound, pending)
    assert dom.tolist() == [0, 0, 1, 1, 2, 0, -1] and dom.dtype == np.int32       # zones a, b, c in node order
    assert skew.tolist() == [1] and skew.dtype == np.int32
    assert counts.tolist() == [[1, 1, 0]] and counts.dtype == np.int32            # b0 in a, b1 in b; b2 is another app
    assert group.tolist() == [0] * 7 + [0, -1] and group.dtype == np.int32        # `plain` counts, `other` does not
    assert enforce.tolist() == [1] * 7 + [0, 0] and enforce.dtype == np.uint8
    # no constraint among the pending pods: one domain, one empty group, nobody in it
    dom, skew, counts, group, enforce = spread_tables(nodes, bound, pending[-2:])
    assert dom.tolist() == [0] * 7 and counts.tolist() == [[0]] and group.tolist() == [-1, -1]
    # two constraints that differ in maxSkew are two groups, each with the bound pods its selector matches
    extra = pod_from_kube(pl["items"][3])
    extra.spread = type(extra.spread)(max_skew=2, topology_key=ZONE, match_labels=extra.spread.match_labels)
    _, skew, counts, group, _ = spread_tables(nodes, bound, pending + [extra])
    assert skew.tolist() == [1, 2] and counts.tolist() == [[1, 1, 0], [1, 1, 0]] and group.tolist()[-1] == 1


def test_second_topology_key_is_an_error():
    from ksched.host import node_from_kube, pod_from_kube, spread_tables
    nl, pl = kube_json()
    nodes = [node_from_kube(x) for x in nl["items"]]
    pending = [pod_from_kube(x) for x in pl["items"][3:6]]
    pending[2].spread = type(pending[2].spread)(max_skew=1, topology_key="kubernetes.io/hostname",
                                                match_labels=pending[2].spread.match_labels)
    with pytest.raises(ValueError, match="one topology key"):
        spread_tables(nodes, [], pending)
    with pytest.raises(ValueError, match="no node carries"):
        spread_tables([node_from_kube({"metadata": {"name": "bare"}, "status": {"capacity": {}}})], [], pending[2:])
