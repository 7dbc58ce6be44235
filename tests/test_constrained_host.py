"""ksched_schedule_constrained without a GPU: the library's export, the CPU restatement (constrained_ref) on the worked
example of include/ksched.h's rules and on its four equivalences -- all off is oracle.schedule, one constraint on is
gang_ref / spread_ref / ext_ref -- and ksched.host's path from Kubernetes-shaped objects: group_gangs first, then
spread_tables and ext_tables on the reordered pods, one engine call, the gangs resolved as schedule_gangs does."""
import dataclasses
import json

import numpy as np
import pytest

import constrained_ref as CR
import ext_ref as ER
import gang_ref as GR
import spread_ref as SR

GPU = "amd.com/gpu"
ZONE = "topology.kubernetes.io/zone"


def test_library_exports_the_constrained_call():
    from test_abi import header_symbols
    from ksched import _lib as L
    lb = L.lib()
    assert "ksched_schedule_constrained" in header_symbols() and hasattr(lb, "ksched_schedule_constrained")
    assert lb.ksched_abi_version() == 6
    assert lb.ksched_schedule_constrained(None, 0, None, None, None, None, 0, None, None, None, None, None, None, None,
                                          None, None) == L.E_INVALID


def test_worked_example_reference(oracle_mod):
    c = CR.worked_example()
    idx, score, feas, placed, ext, counts, state, info = CR.schedule_constrained(oracle_mod, c)
    assert idx.tolist() == [0, 2, 0, -3, -1, 1]
    assert feas.tolist() == [3, 1, 2, 1, 0, 1]
    assert placed.tolist() == [3, 0, 1]
    assert counts.tolist() == [[2, 1]] and ext.tolist() == [[0, 0, 0]]
    p01, p02 = float(np.float32(0.1)), float(np.float32(0.2))
    assert score.tolist() == [p01, 0.5, p01, 0.0, 0.0, p02]
    # n2's row is restored: it holds p1 only
    assert state[0].tolist() == [64000 - 200, 64000 - 100, 64000 - 100] and state[2].tolist() == [108, 109, 109]
    assert info == dict(rejected=1, rollbacks=1, partial=0, accepted_after_reject=1, undo_ext=0, undo_spread=1,
                        min_fell=1, narrowed_spread=2, narrowed_ext=3)
    assert oracle_mod.schedule(c.cl)[0].tolist() == [0] * 6


def _same(got, want):
    for a, b in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype == np.float64:
            a, b = a.view(np.int64), b.view(np.int64)
        assert np.array_equal(a, b)


@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("priority,domain", [(0, 0), (0, 1), (1, 1)])
def test_reference_equivalences(priority, domain, labels, oracle_mod):
    c = CR.adversarial(64, 256, priority=priority, domain=domain, labels=labels)
    off = dataclasses.replace(c, gang_off=None, gang_min=None, group=None, enforce=None, req_ext=None)
    # all off: the plain schedule
    got, want = CR.schedule_constrained(oracle_mod, off), oracle_mod.schedule(c.cl)
    _same(got[:3] + got[6], want[:3] + want[3])
    assert got[3].size == 0 and got[4] is None and got[5] is None and (got[0] >= 0).any() and (got[0] < 0).any()
    # gangs alone
    got = CR.schedule_constrained(oracle_mod, dataclasses.replace(off, gang_off=c.gang_off))
    want = GR.schedule_gangs(oracle_mod, c.cl, c.gang_off)
    _same(got[:4] + got[6], want[:4] + want[4])
    assert all(got[7][k] == want[5][k] for k in want[5]) and want[5]["rollbacks"] >= 1  # (the rollback classes: the test below)
    gmin = GR.half_min(c.gang_off)
    got = CR.schedule_constrained(oracle_mod, dataclasses.replace(off, gang_off=c.gang_off, gang_min=gmin))
    want = GR.schedule_gangs(oracle_mod, c.cl, c.gang_off, gmin)
    _same(got[:4] + got[6], want[:4] + want[4])
    # spread alone
    got = CR.schedule_constrained(oracle_mod, dataclasses.replace(off, group=c.group, enforce=c.enforce))
    want = SR.schedule_spread(oracle_mod, c.cl, c.node_domain, c.max_skew, c.counts, c.group, c.enforce)
    _same(got[:3] + (got[5],) + got[6], want[:4] + want[4])
    assert got[7]["narrowed_spread"] == want[5]["narrowed"] >= 10
    # ext alone
    got = CR.schedule_constrained(oracle_mod, dataclasses.replace(off, req_ext=c.req_ext))
    want = ER.schedule_ext(oracle_mod, c.cl, c.node_ext, c.req_ext)
    _same(got[:3] + (got[4],) + got[6], want[:4] + want[4])
    assert got[7]["narrowed_ext"] == want[5]["narrowed"] >= 10


@pytest.mark.parametrize("half", [False, True])
def test_generator_reaches_the_rollback_classes(half, oracle_mod):
    """The classes the device tests assert, on the families' shape (resource priority, feasible domain)."""
    info = CR.schedule_constrained(oracle_mod, CR.adversarial(64, 256, domain=1, half=half))[7]
    if half:
        assert info["rollbacks"] >= 5 and info["partial"] >= 10 and info["undo_spread"] >= 5, info
        assert info["undo_ext"] >= 3 and info["min_fell"] >= 3, info
    else:
        assert min(info["rollbacks"], info["undo_ext"], info["undo_spread"]) >= 10 and info["min_fell"] >= 5, info


def kube_json():
    """The worked example as Kubernetes objects, the gangs interleaved in the pod list: job1 {p0, p1, p2}, job2 {p3, p4},
    p5 alone; p0-p4 carry app=train and the zone constraint, p5 neither."""
    from ksched.host import GROUP_NAME_ANNOTATION, PRICE_ANNOTATION, SCHEDULER_ANNOTATION

    def node(name, zone, price, gpus):
        return {"metadata": {"name": name, "labels": {ZONE: zone}, "annotations": {PRICE_ANNOTATION: price}},
                "status": {"capacity": {"cpu": "64", "memory": "16777216Ki", "pods": "110", GPU: str(gpus)}}}

    def pod(name, gpus, job=None, train=True):
        ann = {SCHEDULER_ANNOTATION: "hightower"}
        if job:
            ann[GROUP_NAME_ANNOTATION] = job
        spec = {"nodeName": "", "containers": [{"name": "c", "resources": {"requests": {
            "cpu": "100m", **({GPU: str(gpus)} if gpus else {})}}}]}
        if train:
            spec["topologySpreadConstraints"] = [{"maxSkew": 1, "topologyKey": ZONE, "whenUnsatisfiable": "DoNotSchedule",
                                                  "labelSelector": {"matchLabels": {"app": "train"}}}]
        return {"metadata": {"name": name, "annotations": ann, "labels": {"app": "train"} if train else {}}, "spec": spec}

    nodes = {"items": [node("n0", "A", "0.10", 2), node("n1", "A", "0.20", 1), node("n2", "B", "0.50", 1)]}
    pods = {"items": [pod("p0", 1, "job1"), pod("p3", 0, "job2"), pod("p1", 1, "job1"), pod("p4", 2, "job2"),
                      pod("p2", 1, "job1"), pod("p5", 1, train=False)]}
    return nodes, pods


def test_tables_in_the_documented_order():
    from ksched.host import ext_tables, group_gangs, node_from_kube, pod_from_kube, spread_tables
    nl, pl = kube_json()
    nodes = [node_from_kube(x) for x in json.loads(json.dumps(nl))["items"]]
    pending = [pod_from_kube(x) for x in json.loads(json.dumps(pl))["items"]]
    pods, off, gmin = group_gangs(pending)  # first: it reorders the pods
    assert [p.name for p in pods] == ["p0", "p1", "p2", "p3", "p4", "p5"]
    dom, skew, counts, group, enforce = spread_tables(nodes, [], pods)
    names, node_ext, req_ext = ext_tables(nodes, [], pods)
    c = CR.worked_example()
    assert off.tolist() == c.gang_off.tolist() and gmin.tolist() == [3, 2, 1]
    assert dom.tolist() == c.node_domain.tolist() and skew.tolist() == [1] and counts.tolist() == [[0, 0]]
    assert group.tolist() == c.group.tolist() and enforce.tolist() == [1, 1, 1, 1, 1, 0]
    assert names == [GPU] and node_ext.tolist() == c.node_ext.tolist() and req_ext.tolist() == c.req_ext.tolist()
    # on the list as it came, the per-pod arrays would belong to other pods
    assert ext_tables(nodes, [], pending)[2].tolist() != req_ext.tolist()


class StubEngine:
    """Stands in for ksched.engine.Engine: records the calls and answers schedule_constrained from the reference."""

    def __init__(self, O, cl):
        self.O, self.cl, self.calls = O, cl, []

    def load_spread(self, node_domain, max_skew, counts):
        self.calls.append("load_spread")
        self.spread = (node_domain, max_skew, counts)

    def load_ext(self, node_ext):
        self.calls.append("load_ext")
        self.node_ext = node_ext

    def schedule_constrained(self, rc, rm, rp, sel, off, gmin, group, enforce, req_ext):
        self.calls.append("schedule_constrained")
        cl = dataclasses.replace(self.cl, req_cpu=rc, req_mem=rm, req_pods=rp)
        c = CR.Case(cl, off, gmin, *self.spread, group, enforce, self.node_ext, req_ext)
        return CR.schedule_constrained(self.O, c)[:4]


def test_fake_cluster_schedule_constrained_on_a_stub_engine(oracle_mod):
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, GangRejected, node_from_kube, pod_from_kube
    nl, pl = kube_json()
    fc = FakeCluster.__new__(FakeCluster)  # (no device: the engine is the stub)
    fc.nodes = [node_from_kube(x) for x in nl["items"]]
    fc.pods = [pod_from_kube(x) for x in pl["items"]]
    fc.events, fc.use_labels, fc.priority, fc.domain = [], False, L.PRIORITY_BEST_PRICE, L.DOMAIN_FEASIBLE
    fc.engine = StubEngine(oracle_mod, CR.worked_example().cl)
    res = fc.schedule_constrained()
    assert fc.engine.calls == ["load_spread", "load_ext", "schedule_constrained"]
    assert [p.name for p, _ in res] == ["p0", "p1", "p2", "p3", "p4", "p5"]
    assert [getattr(r, "name", type(r)) for _, r in res] == ["n0", "n2", "n0", GangRejected, FitError, "n1"]
    assert [p.node_name for p, _ in res] == ["n0", "n2", "n0", "", "", "n1"]
    assert [(e["involved"], e["message"]) for e in fc.events if e["reason"] == "FailedScheduling"] == [
        ("p3", "pod (p3) rejected with its gang (job2): 1 of 2 members placed, 2 needed"),
        ("p4", "pod (p4) failed to fit in any node")]
