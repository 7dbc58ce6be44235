"""ksched_schedule_full without a GPU: the library's export, the CPU restatement (full_ref) on the worked example of
include/ksched.h and on its equivalences -- affinity off is constrained_ref, affinity alone with gangs of one is
affinity_ref -- the conditions every case of test_gpu_full.py must meet (asserted here from the reference and its
deliberately wrong skip_undo variants, so a bad generator fails here and not on the device), and ksched.host's path from
Kubernetes-shaped objects."""
import dataclasses
import json

import numpy as np
import pytest

import affinity_ref as AR
import constrained_ref as CR
import full_ref as FR

GPU = "amd.com/gpu"
ZONE = "topology.kubernetes.io/zone"
HOST = "kubernetes.io/hostname"

# the generator's seeds per half-required family (priority, domain, labels) where the defaults miss a condition below:
# few members fail there, so few half-required gangs are rejected
HALF_SEEDS = {(0, 0, False): dict(aff_seed=8), (0, 0, True): dict(seed=9), (1, 0, True): dict(aff_seed=8),
              (1, 1, True): dict(aff_seed=8)}

_REF = {}


def family(priority, domain, labels, half):
    kw = dict(priority=priority, domain=domain, labels=labels, half=half)
    if half:
        kw.update(HALF_SEEDS.get((priority, domain, labels), {}))
    return kw


def case(O, n, p, **kw):
    """(case, reference) of a named input, computed once and shared by both test files (never modified)."""
    key = (n, p) + tuple(sorted(kw.items()))
    if key not in _REF:
        c = FR.adversarial(n, p, **kw)
        _REF[key] = (c, FR.schedule_full(O, c))
    return _REF[key]


def diffs(O, c, want):
    return {k: FR.diff(want, FR.schedule_full(O, c, skip_undo={k})) for k in ("node", "zone", "any")}


def conditions(O, c, want, half=False, zone=True, any_=False):
    """The conditions of a rollback case: each kind of missing undo would change at least this many pods' results."""
    info, d = want[7], diffs(O, c, want)
    if half:
        assert d["node"] >= 5 and info["partial"] >= 10 and info["rollbacks"] >= 5, (d, info)
        return
    assert d["node"] >= 10, (d, info)
    assert not zone or d["zone"] >= 10, (d, info)
    assert not any_ or d["any"] >= 10, (d, info)
    assert info["rollbacks"] >= 1 and info["undo_node_word"] >= 1, info


def outside_workgroup_0(c, want, wgs):
    """The workgroup case under exact_wgs = wgs: final winners, and undone slots -- the winners of rolled-back members
    with an affinity word, which the outputs no longer name (the reference keeps them) -- lie outside workgroup 0's
    nodes [0, per_wg), the undone ones in every other workgroup, and some of them in a zone (a zone word is undone by
    thread 0 of every workgroup, whichever owns the slot)."""
    per_wg = -(-c.cl.n_nodes // wgs)
    assert (want[0] >= per_wg).sum() >= 10
    undone = np.asarray(want[7]["rolled_aff_nodes"])
    assert (undone >= per_wg).sum() >= 10, want[7]
    assert {int(w) // per_wg for w in undone} >= set(range(1, -(-c.cl.n_nodes // per_wg)))
    assert (np.asarray(c.aff_domain)[undone[undone >= per_wg]] >= 0).sum() >= 10


# every generated case of test_gpu_full.py: name -> (n, p, generator arguments, arguments of conditions())
def gpu_cases():
    out = {}
    for pr in (0, 1):
        for dm in (0, 1):
            for lb in (False, True):
                for half in (False, True):
                    out[("family", pr, dm, lb, half)] = (64, 256, family(pr, dm, lb, half), dict(half=half, any_=True))
    out["workgroups"] = (64, 256, dict(domain=1), dict(any_=True))
    for n in (1, 63, 65):
        out[("nodes", n)] = (n, 256, dict(D=min(3, n), D_aff=min(3, n), domain=1), {})
    out["two_slots"] = (300, 1024, dict(domain=1), {})
    out["eight_slots"] = (1100, 1024, dict(domain=1, labels=True), {})
    out["zones_1024"] = (1100, 512, dict(D_aff=1024, domain=1), {})
    out["no_zone_key"] = (64, 256, dict(D_aff=0, domain=1), dict(zone=False))
    out["other_key"] = (64, 256, dict(D=4, D_aff=7, domain=1), {})
    out["gang_cap"] = (64, 1100, dict(domain=1, gang_off=(0, 1024, 1100)), dict(any_=True))
    return out


def test_library_exports_the_full_call():
    from test_abi import header_symbols
    from ksched import _lib as L
    lb = L.lib()
    assert "ksched_schedule_full" in header_symbols() and hasattr(lb, "ksched_schedule_full")
    assert "ksched_schedule_full" in [s[0] for s in L.SIGNATURES]
    assert lb.ksched_abi_version() == 6
    assert lb.ksched_schedule_full(None, 0, *([None] * 4), 0, *([None] * 14)) == L.E_INVALID


def test_worked_example_reference(oracle_mod):
    c = FR.worked_example()
    want = FR.schedule_full(oracle_mod, c)
    idx, score, feas, placed, ext, counts, state, info, nm, nah, naz = want
    assert idx.tolist() == [-3, -3, -1, 0, 1, 2] and feas.tolist() == [3, 1, 0, 3, 1, 2] and placed.tolist() == [0, 2, 1]
    assert counts.tolist() == [[2, 1]] and ext.tolist() == [[0, 0, 1, 0]]
    assert nm.tolist() == [1, 1, 0, 0] and nah.tolist() == [1, 1, 0, 0] and naz.tolist() == [0, 0, 0, 0]
    assert score.tolist() == [0.0, 0.0, 0.0, float(np.float32(0.1)), float(np.float32(0.2)), float(np.float32(0.3))]
    assert state[2].tolist() == [109, 109, 109, 110]
    assert info["rollbacks"] == 1 and info["rewaived"] == 1 and info["waived"] == 2, info
    assert min(info[k] for k in ("undo_ext", "undo_spread", "undo_node_word", "undo_zone_word", "undo_any")) == 1, info
    # the header's "why" of p3: with any_zone left set it finds no node; with the node words left set n0 and n1 refuse it
    left_any = FR.schedule_full(oracle_mod, c, skip_undo={"any"})
    assert left_any[0][3] == -1 and left_any[2][3] == 0
    left_node = FR.schedule_full(oracle_mod, c, skip_undo={"node"})
    assert left_node[2][3] == 1 and left_node[0][3] != 0  # (only n2 is left, and its gang then fails with p4)
    d = diffs(oracle_mod, c, want)
    assert d["any"] >= 1 and d["node"] >= 1, d


@pytest.mark.parametrize("half", [False, True])
def test_affinity_off_is_the_constrained_reference(half, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, domain=1, half=half)
    off = dataclasses.replace(c, member=None, anti_host=None, anti_zone=None, aff_group=None, aff_zone=None)
    got, want = FR.schedule_full(oracle_mod, off), CR.schedule_constrained(oracle_mod, FR.without_affinity(c))
    CR.same(got[:4], got[4], got[5], got[6], want)
    assert got[8] is None and want[7]["rollbacks"] >= 5


@pytest.mark.parametrize("D_aff", [3, 0])
def test_affinity_alone_is_the_affinity_reference(D_aff, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, domain=1, D_aff=D_aff)
    only = dataclasses.replace(c, gang_off=None, gang_min=None, group=None, enforce=None, req_ext=None)
    got, want = FR.schedule_full(oracle_mod, only), AR.schedule_affinity(oracle_mod, FR.affinity_only(c))
    AR.same(got[:3], got[8:11], got[6], want)
    assert got[3].shape == (0,) and got[4] is None and got[5] is None and got[7]["rollbacks"] == 0
    assert got[7]["waived"] == want[7]["waived"] >= 1


@pytest.mark.parametrize("name", list(gpu_cases()), ids=str)
def test_gpu_cases_meet_their_conditions(name, oracle_mod):
    n, p, kw, cond = gpu_cases()[name]
    c, want = case(oracle_mod, n, p, **kw)
    conditions(oracle_mod, c, want, **cond)
    if name == "eight_slots":  # winners in several slot rows, and beyond the first 1024 nodes
        assert (want[0] >= 1024).sum() >= 5 and len({int(w) // 256 for w in want[0] if w >= 0}) >= 4
    if name == "workgroups":
        for wgs in (2, 4, 7):
            outside_workgroup_0(c, want, wgs)
    if name == "two_slots":
        assert (want[0] >= 256).sum() >= 10
    if name == "gang_cap":
        rolled = want[0][:1024] == FR.GANG_REJECTED
        assert want[3][0] == 0 and rolled.sum() >= 200 and want[7]["rewaived"] >= 1, want[7]
        assert (rolled & (c.member[:1024] != 0)).sum() >= 100
    if name == "other_key":
        assert not np.array_equal(c.node_domain, c.aff_domain) and c.counts.shape[1] != c.aff_D


def kube_json():
    """The worked example as Kubernetes objects, the gangs interleaved in the pod list: job1 {p0, p1, p2}, job2 {p3, p4},
    p5 alone.  p0-p4 carry app=train (so they count in p5's spread group), refuse a host that holds app=train and want
    a zone that does; p5 carries the spread constraint and no label."""
    from ksched.host import GROUP_NAME_ANNOTATION, PRICE_ANNOTATION, SCHEDULER_ANNOTATION
    train = {"labelSelector": {"matchLabels": {"app": "train"}}}

    def node(name, zone, price, gpus):
        return {"metadata": {"name": name, "labels": {ZONE: zone, HOST: name}, "annotations": {PRICE_ANNOTATION: price}},
                "status": {"capacity": {"cpu": "64", "memory": "16777216Ki", "pods": "110", GPU: str(gpus)}}}

    def pod(name, job=None, worker=True):
        ann = {SCHEDULER_ANNOTATION: "hightower"}
        if job:
            ann[GROUP_NAME_ANNOTATION] = job
        spec = {"nodeName": "", "containers": [{"name": "c", "resources": {"requests": {
            "cpu": "100m", **({GPU: "1"} if worker else {})}}}]}
        if worker:
            spec["affinity"] = {
                "podAntiAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [dict(train, topologyKey=HOST)]},
                "podAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": [dict(train, topologyKey=ZONE)]}}
        else:
            spec["topologySpreadConstraints"] = [dict(train, maxSkew=1, topologyKey=ZONE, whenUnsatisfiable="DoNotSchedule")]
        return {"metadata": {"name": name, "annotations": ann, "labels": {"app": "train"} if worker else {}}, "spec": spec}

    nodes = {"items": [node("n0", "A", "0.10", 1), node("n1", "A", "0.20", 1), node("n2", "B", "0.30", 1),
                       node("n3", "B", "0.40", 0)]}
    pods = {"items": [pod("p0", "job1"), pod("p3", "job2"), pod("p1", "job1"), pod("p4", "job2"), pod("p2", "job1"),
                      pod("p5", worker=False)]}
    return nodes, pods


def test_tables_in_the_documented_order():
    from ksched.host import affinity_tables, ext_tables, group_gangs, node_from_kube, pod_from_kube, spread_tables
    nl, pl = kube_json()
    nodes = [node_from_kube(x) for x in json.loads(json.dumps(nl))["items"]]
    pending = [pod_from_kube(x) for x in json.loads(json.dumps(pl))["items"]]
    pods, off, gmin = group_gangs(pending)  # first: it reorders the pods
    assert [p.name for p in pods] == ["p0", "p1", "p2", "p3", "p4", "p5"]
    c = FR.worked_example()
    dom, skew, counts, group, enforce = spread_tables(nodes, [], pods)
    names, node_ext, req_ext = ext_tables(nodes, [], pods)
    t = affinity_tables(nodes, [], pods)
    assert off.tolist() == c.gang_off.tolist() and gmin.tolist() == [3, 2, 1]
    assert dom.tolist() == c.node_domain.tolist() and skew.tolist() == [1] and counts.tolist() == [[0, 0]]
    assert group.tolist() == c.group.tolist() and enforce.tolist() == c.enforce.tolist()
    assert names == [GPU] and node_ext.tolist() == c.node_ext.tolist() and req_ext.tolist() == c.req_ext.tolist()
    for got, want in zip(t, c.aff_table() + c.aff_pods()):
        assert got.tolist() == want.tolist()


class StubEngine:
    """Stands in for ksched.engine.Engine: records the calls and answers schedule_full from the reference."""

    def __init__(self, O, cl):
        self.O, self.cl, self.calls = O, cl, []

    def load_spread(self, node_domain, max_skew, counts):
        self.calls.append("load_spread")
        self.spread = (node_domain, max_skew, counts)

    def load_ext(self, node_ext):
        self.calls.append("load_ext")
        self.node_ext = node_ext

    def load_affinity(self, node_domain, node_member, node_anti_host, node_anti_zone):
        self.calls.append("load_affinity")
        self.aff = (int(node_domain.max()) + 1, node_domain, node_member, node_anti_host, node_anti_zone)

    def schedule_full(self, rc, rm, rp, sel, off, gmin, group, enforce, req_ext, *words):
        self.calls.append("schedule_full")
        cl = dataclasses.replace(self.cl, req_cpu=rc, req_mem=rm, req_pods=rp)
        c = FR.Case(cl, off, gmin, *self.spread, group, enforce, self.node_ext, req_ext, *self.aff, *words)
        return FR.schedule_full(self.O, c)[:4]


def test_fake_cluster_schedule_full_on_a_stub_engine(oracle_mod):
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, GangRejected, node_from_kube, pod_from_kube
    nl, pl = kube_json()
    fc = FakeCluster.__new__(FakeCluster)  # (no device: the engine is the stub)
    fc.nodes = [node_from_kube(x) for x in nl["items"]]
    fc.pods = [pod_from_kube(x) for x in pl["items"]]
    fc.events, fc.use_labels, fc.priority, fc.domain = [], False, L.PRIORITY_BEST_PRICE, L.DOMAIN_FEASIBLE
    fc.engine = StubEngine(oracle_mod, FR.worked_example().cl)
    res = fc.schedule_full()
    assert fc.engine.calls == ["load_spread", "load_ext", "load_affinity", "schedule_full"]
    assert [p.name for p, _ in res] == ["p0", "p1", "p2", "p3", "p4", "p5"]
    assert [getattr(r, "name", type(r)) for _, r in res] == [GangRejected, GangRejected, FitError, "n0", "n1", "n2"]
    assert [p.node_name for p, _ in res] == ["", "", "", "n0", "n1", "n2"]
    assert [(e["involved"], e["message"]) for e in fc.events if e["reason"] == "FailedScheduling"] == [
        ("p0", "pod (p0) rejected with its gang (job1): 2 of 3 members placed, 3 needed"),
        ("p1", "pod (p1) rejected with its gang (job1): 2 of 3 members placed, 3 needed"),
        ("p2", "pod (p2) failed to fit in any node")]
