"""ksched_rank_full / ksched_explain_full without a GPU: the CPU restatement (dryrun_ref) against include/ksched.h's
worked example, against rank_ref with every constraint off and against full_ref.schedule_full pod by pod; what each GPU
case of test_gpu_dryrun.py is there for, asserted on the restatement alone; the exports and prototypes; FakeCluster's two
methods on a stub engine; and the stand-alone check program of the calls' host side."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import dryrun_ref as DR
import full_ref as FR
import rank_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZONE, HOST, GPU = "topology.kubernetes.io/zone", "kubernetes.io/hostname", "amd.com/gpu"


def main_case(priority=0, domain=0, labels=True):
    """The GPU tests' main case, full_ref.adversarial(700, 64) in every instantiation family: R = 4 columns, a 2 x 3
    spread table and 12 affinity groups over 3 zones of another key, against its initial tables."""
    return FR.adversarial(700, 64, priority=priority, domain=domain, labels=labels)


def off_case(cl):
    """cl with every constraint off."""
    return FR.Case(cl)


# ---- the exports and the prototypes ------------------------------------------------------------------------------------
def test_library_exports_the_dry_runs():
    from test_abi import header_symbols
    from ksched import _lib as L
    lb = L.lib()
    names = [s[0] for s in L.SIGNATURES]
    for fn in ("ksched_rank_full", "ksched_explain_full"):
        assert fn in header_symbols() and hasattr(lb, fn) and fn in names
    assert lb.ksched_abi_version() == 6
    assert lb.ksched_rank_full(None, 0, *([None] * 12), 1, *([None] * 6)) == L.E_INVALID
    assert lb.ksched_explain_full(None, 0, 0, 0, 0, -1, 1, None, 0, 0, 0, -1, 0, None, None) == L.E_INVALID
    header = open(L.HEADER_PATH).read()
    for name, value in (("REASON_EXT0", 5), ("REASON_SPREAD_NO_KEY", 9), ("REASON_SPREAD_SKEW", 10), ("REASON_AFFINITY", 11),
                        ("REASON_ANTI_AFFINITY", 12), ("REASON_EXISTING_ANTI_AFFINITY", 13), ("NUM_REASONS_FULL", 14)):
        assert getattr(L, name) == value and f"#define KSCHED_{name} " in header
        assert int(header.split(f"#define KSCHED_{name} ")[1].split()[0]) == value
    assert L.NUM_REASONS == 5 and L.REASON_EXT0 + L.EXT_MAX == L.REASON_SPREAD_NO_KEY
    assert sorted(L.REASON_TEXT_FULL) == list(range(1, 14))
    assert all(L.REASON_TEXT_FULL[r] == L.REASON_TEXT[r] for r in L.REASON_TEXT)
    assert L.reason_text_full(6, ["a", GPU]) == "Insufficient " + GPU
    assert L.REASON_TEXT_FULL[9] == "node(s) didn't match pod topology spread constraints (missing required label)"
    assert L.REASON_TEXT_FULL[10] == "node(s) didn't match pod topology spread constraints"
    assert L.REASON_TEXT_FULL[11] == "node(s) didn't match pod affinity rules"
    assert L.REASON_TEXT_FULL[12] == "node(s) didn't match pod anti-affinity rules"
    assert L.REASON_TEXT_FULL[13] == "node(s) didn't satisfy existing pods anti-affinity rules"


# ---- the header's worked example, column for column --------------------------------------------------------------------
def test_worked_example_reference(oracle_mod):
    c, t = DR.worked_example()
    # its start is the end state of ksched_schedule_full's own example
    end = FR.schedule_full(oracle_mod, FR.worked_example())
    assert [np.asarray(x).tolist() for x in DR.after(end).state] == [np.asarray(x).tolist() for x in t.state]
    assert end[5].tolist() == t.counts.tolist() and end[4].tolist() == t.ext.tolist()
    assert [x.tolist() for x in end[8:11]] == [x.tolist() for x in t.words]
    (idx, score, reason, count, feas, hist), per_node, waived = DR.rank_full(oracle_mod, c, 4, t)
    assert per_node.tolist() == [[5, 5, 11, 5], [12, 12, 11, 11], [13, 13, 0, 0], [10, 10, 0, 0]]
    assert idx.tolist() == [[-1] * 4, [-1] * 4, [2, 3, -1, -1], [2, 3, -1, -1]]
    p3, p4 = float(np.float32(0.3)), float(np.float32(0.4))
    assert score.view(np.float64).tolist() == [[0.0] * 4, [0.0] * 4, [p3, p4, 0.0, 0.0], [p3, p4, 0.0, 0.0]]
    assert not reason.any() and count.tolist() == [0, 0, 2, 2] and feas.tolist() == [0, 0, 2, 2] and not waived.any()
    assert hist[0].tolist() == [0] * 5 + [3] + [0] * 5 + [1, 0, 0] and hist[3, 10] == 2 and (hist.sum(1) == 4).all()


# ---- every constraint off: ksched_rank's own reference ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["small93", "c5hc"])
def test_all_off_is_the_rank_reference(name, oracle_mod):
    cl = RR.make(name)
    for k in (1, 16, 64):
        got, per_node, _ = DR.rank_full(oracle_mod, off_case(cl), k)
        RR.same((got[0], got[1].view(np.float64)) + got[2:5], RR.want(oracle_mod, cl, k))
        assert (per_node < 5).all() and (got[5].sum(1) == cl.n_nodes).all() and (got[5][:, 0] == got[4]).all()


# ---- entry 0 is what ksched_schedule_full would choose --------------------------------------------------------------------
def follow_scheduler(O, c, k, rank, schedule, pods=None):
    """Pod by pod, each a gang of one: rank(i, tables) -- a rank_full result for pod i -- then schedule(one-pod case,
    tables) -- a full_ref.schedule_full-shaped result, which moves the tables.  The feasible counts agree;
    with an eligible node, entry 0 and its score bits are the scheduler's choice, or the list is empty and the pod gets
    NO_POSITIVE_SCORE; without one the pod gets NO_FIT, and only the all-node domain still ranks nodes (ksched_rank's
    quirk: they carry their codes).  Returns the outcomes."""
    t = DR.initial(c)
    out = []
    for i in (range(c.cl.n_pods) if pods is None else pods):
        idx, score, _, count, feas, _ = rank(i, t)
        one = dataclasses.replace(FR.pods(c, i, i + 1), counts=t.counts, node_ext=t.ext)
        ref = schedule(one, t)
        w = int(ref[0][0])
        assert int(feas[0]) == int(ref[2][0]), (i, int(feas[0]), int(ref[2][0]))
        if feas[0] == 0:  # ksched_rank's rule: no eligible node is NO_FIT -- whatever the all-node domain still ranks
            assert w == -1 and (count[0] == 0 or (c.cl.priority == 0 and c.cl.domain == 0)), (i, w, int(count[0]))
        elif count[0] == 0:
            assert w == -2, (i, w)
        else:
            assert idx[0, 0] == w, (i, idx[0, :count[0]], w)
            assert np.asarray(score)[0, :1].view(np.int64)[0] == ref[1][:1].view(np.int64)[0], i
        out.append(w)
        t = DR.after(ref)
    return out


@pytest.mark.parametrize("priority, domain", [(0, 0), (0, 1), (1, 1)])
def test_entry_0_is_schedule_full_of_that_pod(priority, domain, oracle_mod):
    O = oracle_mod
    c = FR.adversarial(211, 96, priority=priority, domain=domain, labels=True)
    moved = {}

    def rank(i, t):
        got, per_node, _ = DR.rank_full(O, c, 4, t, pods=[i])
        for code in np.unique(per_node):
            moved[int(code)] = moved.get(int(code), 0) + 1
        return (got[0], got[1].view(np.float64)) + got[2:]
    out = follow_scheduler(O, c, 4, rank, lambda one, t: FR.schedule_full(O, one, state=t.state, table=t.words))
    assert sum(w >= 0 for w in out) >= 20 and sum(w == -1 for w in out) >= 3, out
    assert moved.get(DR.SPREAD_SKEW, 0) >= 1, moved  # (absent against the initial, all-equal counts)


# ---- what the GPU cases are there for -----------------------------------------------------------------------------------
def test_main_case_meets_its_conditions(oracle_mod):
    # against the initial tables, all-node domain: every code, a waiver, ineligible nodes ranked with their full code
    got, per_node, waived = DR.rank_full(oracle_mod, main_case(0, 0), 64)
    assert sorted(np.unique(per_node).tolist()) == list(range(14))
    assert waived.sum() >= 1 and (got[4] == 0).sum() >= 5 and not (got[4] == 700).any()
    assert (got[2] >= 5).sum() >= 100 and (got[3] == 64).all()  # (every node with a positive score is ranked)
    # the lists' lengths differ where only eligible nodes are ranked: the same case in the feasible domain
    for priority in (0, 1):
        cnt = DR.rank_full(oracle_mod, main_case(priority, 1), 64)[0][3]
        assert (cnt == 64).any() and ((cnt > 0) & (cnt < 64)).any() and (cnt == 0).any(), cnt
    # after ksched_schedule_full has run the case: moved counts, columns and words, still every code
    c = main_case(0, 0)
    end = FR.schedule_full(oracle_mod, c)
    t = DR.after(end)
    assert (t.counts != c.counts).any() and (t.ext != c.node_ext).any() and (t.words[0] != c.node_member).any()
    assert sorted(np.unique(DR.rank_full(oracle_mod, c, 5, t)[1]).tolist()) == list(range(14))


def test_one_constraint_cases_meet_their_conditions(oracle_mod):
    import affinity_ref as AR
    import spread_ref as SR
    sp = SR.adversarial(7, 300, 64, 64, 64, 0, 1, False)  # S x D = 64 x 64, the cap
    c = FR.Case(sp[0], None, None, *sp[1:])
    per_node = DR.rank_full(oracle_mod, c, 5)[1]
    assert c.counts.shape == (64, 64) and (per_node == DR.SPREAD_SKEW).any() and (per_node == DR.SPREAD_NO_KEY).any()
    for D in (1024, 0):  # every zone id the table admits; no zone key at all
        a = AR.adversarial(7, 2100, 64, D, 12, 0, 1, False)
        c = FR.Case(a.cl, aff_D=D, aff_domain=a.node_domain, node_member=a.node_member, node_anti_host=a.node_anti_host,
                    node_anti_zone=a.node_anti_zone, member=a.member, anti_host=a.anti_host, anti_zone=a.anti_zone,
                    aff_group=a.aff_group, aff_zone=a.aff_zone)
        per_node = DR.rank_full(oracle_mod, c, 5)[1]
        assert {11, 12, 13} <= set(np.unique(per_node).tolist()), (D, np.unique(per_node))
        assert (a.node_domain is None or int(np.max(a.node_domain)) == D - 1)


# ---- FakeCluster on a stub engine ---------------------------------------------------------------------------------------------
def kube_objects():
    """The worked example's start as Node / Pod objects, and the four pods.  Bound: b0 on n0 and b1 on n1 (app=train,
    job=x, a gpu each, refusing a host that holds app=train), b2 on n2 (job=x only).  The spread selector is job=x
    (counts A 2, B 1), the affinity group app=train (node_member = node_anti_host = {1, 1, 0, 0})."""
    from ksched.host import SCHEDULER_ANNOTATION, AffinityTerm, Container, Node, Pod, SpreadConstraint
    train, job = (("app", "train"),), (("job", "x"),)
    nodes = [Node(name, {"cpu": "64", "memory": "16777216Ki", "pods": "110", GPU: str(g)}, price=pr,
                  label_map={ZONE: z, HOST: name})
             for name, z, pr, g in (("n0", "A", "0.10", 1), ("n1", "A", "0.20", 1), ("n2", "B", "0.30", 1), ("n3", "B", "0.40", 0))]
    anti = (AffinityTerm(HOST, train),)

    def pod(name, gpu=0, labels=None, node="", spread=False, affinity=(), anti_affinity=()):
        req = {"cpu": "100m", **({GPU: str(gpu)} if gpu else {})}
        return Pod(name, [Container("c", req)], node_name=node, annotations={SCHEDULER_ANNOTATION: "hightower"},
                   labels=dict(labels or {}), spread=SpreadConstraint(1, ZONE, job) if spread else None,
                   affinity=affinity, anti_affinity=anti_affinity)
    worker = {"app": "train", "job": "x"}
    bound = [pod("b0", 1, worker, "n0", anti_affinity=anti), pod("b1", 1, worker, "n1", anti_affinity=anti),
             pod("b2", 0, {"job": "x"}, "n2")]
    zone_aff = (AffinityTerm(ZONE, train),)
    four = dict(X=pod("X", 1, {"app": "train"}, spread=True, affinity=zone_aff, anti_affinity=anti),
                Y=pod("Y", 0, {"app": "train"}, affinity=zone_aff, anti_affinity=anti),
                Z=pod("Z", 0, {"app": "train"}), W=pod("W", 0, spread=True))
    return nodes, bound, four


WORKED_MESSAGES = dict(
    X=["fit failure on node (n0): Insufficient amd.com/gpu", "fit failure on node (n1): Insufficient amd.com/gpu",
       "fit failure on node (n2): node(s) didn't match pod affinity rules", "fit failure on node (n3): Insufficient amd.com/gpu"],
    Y=["fit failure on node (n0): node(s) didn't match pod anti-affinity rules",
       "fit failure on node (n1): node(s) didn't match pod anti-affinity rules",
       "fit failure on node (n2): node(s) didn't match pod affinity rules",
       "fit failure on node (n3): node(s) didn't match pod affinity rules"],
    Z=["fit failure on node (n0): node(s) didn't satisfy existing pods anti-affinity rules",
       "fit failure on node (n1): node(s) didn't satisfy existing pods anti-affinity rules"],
    W=["fit failure on node (n0): node(s) didn't match pod topology spread constraints",
       "fit failure on node (n1): node(s) didn't match pod topology spread constraints"])
WORKED_LISTS = dict(X=[], Y=[], Z=[("n2", 0.3), ("n3", 0.4)], W=[("n2", 0.3), ("n3", 0.4)])


def check_fake_cluster(fc, four):
    """rank_pod_full and explain_pod_full of the four pods on a FakeCluster holding kube_objects()' nodes and bound pods."""
    for name, pod in four.items():
        ranked = fc.rank_pod_full(pod, k=4)
        assert [(nd.name, float(np.float32(s)), why) for nd, s, why in ranked] == \
            [(nm, float(np.float32(s)), None) for nm, s in WORKED_LISTS[name]], (name, ranked)
        counts, message = fc.explain_pod_full(pod)
        assert message == f"pod ({name}) failed to fit in any node\n" + "\n".join(WORKED_MESSAGES[name]), (name, message)
        assert counts.sum() == 4 and counts[0] == len(WORKED_LISTS[name])
    assert all(not p.node_name for p in four.values()) and not fc.events


class StubEngine:
    """Stands in for ksched.engine.Engine: records the calls and answers the dry runs from the restatement."""

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

    def _case(self, rc, rm, rp, group, enforce, req_ext, words):
        cl = dataclasses.replace(self.cl, req_cpu=rc, req_mem=rm, req_pods=rp)
        return FR.Case(cl, None, None, *self.spread, group, enforce, self.node_ext, req_ext, *self.aff, *words)

    def rank_full(self, rc, rm, rp, sel, k, group, enforce, req_ext, *words):
        self.calls.append("rank_full")
        got = DR.rank_full(self.O, self._case(rc, rm, rp, group, enforce, req_ext, words), k)[0]
        return (got[0], got[1].view(np.float64)) + got[2:]

    def explain_full(self, rc, rm, rp, sel, group, enforce, req_ext, member, anti_host, anti_zone, aff_group, aff_zone):
        self.calls.append("explain_full")
        one = lambda v, t: np.array([v], t)
        c = self._case(one(rc, np.int64), one(rm, np.int64), one(rp, np.int64), one(group, np.int32), one(enforce, np.uint8),
                       np.asarray(req_ext, np.int64)[:, None], (one(member, np.uint64), one(anti_host, np.uint64),
                                                               one(anti_zone, np.uint64), one(aff_group, np.int32),
                                                               one(aff_zone, np.uint8)))
        got, per_node, _ = DR.rank_full(self.O, c, 1)
        return got[5][0], per_node[0]


def test_fake_cluster_dry_runs_on_a_stub_engine(oracle_mod):
    from ksched import _lib as L
    from ksched.host import FakeCluster, pack_nodes, parse_price
    nodes, bound, four = kube_objects()
    fc = FakeCluster.__new__(FakeCluster)  # (no device: the engine is the stub)
    fc.nodes, fc.pods = nodes, list(bound)
    fc.events, fc.use_labels, fc.priority, fc.domain = [], False, L.PRIORITY_BEST_PRICE, L.DOMAIN_FEASIBLE
    ac, am, ap = pack_nodes(nodes, bound)
    base = DR.worked_example()[0].cl
    assert ap.tolist() == [109, 109, 109, 110]
    fc.engine = StubEngine(oracle_mod, dataclasses.replace(
        base, alloc_cpu=ac, alloc_mem=am, alloc_pods=ap, price=np.array([parse_price(x.price) for x in nodes], np.float32)))
    check_fake_cluster(fc, four)
    assert fc.engine.calls == ["load_spread", "load_ext", "load_affinity", "rank_full",
                               "load_spread", "load_ext", "load_affinity", "explain_full"] * 4
    # the tables its methods load are the header's
    fc.rank_pod_full(four["X"], k=1)
    assert fc.engine.spread[2].tolist() == [[2, 1]] and fc.engine.node_ext.tolist() == [[0, 0, 1, 0]]
    assert [x.tolist() for x in fc.engine.aff[2:]] == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]]


# ---- the calls' host side on its own ------------------------------------------------------------------------------------------
def test_check_program_builds_and_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler"
    exe = str(tmp_path / "dryrun_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "k8s-scheduler_amd", "csrc"),
                    os.path.join(ROOT, "tests", "diag", "dryrun_check_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "all checks passed" in out
