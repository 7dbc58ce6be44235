"""ksched_preempt on the device: every output column equal to the plain-Python restatement (preempt_ref), over the
table's block and span edges, the pod tile's edges, the priority and tie cases, and the call's promises: a dry run,
a table that load_nodes invalidates, and victims that do make room on the chosen node."""
import os
import re

import numpy as np
import pytest

import preempt_ref as PR
from conftest import PKG

pytestmark = pytest.mark.gpu

T = 4  # the scan kernel's pod tile, kPreemptTile (test_tile_constant pins it to the header)
CASES = {1: (1, 129, 48), 2: (2, 211, 96), 3: (3, 65, 24)}
_REF = {}


def case(seed):
    """(alloc, bound, pods) of a generator case and its reference answer at vcap = 1024, computed once, never modified."""
    if seed not in _REF:
        cl = PR.gen(*CASES[seed])
        _REF[seed] = (cl, PR.preempt(*cl, 1024))
    return _REF[seed]


def cut(want, vcap):
    """A vcap = 1024 reference answer as a smaller vcap returns it: the victim rows cut, the counts in full."""
    return want[:5] + (np.ascontiguousarray(want[5][:, :vcap]),)


def engine(alloc, bound=None, labels=None):
    from ksched import MODE_EXACT, Engine
    e = Engine(mode=MODE_EXACT, device=0, use_labels=labels is not None)
    e.load_nodes(*alloc, labels=labels)
    if bound is not None:
        e.load_bound(*bound)
    return e


def first_nodes(cl, n):
    """The first n nodes of a cluster with the bound pods they hold."""
    alloc, bound, pods = cl
    keep = bound[0] < n
    return tuple(a[:n] for a in alloc), tuple(b[keep] for b in bound), pods


def test_tile_constant():
    txt = open(os.path.join(PKG, "csrc", "ksched_preempt.h")).read()
    assert int(re.search(r"constexpr int kPreemptTile = (\d+);", txt).group(1)) == T


# ---- 1. parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_preempt_parity(seed, gpu_available):
    (alloc, bound, pods), want = case(seed)
    nofit, novictim, multi = PR.classes(want)
    assert nofit >= 1 and novictim >= 1 and multi >= 1  # every class of answer occurs
    assert want[1].max() > 4  # vcap 1 and 4 do truncate
    with engine(alloc, bound) as e:
        for vcap in (1, 4, 64, 1024):
            got = e.preempt(*pods[:3], None, pods[3], vcap=vcap)
            PR.same(got, cut(want, vcap))
            assert np.array_equal(got[1], want[1])  # the count is the full one at every vcap


def test_preempt_parity_labels(gpu_available):
    (alloc, bound, pods), plain = case(2)
    labels, selector = PR.labels_for(7, len(alloc[0]), len(pods[0]))
    want = PR.preempt(alloc, bound, pods, 64, labels=labels, selector=selector)
    assert all(PR.classes(want)) and not np.array_equal(want[4], plain[4])  # the label check removes candidates
    with engine(alloc, bound, labels=labels) as e:
        PR.same(e.preempt(*pods[:3], selector, pods[3], vcap=64), want)


# ---- 2. small n: block and span edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_preempt_small_n(n, gpu_available):
    alloc, bound, pods = first_nodes(case(2)[0], n)
    with engine(alloc, bound) as e:
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=16), PR.preempt(alloc, bound, pods, 16))


def test_preempt_many_spans(gpu_available):
    """3000 nodes and one tile of pods: three spans of 1024 rows, every wave walks four blocks, the last span is short."""
    alloc, bound, pods = PR.gen(5, 3000, 8, maxseg=12)
    alloc[0][:2500] = 0  # no cpu left on the low nodes: the winners sit in the later spans
    want = PR.preempt(alloc, bound, pods, 16)
    assert (want[0] >= 2048).any() and ((want[0] >= 1024) & (want[0] < 2048)).any() and (want[1] > 1).any()
    with engine(alloc, bound) as e:
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=16), want)


# ---- 3. pod count: the tile's edges, and more than one chunk ----------------------------------------------------------
def test_preempt_pod_tiles(gpu_available):
    (alloc, bound, pods), want = case(2)
    with engine(alloc, bound) as e:
        for m in (1, T - 1, T, T + 1):
            got = e.preempt(*(p[:m] for p in pods[:3]), None, pods[3][:m], vcap=64)
            PR.same(got, tuple(w[:m] for w in cut(want, 64)))


def test_preempt_chunks(gpu_available):
    """1024 + 5 pods: the second pair of launches reuses the workspace for a one-tile tail."""
    alloc, bound, pods = PR.gen(4, 20, 1024 + 5, maxseg=10)
    with engine(alloc, bound) as e:
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=3), PR.preempt(alloc, bound, pods, 3))


# ---- 4. segments -----------------------------------------------------------------------------------------------------
def test_preempt_empty_table(gpu_available):
    """nb = 0: a pod goes where it fits now (the lowest such node), else nowhere."""
    (alloc, _, pods), _ = case(1)
    z = np.zeros(0, np.int64)
    with engine(alloc, (z.astype(np.int32), z, z, z.astype(np.int32))) as e:
        node, nv, mx, sm, cand, vic = e.preempt(*pods[:3], None, pods[3], vcap=4)
    fit = (alloc[0][None, :] >= pods[0][:, None]) & (alloc[1][None, :] >= pods[1][:, None]) & (alloc[2][None, :] >= pods[2][:, None])
    assert fit.any(axis=1).any() and not fit.any(axis=1).all()
    assert np.array_equal(node, np.where(fit.any(axis=1), fit.argmax(axis=1), PR.NO_FIT))
    assert np.array_equal(cand, fit.sum(axis=1)) and not nv.any() and not sm.any()
    assert (mx == PR.NO_VICTIM_PRIO).all() and (vic == -1).all()


def test_preempt_full_segment(gpu_available):
    """One node with exactly KSCHED_BOUND_MAX_PER_NODE pods among empty neighbours; one more is refused."""
    from ksched import KschedError
    from ksched import _lib as L
    r = np.random.default_rng(11)
    n = 67
    alloc = (np.zeros(n, np.int64), np.full(n, 1 << 20), np.full(n, 4))
    nb = L.BOUND_MAX_PER_NODE
    bound = (np.full(nb, 65, np.int32), np.ones(nb, np.int64), np.zeros(nb, np.int64), r.integers(-2, 6, nb).astype(np.int32) * 100)
    pods = (np.array([700, 1, 2000]), np.zeros(3, np.int64), np.ones(3, np.int64), np.array([1000, 1000, 1000], np.int32))
    want = PR.preempt(alloc, bound, pods, 1024)
    assert want[0].tolist() == [65, 65, PR.NO_FIT] and want[1].tolist() == [700, 1, 0]
    with engine(alloc, bound) as e:
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=1024), want)
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=4), cut(want, 4))
        more = tuple(np.concatenate([b, b[:1]]) for b in bound)
        with pytest.raises(KschedError) as ei:
            e.load_bound(*more)
        assert ei.value.code == L.E_INVALID and "load_bound" in str(ei.value)


def test_preempt_block_of_every_length(gpu_available):
    """A block whose 64 nodes hold 0, 1, ..., 63 pods, and a short second block."""
    r = np.random.default_rng(12)
    n = 70
    seg = np.concatenate([np.arange(64), [5, 0, 1, 0, 2, 3]])
    node = np.repeat(np.arange(n), seg)
    node = node[r.permutation(node.size)].astype(np.int32)
    nb = node.size
    bound = (node, r.integers(1, 40, nb) * 50, r.integers(0, 64, nb) * 1024, r.integers(-2, 6, nb).astype(np.int32) * 100)
    alloc = (r.integers(0, 2000, n), r.integers(0, 1 << 20, n), r.integers(0, 4, n))
    pods = (r.integers(1, 400, 24) * 50, r.integers(0, 1 << 20, 24), r.integers(1, 4, 24), r.integers(-3, 8, 24).astype(np.int32) * 100)
    want = PR.preempt(alloc, bound, pods, 64)
    assert all(PR.classes(want))
    with engine(alloc, bound) as e:
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=64), want)


# ---- 5. priorities ---------------------------------------------------------------------------------------------------
def test_preempt_priority_edges(gpu_available):
    (alloc, bound, pods), _ = case(1)
    m = len(pods[0])
    with engine(alloc, bound) as e:
        # below (or at) every bound pod: nobody may go, so a candidate is a node that fits now
        low = np.full(m, bound[3].min(), np.int32)
        got = e.preempt(*pods[:3], None, low, vcap=8)
        PR.same(got, PR.preempt(alloc, bound, pods[:3] + (low,), 8))
        assert not got[1].any() and (got[0] >= 0).any() and (got[2] == PR.NO_VICTIM_PRIO).all()
        # above every bound pod: every pod of a node is a potential victim
        high = np.full(m, bound[3].max() + 1, np.int32)
        got = e.preempt(*pods[:3], None, high, vcap=8)
        PR.same(got, PR.preempt(alloc, bound, pods[:3] + (high,), 8))
        assert (got[1] > 1).any()
    # every bound pod at one priority: the importance order is the table's order alone
    flat = bound[:3] + (np.full(len(bound[0]), 100, np.int32),)
    want = PR.preempt(alloc, flat, pods, 16)
    assert (want[1] > 1).any()
    with engine(alloc, flat) as e:
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=16), want)


# ---- 6. ties across nodes ------------------------------------------------------------------------------------------
def test_preempt_ties_take_the_lowest_node(gpu_available):
    n = 130
    alloc = (np.zeros(n, np.int64), np.full(n, 1 << 20), np.full(n, 4))
    node = np.tile(np.arange(n, dtype=np.int32), 2)  # table pods t and t + n sit on node t
    bound = (node, np.full(2 * n, 600), np.zeros(2 * n, np.int64), np.repeat(np.array([100, 50], np.int32), n))
    pods = (np.array([1000]), np.array([0]), np.array([1]), np.array([1000], np.int32))
    with engine(alloc, bound) as e:
        got = e.preempt(*pods[:3], None, pods[3], vcap=4)
        PR.same(got, PR.preempt(alloc, bound, pods, 4))
        assert got[0].tolist() == [0] and got[4].tolist() == [n] and got[5].tolist() == [[0, n, -1, -1]]
        bound[3][0] = 150  # node 0's key rises: the tie is now among nodes 1 .. 129
        e.load_bound(*bound)
        got = e.preempt(*pods[:3], None, pods[3], vcap=4)
        PR.same(got, PR.preempt(alloc, bound, pods, 4))
        assert got[0].tolist() == [1] and got[5].tolist() == [[1, n + 1, -1, -1]]


# ---- 7. a dry run ------------------------------------------------------------------------------------------------------
def test_preempt_commits_nothing(gpu_available):
    (alloc, bound, pods), want = case(1)
    with engine(alloc, bound) as e, engine(alloc) as plain:
        before = e.read_nodes()
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=1024), want)
        assert all(np.array_equal(a, b) for a, b in zip(before, e.read_nodes())), "preempt changed a node row"
        a = e.schedule(*pods[:3])
        b = plain.schedule(*pods[:3])
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        # the last schedule call's explanations survive a preempt (and a load_bound)
        cnt0, nf0 = e.explain_batch()
        e.load_bound(*bound)
        e.preempt(*pods[:3], None, pods[3], vcap=2)
        cnt1, nf1 = e.explain_batch()
        assert nf0 == nf1 and np.array_equal(cnt0, cnt1)
        assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), plain.read_nodes()))


# ---- 8. state and errors ---------------------------------------------------------------------------------------------
def test_preempt_state_and_errors(gpu_available):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    (alloc, bound, pods), _ = case(3)
    one = (pods[0][:1], pods[1][:1], pods[2][:1], None, pods[3][:1])

    def code(fn):
        with pytest.raises(KschedError) as ei:
            fn()
        return ei.value.code

    with Engine(mode=MODE_EXACT, device=0) as e:
        assert code(lambda: e.load_bound(*bound)) == L.E_STATE  # before load_nodes
        e.load_nodes(*alloc)
        assert code(lambda: e.preempt(*one, vcap=4)) == L.E_STATE  # before load_bound
        e.load_bound(*bound)
        assert e.preempt(*one, vcap=4)[0].shape == (1,)
        for vcap in (0, 1025):
            assert code(lambda: e.preempt(*one, vcap=vcap)) == L.E_INVALID
        for bad in (-1, len(alloc[0])):
            nodes = bound[0].copy()
            nodes[3] = bad
            assert code(lambda: e.load_bound(nodes, *bound[1:])) == L.E_INVALID
        assert e.preempt(*one, vcap=4)[0].shape == (1,)  # a refused table leaves the loaded one in place
        assert e.preempt(*(p[:0] for p in pods[:3]), None, pods[3][:0], vcap=4)[5].shape == (0, 4)
        e.load_nodes(*alloc)  # a second load_nodes invalidates the table
        assert code(lambda: e.preempt(*one, vcap=4)) == L.E_STATE
        e.load_bound(*bound)
        assert e.preempt(*one, vcap=4)[0].shape == (1,)


# ---- 9. closing the loop -----------------------------------------------------------------------------------------------
def test_preempt_victims_make_room(gpu_available):
    """With the victims gone the pod fits on the chosen node; with the last of them left in place it does not."""
    from ksched import _lib as L
    (alloc, bound, pods), want = case(1)
    node, nv, _, _, _, vic = want
    with engine(alloc, bound) as e:
        PR.same(e.preempt(*pods[:3], None, pods[3], vcap=1024), want)
        checked = 0
        for i in np.flatnonzero(nv > 0):
            j, vs = int(node[i]), vic[i, :nv[i]]
            req = (int(pods[0][i]), int(pods[1][i]), int(pods[2][i]))
            assert e.explain(*req)[1][j] != L.REASON_FIT
            rest, last = vs[:-1], vs[-1:]
            e.apply_delta([j], [bound[1][rest].sum()], [bound[2][rest].sum()], [len(rest)])
            assert e.explain(*req)[1][j] != L.REASON_FIT
            e.apply_delta([j], [bound[1][last].sum()], [bound[2][last].sum()], [1])
            assert e.explain(*req)[1][j] == L.REASON_FIT
            e.apply_delta([j], [-bound[1][vs].sum()], [-bound[2][vs].sum()], [-len(vs)])
            checked += 1
        assert checked >= 31
        assert all(np.array_equal(a, b) for a, b in zip(alloc, e.read_nodes()))


# ---- 10. FakeCluster ---------------------------------------------------------------------------------------------------
def test_fake_cluster_preempt_pod(gpu_available):
    """tests/test_preempt_host.py's hand example as kube JSON: pod A preempts bound-1 on node-0, pod B has no node."""
    import kube_json
    from ksched import DOMAIN_FEASIBLE, MODE_EXACT, cluster
    from ksched.host import FakeCluster, FitError
    z = np.zeros(0, np.int64)
    cl = cluster.Cluster(name="hand", alloc_cpu=z, alloc_mem=z, alloc_pods=z, req_cpu=z, req_mem=z, req_pods=z)
    cl.node_names = ["node-0", "node-1", "node-2"]
    cl.node_capacity = [dict(cpu=c, memory="1048576Ki", pods="12") for c in ("1500m", "1000m", "1500m")]
    cl.bound_pods = [(f"node-{j}", [dict(cpu=c)]) for j, c in ((2, "500m"), (0, "600m"), (1, "500m"), (0, "500m"), (1, "500m"), (2, "600m"))]
    cl.pending_pods = [[dict(cpu="1000m")], [dict(cpu="1000m")]]
    nl, pl = kube_json.to_kube(cl)
    for item, prio in zip(pl["items"], (100, 200, 200, 100, 50, 200, 1000, 150)):
        item["spec"]["priority"] = prio
    fc = FakeCluster.from_kube_json(nl, pl, domain=DOMAIN_FEASIBLE, mode=MODE_EXACT, device=0)
    a, b = fc.unscheduled_pods()
    assert (a.priority, b.priority) == (1000, 150)
    node, victims = fc.preempt_pod(a)
    assert node.name == "node-0" and [v.name for v in victims] == ["bound-1"]
    assert len(fc.pods) == 8 and not fc.events and not a.node_name  # a dry run
    with pytest.raises(FitError):
        fc.preempt_pod(b)
    with pytest.raises(FitError):
        fc.schedule_pod(a)  # it fits nowhere yet
    node, victims = fc.preempt_pod(a, evict=True)
    assert node.name == "node-0" and [v.name for v in victims] == ["bound-1"]
    assert "bound-1" not in [p.name for p in fc.pods] and not a.node_name
    assert [(ev["reason"], ev["involved"]) for ev in fc.events if ev["reason"] == "Preempted"] == [("Preempted", "bound-1")]
    assert fc.schedule_pod(a).name == "node-0"  # the victim's resources are back on the node
