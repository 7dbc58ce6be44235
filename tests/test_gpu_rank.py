"""ksched_rank on the device: every ranked list against the oracle's (oracle.local_topk, merge_topk for shards), column
for column -- idx, score bits, reason, count, feasible -- and the call's promises: it commits nothing, entry 0 is what
the scheduler picks next, and shard lists merge into the one-context lists."""
import numpy as np
import pytest

import rank_ref as RR

pytestmark = pytest.mark.gpu

_REF = {}


def ref(O, name, k):
    """The oracle's lists of a named cluster, computed once per (cluster, k) and shared (never modified)."""
    if name not in _REF:
        _REF[name] = RR.make(name)
    if (name, k) not in _REF:
        _REF[(name, k)] = RR.want(O, _REF[name], k)
    return _REF[name], _REF[(name, k)]


def longest_run(row):
    """Length of the longest run of equal values in a 1-d array."""
    edges = np.flatnonzero(np.concatenate(([True], row[1:] != row[:-1], [True])))
    return int(np.diff(edges).max())


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def rank(e, cl, k, pods=slice(None)):
    sel = None if cl.selector is None else cl.selector[pods]
    return e.rank(cl.req_cpu[pods], cl.req_mem[pods], cl.req_pods[pods], sel, k=k)


# ---- 1. parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3", "c2", "c5hc", "c5", "small93"])
def test_rank_parity(name, gpu_available, oracle_mod):
    cl, (idx, score, _, count, feas) = ref(oracle_mod, name, 64)
    with engine(cl) as e:
        for k in (1, 5, 16, 64):
            RR.same(rank(e, cl, k), ref(oracle_mod, name, k)[1])
    # the classes of input this cluster is here for do occur (in the oracle's lists, which the device's equal)
    if name == "c3":  # a pod requesting no cpu or memory: its whole top 64 is one tie class, in index order
        assert any(longest_run(score[i]) == 64 and (np.diff(idx[i]) > 0).all() for i in range(cl.n_pods))
    if name == "c2":  # 200 distinct prices over 5000 nodes: runs of equal prices, ordered by node index inside
        assert max(longest_run(score[i]) for i in range(cl.n_pods)) >= 16
        assert (np.diff(idx, axis=1)[np.diff(score, axis=1) == 0] > 0).all()
    if name == "c5":  # the predicate matters: few of the 5000 nodes are feasible for some pods
        assert feas.min() < 100 and (count == 64).any()
    if name == "c5hc":
        assert (count == 64).any() and ((count > 0) & (count < 64)).any()
    if name == "small93":  # the all-node domain ranks nodes that fail the predicate: the reason column says why
        assert (ref(oracle_mod, name, 64)[1][2] != 0).any()


@pytest.mark.parametrize("s", [0, 1, 2, 3])
@pytest.mark.parametrize("p", [0, 1])
def test_rank_parity_random_small(s, p, gpu_available, oracle_mod):
    from ksched import cluster
    cl = cluster.random_small(90 + s, 211, 96, priority=p, domain=s % 2, use_labels=s % 2 == 1)
    # the +-2^62 / 2^53 edge values: this call cannot take the FAST53 instantiation
    assert max(np.abs(cl.alloc_cpu).max(), np.abs(cl.req_cpu).max()) >= 1 << 52
    with engine(cl) as e:
        for k in (1, 5, 16, 64):
            want = RR.want(oracle_mod, cl, k)
            RR.same(rank(e, cl, k), want)
    count = want[3]  # (k = 64) these seeds mix full and partial lists; seed 93 under the feasible domain has empty ones
    if (s, p) == (3, 0):
        assert (count == 0).sum() == 3 and ((count > 0) & (count < 64)).sum() == 93
    elif (s, p) != (2, 0):
        assert (count == 64).any() and ((count > 0) & (count < 64)).any()


# ---- 2. small n ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_rank_small_n(n, gpu_available, oracle_mod):
    import dataclasses
    full = ref(oracle_mod, "c3", 64)[0]
    cl = dataclasses.replace(full, alloc_cpu=full.alloc_cpu[:n], alloc_mem=full.alloc_mem[:n],
                             alloc_pods=full.alloc_pods[:n])
    with engine(cl) as e:
        got = rank(e, cl, 64)
    RR.same(got, RR.want(oracle_mod, cl, 64))
    assert got[3].max() == min(n, 64)


def test_rank_no_nodes(gpu_available):
    from ksched import MODE_EXACT, Engine
    z = np.zeros(0, np.int64)
    with Engine(mode=MODE_EXACT, device=0) as e:
        e.load_nodes(z, z, z)
        idx, score, reason, count, feas = e.rank([100, 0], [1024, 0], [1, 0], k=3)
    assert (idx == -1).all() and not score.any() and not reason.any() and not count.any() and not feas.any()


# ---- 3. span and tile boundaries ---------------------------------------------------------------------------------
def test_rank_many_spans(gpu_available, oracle_mod):
    from ksched import cluster
    # 3 pods are one tile, so the scan takes the shortest spans: ceil(100003 / 1024) = 98 of them (the last one 675
    # rows: its fourth wave has no row at all), folded by the merge kernel's four waves
    cl = cluster.make_cluster("c4", n_nodes=100003, n_pods=3)
    with engine(cl) as e:
        RR.same(rank(e, cl, 64), RR.want(oracle_mod, cl, 64))


def test_rank_pod_tiles(gpu_available, oracle_mod):
    """m = 1, 7, 65, 300: one partial tile, full tiles with a partial last one (c3's 20011 rows are 20 spans for each
    of these m).  A pod's lists do not depend on the pods ranked with it."""
    from ksched import cluster
    cl = cluster.make_cluster("c3", n_nodes=20011, n_pods=300)
    with engine(cl) as e:
        all300 = rank(e, cl, 64)
        RR.same(all300, RR.want(oracle_mod, cl, 64))
        for m in (1, 7, 65):
            part = rank(e, cl, 64, slice(0, m))
            for a, b in zip(part, all300):
                assert np.array_equal(a.view(np.uint8), b[:m].view(np.uint8))


def test_rank_chunks(gpu_available, oracle_mod):
    """More pods than one chunk of 1024: the second pair of launches reuses the workspace, with other spans (300 rows
    are one span) and a one-tile tail."""
    from ksched import cluster
    cl = cluster.make_cluster("c3", n_nodes=300, n_pods=1024 + 5)
    with engine(cl) as e:
        RR.same(rank(e, cl, 5), RR.want(oracle_mod, cl, 5))


# ---- 4. agreement with the scheduler -----------------------------------------------------------------------------
def test_rank_agrees_with_schedule(gpu_available, oracle_mod):
    from ksched import NO_FIT, NO_POSITIVE_SCORE, cluster
    cl = cluster.make_cluster("c5hc", n_nodes=2000, n_pods=40)
    with engine(cl) as e:
        for i in range(cl.n_pods):
            one = slice(i, i + 1)
            before = e.read_nodes()
            idx, score, _, count, feas = rank(e, cl, 4, one)
            assert all(np.array_equal(a, b) for a, b in zip(before, e.read_nodes())), "rank changed a node row"
            oi, os_, of = e.schedule(cl.req_cpu[one], cl.req_mem[one], cl.req_pods[one], cl.selector[one])
            assert feas[0] == of[0]
            if count[0] == 0:
                assert oi[0] == (NO_FIT if feas[0] == 0 else NO_POSITIVE_SCORE) and os_[0] == 0.0
            else:
                assert idx[0, 0] == oi[0] and score[0, :1].view(np.int64)[0] == os_.view(np.int64)[0]
        # the last schedule call's explanations survive a rank
        cnt0, nf0 = e.explain_batch()
        rank(e, cl, 4)
        cnt1, nf1 = e.explain_batch()
        assert nf0 == nf1 and np.array_equal(cnt0, cnt1)


# ---- 5. sharded ------------------------------------------------------------------------------------------------------
def test_rank_sharded_merge(gpu_available, oracle_mod):
    from ksched import MODE_EXACT
    from ksched.dist import make_sharded_engine, merge_ranked
    cl, want = ref(oracle_mod, "c3", 16)
    shards = []
    for r in range(2):  # two contexts of this process, one after the other: nothing is scheduled, so no communicator
        e, (lo, hi) = make_sharded_engine(cl, r, 2, device=0, mode=MODE_EXACT, comm=False)
        with e:
            shards.append(rank(e, cl, 16))
        recs, fc = RR.shard_recs(oracle_mod, cl, 16, lo, hi)
        RR.same(shards[-1], RR.columns(oracle_mod, cl, recs, fc, 16, lo=lo, hi=hi))
    merged = merge_ranked(cl.priority, shards)
    RR.same(merged, want)
    with engine(cl) as e:
        for a, b in zip(rank(e, cl, 16), merged):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 6. the README's demo ------------------------------------------------------------------------------------------
def test_rank_readme_demo(gpu_available):
    from ksched import DOMAIN_FEASIBLE, PRIORITY_BEST_PRICE, cluster
    from ksched.host import Container, FakeCluster, Node, Pod
    cl = cluster.readme_demo()
    nodes = [Node(nm, cap, price=pr) for nm, cap, pr in zip(cl.node_names, cl.node_capacity, cl.node_price_str)]
    pod = Pod("nginx", [Container(requests=r) for r in cl.pending_pods[0]])
    fc = FakeCluster(nodes, [pod], priority=PRIORITY_BEST_PRICE, domain=DOMAIN_FEASIBLE, device=0)
    got = fc.rank_pod(pod, k=6)
    assert [nd.name[-4:] for nd, _, _ in got] == ["pxee", "3vzg", "nmz7", "zynj", "00lq", "xm4i"]
    assert [s for _, s, _ in got] == [float(np.float32(x)) for x in (0.05, 0.40, 0.40, 0.40, 0.80, 1.60)]
    assert all(why is None for _, _, why in got) and not pod.node_name
    assert [nd.name[-4:] for nd, _, _ in fc.rank_pod(pod, k=2)] == ["pxee", "3vzg"]


def test_rank_reason_text_all_node_domain(gpu_available):
    """The all-node domain ranks nodes that fail the predicate: rank_pod names the failing check."""
    from ksched import DOMAIN_ALL, PRIORITY_RESOURCE
    from ksched.host import Container, FakeCluster, Node, Pod
    nodes = [Node("big", dict(cpu="8", memory="1024Ki", pods="10")), Node("small", dict(cpu="1", memory="1024Ki", pods="10"))]
    pod = Pod("p", [Container(requests=dict(cpu="2", memory="1Ki"))])
    fc = FakeCluster(nodes, [pod], priority=PRIORITY_RESOURCE, domain=DOMAIN_ALL, device=0)
    got = fc.rank_pod(pod, k=2)
    assert [(nd.name, why) for nd, _, why in got] == [("big", None), ("small", "Insufficient CPU")]


# ---- 7. errors ---------------------------------------------------------------------------------------------------
def test_rank_errors(gpu_available):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    one = np.ones(1, np.int64)
    with Engine(mode=MODE_EXACT, device=0) as e:
        with pytest.raises(KschedError) as ei:
            e.rank(one, one, one, k=4)
        assert ei.value.code == L.E_STATE and "rank" in str(ei.value)
        e.load_nodes(one * 4000, one * 4096, one * 10)
        for k in (0, 65):
            with pytest.raises(KschedError) as ei:
                e.rank(one, one, one, k=k)
            assert ei.value.code == L.E_INVALID and "rank" in str(ei.value)
        assert e.rank(one, one, one, k=1)[0].tolist() == [[0]]
        assert e.rank(one[:0], one[:0], one[:0], k=1)[0].shape == (0, 1)
