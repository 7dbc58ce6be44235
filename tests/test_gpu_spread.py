"""ksched_schedule_spread on the device against the CPU restatement (spread_ref: the oracle, pod by pod, under the numpy
eligibility mask): idx, score bits, feasible, the final counts and the final node rows, all exactly.  The classes of
pods each case is here for -- narrowed, moved, spread_nofit, min_rose, count_only, off_domain -- are asserted from the
reference's output before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import spread_ref as SR

pytestmark = pytest.mark.gpu

_REF = {}


def case(O, kind, n, p, D, S, priority=0, domain=0, labels=False):
    """(inputs, reference) of a named input, computed once and shared (never modified)."""
    key = (kind, n, p, D, S, priority, domain, labels)
    if key not in _REF:
        a = SR.adversarial(7, n, p, D, S, priority, domain, labels) if kind == "adv" else SR.healthy(7, n, p, D, S)
        _REF[key] = (a, SR.schedule_spread(O, *a))
    return _REF[key]


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def run(e, a, lo=0, hi=None):
    cl, _, _, _, group, enforce = a
    sel = None if cl.selector is None else cl.selector[lo:hi]
    return e.schedule_spread(cl.req_cpu[lo:hi], cl.req_mem[lo:hi], cl.req_pods[lo:hi], sel, group[lo:hi], enforce[lo:hi])


def check(a, want, **kw):
    cl, dom, skew, counts = a[:4]
    with engine(cl, **kw) as e:
        e.load_spread(dom, skew, counts)
        got = run(e, a)
        st = e.stats()
        SR.same(got, e.read_spread(), e.read_nodes(), want)
    assert st["pipeline"] == "exact" and st["pods"] == cl.n_pods and st["placed"] == int((want[0] >= 0).sum())
    assert st["pair_evals"] == cl.n_pods * cl.n_nodes


# ---- 1. families: every instantiation family ------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_spread_families(priority, domain, labels, gpu_available, oracle_mod):
    a, want = case(oracle_mod, "adv", 64, 256, 4, 3, priority, domain, labels)
    info = want[5]
    assert info["narrowed"] >= 50 and info["spread_nofit"] >= 10 and info["min_rose"] >= 10, info
    assert info["count_only"] >= 20 and info["off_domain"] >= 1, info
    if priority == 1 or domain == 1:
        assert info["moved"] >= 40, info
    check(a, want)


# ---- 2. increments come from winners that other workgroups own, with uneven per_wg -----------------------------------------
@pytest.mark.parametrize("wgs", [1, 2, 4, 7])
def test_spread_workgroups(wgs, gpu_available, oracle_mod):
    a, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    per_wg = -(-a[0].n_nodes // wgs)
    grouped = (want[0] >= 0) & (a[4] >= 0)
    assert want[5]["min_rose"] >= 10 and grouped.sum() >= 50
    if wgs > 1:  # counted placements beyond workgroup 0's nodes
        assert (want[0][grouped] >= per_wg).sum() >= 10
    check(a, want, exact_wgs=wgs)


# ---- 3. one node, and node counts around the wave size ---------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(1, 1), (63, 8), (65, 8)])
def test_spread_node_counts(n, D, gpu_available, oracle_mod):
    a, want = case(oracle_mod, "adv", n, 256, D, 3)
    info = want[5]
    if n == 1:  # one domain: the constraint never binds
        assert info["narrowed"] == 0 and info["spread_nofit"] == 0 and (want[0] >= 0).any(), info
    if n == 65:
        assert info["off_domain"] >= 3 and info["spread_nofit"] >= 44, info
    check(a, want)


# ---- 4. two node slots per thread --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", [0, 1])
def test_spread_two_slots(domain, gpu_available, oracle_mod):
    a, want = case(oracle_mod, "adv", 300, 2048, 16, 4, 0, domain)
    info = want[5]
    assert info["spread_nofit"] >= 250 and info["min_rose"] >= 9 and info["count_only"] >= 300, info
    check(a, want, exact_wgs=1)


# ---- 5. the table at its caps, healthy cluster ---------------------------------------------------------------------------------
def test_spread_caps_domains(gpu_available, oracle_mod):
    a, want = case(oracle_mod, "healthy", 1100, 2600, 1024, 4)
    assert want[5]["moved"] >= 1000 and want[5]["min_rose"] >= 2 and want[3][0].min() == 2, want[5]
    check(a, want)


def test_spread_caps_groups(gpu_available, oracle_mod):
    a, want = case(oracle_mod, "healthy", 520, 1500, 256, 16)
    assert want[5]["min_rose"] >= 5, want[5]
    check(a, want)


def test_spread_hostname(gpu_available, oracle_mod):
    a, want = case(oracle_mod, "healthy", 64, 600, 64, 1)
    assert want[5]["min_rose"] >= 8 and a[1].tolist() == list(range(64)), want[5]
    check(a, want)


# ---- 6. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("priority", [0, 1])
def test_spread_no_groups_is_schedule(priority, gpu_available, oracle_mod):
    a, _ = case(oracle_mod, "adv", 64, 256, 4, 3, priority, 1)
    cl, dom, skew, counts = a[:4]
    with engine(cl) as e:
        plain = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        plain_state, plain_st = e.read_nodes(), e.stats()
    with engine(cl) as e:
        e.load_spread(dom, skew, counts)
        got = e.schedule_spread(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, np.full(cl.n_pods, -1), a[5])
        state, st, cnt = e.read_nodes(), e.stats(), e.read_spread()
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1].view(np.int64), plain[1].view(np.int64))
    assert np.array_equal(got[2], plain[2]) and all(np.array_equal(x, y) for x, y in zip(state, plain_state))
    for k in ("pods", "placed", "batches", "truncations", "pair_evals", "pipeline", "rescues", "exact_rows", "scan_rows"):
        assert st[k] == plain_st[k], k
    assert np.array_equal(cnt, counts) and (got[0] >= 0).any() and (got[0] < 0).any()
    assert np.array_equal(got[0], oracle_mod.schedule(cl)[0])


def test_spread_count_only_is_schedule_and_tally(gpu_available, oracle_mod):
    a, _ = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl, dom, skew, counts, group, _ = a
    with engine(cl) as e:
        plain = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
    with engine(cl) as e:
        e.load_spread(dom, skew, counts)
        got = e.schedule_spread(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, group, np.zeros(cl.n_pods, np.uint8))
        cnt = e.read_spread()
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[2], plain[2])
    tally = counts.astype(np.int64).copy()
    on = (got[0] >= 0) & (group >= 0)
    on[on] &= dom[got[0][on]] >= 0
    np.add.at(tally, (group[on], dom[got[0][on]]), 1)
    assert on.sum() >= 50 and np.array_equal(cnt, tally)


# ---- 7. the states ---------------------------------------------------------------------------------------------------------------
def test_spread_two_halves(gpu_available, oracle_mod):
    a, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl, dom, skew, counts = a[:4]
    with engine(cl) as e:
        e.load_spread(dom, skew, counts)
        first = run(e, a, 0, 128)
        mid = e.read_spread()
        second = run(e, a, 128, 256)
        got = tuple(np.concatenate([x, y]) for x, y in zip(first, second))
        SR.same(got, e.read_spread(), e.read_nodes(), want)
    assert (mid != counts).any() and (mid != want[3]).any()


def test_spread_load_nodes_invalidates_and_reload_resets(gpu_available, oracle_mod):
    from ksched import KschedError
    from ksched import _lib as L
    a, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl, dom, skew, counts = a[:4]
    with engine(cl) as e:
        with pytest.raises(KschedError) as ei:  # no table yet
            run(e, a)
        assert ei.value.code == L.E_STATE
        e.load_spread(dom, skew, counts)
        run(e, a)
        assert np.array_equal(e.read_spread(), want[3]) and (want[3] != counts).any()
        e.load_spread(dom, skew, counts)  # a second load resets the counts
        assert np.array_equal(e.read_spread(), counts)
        e.load_spread(dom, skew)          # ... and NULL counts are zeros
        assert not e.read_spread().any() and e.read_spread().shape == counts.shape
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
        for call in (lambda: run(e, a), e.read_spread):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.load_spread(dom, skew, counts)
        SR.same(run(e, a), e.read_spread(), e.read_nodes(), want)


def test_spread_table_survives_other_calls(gpu_available, oracle_mod):
    from ksched import KschedError
    from ksched import _lib as L
    a, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl, dom, skew, counts = a[:4]
    probe = (cl.req_cpu[:16], cl.req_mem[:16], cl.req_pods[:16], None)
    with engine(cl) as e:  # what rank and schedule give without a table
        rank0 = e.rank(*probe, k=8)
        e.save_state()
        sched0 = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
    with engine(cl) as e:
        e.load_spread(dom, skew, counts)
        e.save_state()
        assert all(np.array_equal(x, y) for x, y in zip(e.rank(*probe, k=8), rank0))
        got = run(e, a)
        SR.same(got, e.read_spread(), e.read_nodes(), want)
        for call in (e.explain_batch, lambda: e.explain_pod(0)):  # they know no spread reason
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.restore_state()
        e.sync()
        assert np.array_equal(e.read_spread(), want[3])  # restore_state leaves the counts alone
        e.apply_delta([0, 5], [10, -10], [0, 0], [1, -1])
        e.apply_delta([0, 5], [-10, 10], [0, 0], [-1, 1])
        assert np.array_equal(e.read_spread(), want[3])
        assert all(np.array_equal(x, y) for x, y in zip(e.rank(*probe, k=8), rank0))
        sched = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        assert all(np.array_equal(x, y) for x, y in zip(sched, sched0)) and (sched[0] >= 0).any()
        assert np.array_equal(e.read_spread(), want[3])
        assert e.explain_batch()[1] == int((sched[0] == L.NO_FIT).sum())  # a plain call explains itself again


# ---- 8. every KSCHED_E_INVALID case: nothing changes, the loaded table survives ---------------------------------------------------
def test_spread_invalid_arguments(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    a, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl, dom, skew, counts, group, enforce = a
    n, p = cl.n_nodes, cl.n_pods

    def with_(arr, i, v):
        out = np.array(arr)
        out.flat[i] = v
        return out

    wide = np.arange(n) % 64
    loads = [
        ("D = 0", dict(node_domain=dom, max_skew=skew, n_domains=0)),
        ("S = 0", dict(node_domain=dom, max_skew=skew[:0], counts=counts[:0])),
        ("D above the cap", dict(node_domain=dom, max_skew=skew[:1], n_domains=L.SPREAD_MAX_DOMAINS + 1)),
        ("S above the cap", dict(node_domain=np.zeros(n), max_skew=np.ones(L.SPREAD_MAX_GROUPS + 1), n_domains=1)),
        ("S * D above the cells", dict(node_domain=wide, max_skew=np.ones(L.SPREAD_MAX_GROUPS), n_domains=65)),
        ("a node domain of D", dict(node_domain=with_(dom, 3, 4), max_skew=skew, counts=counts)),
        ("a node domain of -2", dict(node_domain=with_(dom, 3, -2), max_skew=skew, counts=counts)),
        ("a domain no node carries", dict(node_domain=dom, max_skew=skew, n_domains=5)),
        ("a domain no node carries, below the largest", dict(node_domain=np.where(dom == 1, 3, dom), max_skew=skew, counts=counts)),
        ("max_skew 0", dict(node_domain=dom, max_skew=with_(skew, 1, 0), counts=counts)),
        ("max_skew -1", dict(node_domain=dom, max_skew=with_(skew, 2, -1), counts=counts)),
        ("a count of -1", dict(node_domain=dom, max_skew=skew, counts=with_(counts, 5, -1))),
        ("a count above 2^30", dict(node_domain=dom, max_skew=skew, counts=with_(counts, 11, (1 << 30) + 1))),
    ]
    assert (np.bincount(wide, minlength=64) > 0).all() and 64 * 65 > L.SPREAD_MAX_CELLS >= 64 * 64
    with engine(cl) as e:
        e.load_spread(dom, skew, counts)
        run(e, a, 0, 64)
        rows, table = e.read_nodes(), e.read_spread()
        assert (table != counts).any()

        def unchanged():
            assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), rows))
            assert np.array_equal(e.read_spread(), table)

        for what, kw in loads:
            with pytest.raises(KschedError) as ei:
                e.load_spread(**kw)
            assert ei.value.code == L.E_INVALID, what
            unchanged()
        for what, g in (("a group of S", with_(group, 7, 3)), ("a group of -2", with_(group, p - 1, -2)),
                        ("a group of 2^20", with_(group, 0, 1 << 20))):
            with pytest.raises(KschedError) as ei:
                e.schedule_spread(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, g, enforce)
            assert ei.value.code == L.E_INVALID, what
            unchanged()
        # p >= 2^30: the count alone is refused, before any array is read
        one = np.zeros(1, np.int64)
        r = L.lib().ksched_schedule_spread(e._ctx, 1 << 30, L.ptr(one, C.c_int64), L.ptr(one, C.c_int64),
                                           L.ptr(one, C.c_int64), None, L.ptr(np.zeros(1, np.int32), C.c_int32), None,
                                           None, None, None)
        assert r == L.E_INVALID
        unchanged()
        # the table still works: the rest of the pods from where the first 64 left it
        rest = run(e, a, 64, 256)
        assert np.array_equal(rest[0], want[0][64:]) and np.array_equal(e.read_spread(), want[3])
    # opts.nranks > 1: neither call is served, and the rows stay
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0, nranks=2, rank=0,
                nodes_global=2 * n) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        for call in (lambda: e.load_spread(dom, skew, counts), lambda: run(e, a)):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_INVALID
        assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), cl.node_state()))
        with pytest.raises(KschedError) as ei:
            e.read_spread()
        assert ei.value.code == L.E_STATE


# ---- 9. FakeCluster.schedule_spread on Kubernetes JSON ---------------------------------------------------------------------------
def test_fake_cluster_schedule_spread(gpu_available):
    from test_spread_host import ZONE, kube_json
    from ksched import _lib as L
    from ksched.host import FakeCluster, Node
    nl, pl = kube_json()
    kw = dict(priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)
    fc = FakeCluster.from_kube_json(nl, pl, **kw)
    res = fc.schedule_spread()
    assert [p.name for p, _ in res] == [f"w{i}" for i in range(7)] + ["plain", "other"]
    assert all(isinstance(r, Node) for _, r in res)
    # the emptiest zone first, then the cheapest node of every zone the skew allows; n6 is cheapest, without a zone
    assert [r.name for _, r in res] == ["n4", "n0", "n2", "n4", "n0", "n2", "n4", "n6", "n6"]
    zone = {nd.name: nd.label_map.get(ZONE) for nd in fc.nodes}
    web = [zone[p.node_name] for p in fc.pods if p.labels.get("app") == "web" and p.spread is not None]
    assert len(web) == 9 and sorted(web.count(z) for z in "abc") == [3, 3, 3]   # 2 bound + 7 replicas, even
    placed = [zone[r.name] for p, r in res if p.name.startswith("w")]
    assert sorted(placed.count(z) for z in "abc") == [2, 2, 3] and None not in placed
    assert fc.engine.read_spread().tolist() == [[3, 3, 3]]                     # (`plain` landed on n6, outside every zone)
    assert len([e for e in fc.events if e["reason"] == "Scheduled"]) == 9
    fc.engine.close()
    # without the constraints every replica goes to the same node
    fc = FakeCluster.from_kube_json(nl, pl, **kw)
    res = fc.schedule_pods()
    assert {r.name for p, r in res} == {"n6"}
    fc.engine.close()
