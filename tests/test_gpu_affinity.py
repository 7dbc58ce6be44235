"""ksched_schedule_affinity on the device against the CPU restatement (affinity_ref: the oracle, pod by pod, under the
numpy eligibility mask): idx, score bits, feasible, the three node arrays read back and the final node rows, all exactly.
The classes of pods each case is here for -- own_anti, symmetric, aff_narrowed, waived, aff_nofit, zone_moved,
off_domain, moved -- are asserted from the reference's output before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import affinity_ref as AR

pytestmark = pytest.mark.gpu

_REF = {}
SEED = 9  # (the draw on which the smallest family shape, D = 4 with 3 groups, still moves a zone word 11 times)


def case(O, kind, n, p, D, S, priority=0, domain=0, labels=False):
    """(input, reference) of a named input, computed once and shared (never modified)."""
    key = (kind, n, p, D, S, priority, domain, labels)
    if key not in _REF:
        c = AR.adversarial(SEED, n, p, D, S, priority, domain, labels) if kind == "adv" else AR.healthy(SEED, n, p, D, S)
        _REF[key] = (c, AR.schedule_affinity(O, c))
    return _REF[key]


def at_least(info, n=10, **once):
    """Every class of `once` at least that often, every other class at least n times."""
    for k, v in info.items():
        if k != "zone_moved_at":
            assert v >= once.get(k, n), (k, v, info)


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def run(e, c, lo=0, hi=None):
    cl = c.cl
    sel = None if cl.selector is None else cl.selector[lo:hi]
    return e.schedule_affinity(cl.req_cpu[lo:hi], cl.req_mem[lo:hi], cl.req_pods[lo:hi], sel, *c.pods(lo, hi))


def check(c, want, **kw):
    cl = c.cl
    with engine(cl, **kw) as e:
        e.load_affinity(*c.table(), n_domains=c.D)
        got = run(e, c)
        st = e.stats()
        AR.same(got, e.read_affinity(), e.read_nodes(), want)
    assert st["pipeline"] == "exact" and st["pods"] == cl.n_pods and st["placed"] == int((want[0] >= 0).sum())
    assert st["pair_evals"] == cl.n_pods * cl.n_nodes


def rows_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. families: every instantiation family ------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_affinity_families(priority, domain, labels, gpu_available, oracle_mod):
    c, want = case(oracle_mod, "adv", 64, 256, 4, 3, priority, domain, labels)
    at_least(want[7], waived=1, off_domain=1)
    check(c, want)


# ---- 2. winners that other workgroups own, with uneven per_wg; the zone words move on winners beyond workgroup 0's nodes -----
@pytest.mark.parametrize("wgs", [1, 2, 4, 7])
def test_affinity_workgroups(wgs, gpu_available, oracle_mod):
    c, want = case(oracle_mod, "adv", 64, 256, 8, 6, 0, 1)
    at_least(want[7], waived=1, off_domain=1)
    per_wg = -(-c.cl.n_nodes // wgs)
    if wgs > 1:
        assert (want[0][want[7]["zone_moved_at"]] >= per_wg).sum() >= 10
    check(c, want, exact_wgs=wgs)


# ---- 3. one node, and node counts around the wave size ---------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(1, 1), (63, 8), (65, 8)])
def test_affinity_node_counts(n, D, gpu_available, oracle_mod):
    c, want = case(oracle_mod, "adv", n, 256, D, 3)
    if n == 1:  # one node: the first pods of the groups, then the bound pods' terms decide
        assert want[7]["waived"] >= 10 and (want[0] >= 0).any() and (want[0] < 0).any(), want[7]
    else:
        at_least(want[7], waived=1, off_domain=1)
    check(c, want)


# ---- 4. two node slots per thread --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", [0, 1])
def test_affinity_two_slots(domain, gpu_available, oracle_mod):
    c, want = case(oracle_mod, "adv", 300, 2048, 16, 4, 0, domain)
    at_least(want[7], 30, waived=1)
    check(c, want, exact_wgs=1)


# ---- 5. the table at its caps ----------------------------------------------------------------------------------------------------
# (exact_wgs 1 puts the 1100 nodes on eight slots per thread and the 520 on four: the largest dynamic LDS tables)
@pytest.mark.parametrize("wgs", [0, 1])
def test_affinity_caps_domains(wgs, gpu_available, oracle_mod):
    c, want = case(oracle_mod, "healthy", 1100, 1500, 1024, 4)
    at_least(want[7], 20, waived=0, off_domain=0)
    assert want[7]["zone_moved"] >= 500 and c.node_domain.max() == 1023, want[7]
    check(c, want, exact_wgs=wgs)


@pytest.mark.parametrize("wgs", [0, 1])
def test_affinity_caps_groups(wgs, gpu_available, oracle_mod):
    c, want = case(oracle_mod, "healthy", 520, 1200, 256, 64)
    at_least(want[7], waived=10, off_domain=0)
    used = np.bitwise_or.reduce(want[3]) | np.bitwise_or.reduce(want[4]) | np.bitwise_or.reduce(want[5])
    assert int(used) == (1 << 64) - 1  # every one of the 64 bits, the top one included
    check(c, want, exact_wgs=wgs)


def test_affinity_host_scope_only(gpu_available, oracle_mod):
    c, want = case(oracle_mod, "adv", 64, 256, 0, 3, 0, 1)
    at_least(want[7], waived=1, zone_moved=0)
    assert c.node_domain is None and c.D == 0 and not c.anti_zone.any() and not c.aff_zone.any()
    check(c, want)


# ---- 6. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("priority", [0, 1])
def test_affinity_empty_pods_are_schedule(priority, gpu_available, oracle_mod):
    c, _ = case(oracle_mod, "adv", 64, 256, 4, 3, priority, 1)
    cl = c.cl
    with engine(cl) as e:
        plain = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        plain_state, plain_st = e.read_nodes(), e.stats()
    with engine(cl) as e:
        e.load_affinity(*c.table())
        assert rows_equal(e.read_affinity(), c.table()[1:])  # the table reads back as loaded
        got = e.schedule_affinity(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        state, st, tab = e.read_nodes(), e.stats(), e.read_affinity()
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1].view(np.int64), plain[1].view(np.int64))
    assert np.array_equal(got[2], plain[2]) and rows_equal(state, plain_state)
    for k in ("pods", "placed", "batches", "truncations", "pair_evals", "pipeline", "rescues", "exact_rows", "scan_rows"):
        assert st[k] == plain_st[k], k
    assert rows_equal(tab, c.table()[1:]) and c.node_member.any() and (got[0] >= 0).any() and (got[0] < 0).any()
    assert np.array_equal(got[0], oracle_mod.schedule(cl)[0])


def test_affinity_null_table_is_zeros(gpu_available, oracle_mod):
    from ksched import _lib as L
    c, _ = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    with engine(c.cl) as e:
        e.load_affinity(c.node_domain)
        assert not any(x.any() for x in e.read_affinity())
        out = np.full(64, 5, np.uint64)  # any pointer may be NULL
        assert L.lib().ksched_read_affinity(e._ctx, None, None, L.ptr(out, C.c_uint64)) == L.OK and not out.any()
        assert L.lib().ksched_read_affinity(e._ctx, None, None, None) == L.OK


# ---- 7. carry-over: the pods in two calls give what one call gives, table included ---------------------------------------------------
def test_affinity_two_halves(gpu_available, oracle_mod):
    c, want = case(oracle_mod, "adv", 64, 256, 8, 6, 0, 1)
    with engine(c.cl) as e:
        e.load_affinity(*c.table())
        first = run(e, c, 0, 100)
        mid = e.read_affinity()
        second = run(e, c, 100, 256)
        got = tuple(np.concatenate([x, y]) for x, y in zip(first, second))
        AR.same(got, e.read_affinity(), e.read_nodes(), want)
    assert (mid[0] != c.node_member).any() and (mid[0] != want[3]).any()
    # both calls move zone words, and the second starts from the any words the first left
    at = np.array(want[7]["zone_moved_at"])
    assert (at < 100).sum() >= 5 and (at >= 100).sum() >= 5


# ---- 8. state and errors ---------------------------------------------------------------------------------------------------------------
def test_affinity_states(gpu_available, oracle_mod):
    from ksched import KschedError
    from ksched import _lib as L
    c, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl = c.cl
    with engine(cl) as e:
        for call in (lambda: run(e, c), e.read_affinity):  # no table yet
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.load_affinity(*c.table())
        AR.same(run(e, c), e.read_affinity(), e.read_nodes(), want)
        for call in (e.explain_batch, lambda: e.explain_pod(0)):  # they know no affinity reason
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
        for call in (lambda: run(e, c), e.read_affinity):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.load_affinity(*c.table())
        AR.same(run(e, c), e.read_affinity(), e.read_nodes(), want)


def test_affinity_table_beside_other_tables(gpu_available, oracle_mod):
    c, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl = c.cl
    n, p = cl.n_nodes, cl.n_pods
    dom = np.where(c.node_domain < 0, 0, c.node_domain)
    counts = np.arange(8, dtype=np.int32).reshape(2, 4)
    ext = np.arange(2 * n, dtype=np.int64).reshape(2, n)
    with engine(cl) as e:
        sched0 = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
    with engine(cl) as e:
        e.load_spread(dom, np.ones(2, np.int32), counts)
        e.load_ext(ext)
        e.load_affinity(*c.table())
        e.save_state()
        AR.same(run(e, c), e.read_affinity(), e.read_nodes(), want)
        assert np.array_equal(e.read_spread(), counts) and np.array_equal(e.read_ext(), ext)  # neither read nor moved
        e.restore_state()
        e.sync()
        assert rows_equal(e.read_affinity(), want[3:6])  # restore_state leaves the words alone
        e.apply_delta([0, 5], [10, -10], [0, 0], [1, -1])
        e.apply_delta([0, 5], [-10, 10], [0, 0], [-1, 1])
        # the other calls neither read nor move the affinity table
        assert rows_equal(e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector), sched0)
        e.restore_state()
        e.sync()
        e.schedule_spread(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, np.zeros(p, np.int32))
        e.restore_state()
        e.sync()
        e.schedule_ext(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, np.ones((2, p), np.int64))
        assert rows_equal(e.read_affinity(), want[3:6])
        assert e.read_spread().sum() > counts.sum() and e.read_ext().sum() < ext.sum()


def test_affinity_invalid_arguments(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    c, want = case(oracle_mod, "adv", 64, 256, 4, 3, 0, 1)
    cl, dom = c.cl, c.node_domain
    n, p = cl.n_nodes, cl.n_pods

    def with_(arr, i, v):
        out = np.array(arr)
        out.flat[i] = v
        return out

    loads = [
        ("D = -1", dict(node_domain=np.full(n, -1), n_domains=-1)),
        ("D above the cap", dict(node_domain=dom, n_domains=L.SPREAD_MAX_DOMAINS + 1)),
        ("a node domain of D", dict(node_domain=with_(dom, 3, 4), n_domains=4)),
        ("a node domain of -2", dict(node_domain=with_(dom, 3, -2), n_domains=4)),
        ("a node domain of 0 with D = 0", dict(node_domain=with_(np.full(n, -1), 9, 0), n_domains=0)),
        ("a domain no node carries", dict(node_domain=dom, n_domains=5)),
        ("a domain no node carries, below the largest", dict(node_domain=np.where(dom == 1, 3, dom), n_domains=4)),
        ("node_domain NULL with D > 0", dict(node_domain=None, n_domains=4)),
    ]
    with engine(cl) as e:
        e.load_affinity(*c.table())
        run(e, c, 0, 64)
        rows, table = e.read_nodes(), e.read_affinity()
        assert (table[0] != c.node_member).any()

        def unchanged():
            assert rows_equal(e.read_nodes(), rows) and rows_equal(e.read_affinity(), table)

        for what, kw in loads:
            with pytest.raises(KschedError) as ei:
                e.load_affinity(node_member=c.node_member, **kw)
            assert ei.value.code == L.E_INVALID, what
            unchanged()
        for what, g in (("a group of 64", with_(c.aff_group, 7, 64)), ("a group of -2", with_(c.aff_group, p - 1, -2)),
                        ("a group of 2^20", with_(c.aff_group, 0, 1 << 20))):
            with pytest.raises(KschedError) as ei:
                e.schedule_affinity(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.member, c.anti_host, c.anti_zone,
                                    g, c.aff_zone)
            assert ei.value.code == L.E_INVALID, what
            unchanged()
        # p outside [0, 2^30): the count alone is refused, before any array is read
        one = np.zeros(1, np.int64)
        for bad in (1 << 30, -1):
            r = L.lib().ksched_schedule_affinity(e._ctx, bad, L.ptr(one, C.c_int64), L.ptr(one, C.c_int64),
                                                 L.ptr(one, C.c_int64), None, None, None, None,
                                                 L.ptr(np.zeros(1, np.int32), C.c_int32), None, None, None, None)
            assert r == L.E_INVALID
            unchanged()
        # the table still works: the rest of the pods from where the first 64 left it
        rest = run(e, c, 64, 256)
        assert np.array_equal(rest[0], want[0][64:]) and rows_equal(e.read_affinity(), want[3:6])
    # opts.nranks > 1: no call is served, and the rows stay
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0, nranks=2, rank=0,
                nodes_global=2 * n) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        for call in (lambda: e.load_affinity(*c.table()), lambda: run(e, c)):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_INVALID
        assert rows_equal(e.read_nodes(), cl.node_state())
        with pytest.raises(KschedError) as ei:
            e.read_affinity()
        assert ei.value.code == L.E_STATE


# ---- 9. the worked example of include/ksched.h ------------------------------------------------------------------------------------
def test_affinity_worked_example(gpu_available, oracle_mod):
    c = AR.worked_example()
    want = AR.schedule_affinity(oracle_mod, c)
    with engine(c.cl) as e:
        e.load_affinity(*c.table())
        got = run(e, c)
        tab = e.read_affinity()
        AR.same(got, tab, e.read_nodes(), want)
    assert got[0].tolist() == [0, 1, 0, 1, -1, 2, 3, 0, 0] and got[2].tolist() == [4, 3, 3, 1, 0, 2, 1, 4, 2]
    assert [t.tolist() for t in tab] == [[7, 3, 1, 1], [1, 1, 1, 0], [2, 2, 0, 0]]
    with engine(c.cl) as e:
        assert e.schedule(c.cl.req_cpu, c.cl.req_mem, c.cl.req_pods)[0].tolist() == [0] * 9


# ---- 10. FakeCluster.schedule_affinity on Kubernetes JSON ---------------------------------------------------------------------------
def test_fake_cluster_schedule_affinity(gpu_available, oracle_mod):
    from test_affinity_host import kube_case, kube_json
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, Node
    nl, pl = kube_json()
    kw = dict(priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)
    ref_case = kube_case()
    want = AR.schedule_affinity(oracle_mod, ref_case)
    fc = FakeCluster.from_kube_json(nl, pl, **kw)
    res = fc.schedule_affinity()
    assert [p.name for p, _ in res] == ["web-1", "web-2", "web-3", "cache-0", "cache-1", "cache-2", "plain"]
    names = [r.name if isinstance(r, Node) else None for _, r in res]
    assert names == [f"n{i}" if i >= 0 else None for i in want[0]] == ["n1", "n2", "n3", "n0", None, None, "n0"]
    assert all(isinstance(r, FitError) for _, r in res[4:6])
    AR.same((want[0], want[1], want[2]), fc.engine.read_affinity(), fc.engine.read_nodes(), want)
    assert len([e for e in fc.events if e["reason"] == "Scheduled"]) == 5
    assert len([e for e in fc.events if e["reason"] == "FailedScheduling"]) == 2
    fc.engine.close()
    # without the terms every pod goes to the cheapest node
    fc = FakeCluster.from_kube_json(nl, pl, **kw)
    assert {r.name for _, r in fc.schedule_pods()} == {"n0"}
    fc.engine.close()
