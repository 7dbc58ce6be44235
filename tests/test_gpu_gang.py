"""ksched_schedule_gangs on the device against the CPU restatement (gang_ref: the oracle, gang by gang): idx, score bits,
feasible, gang_placed and the final node rows, all exactly.  The classes of gangs each case is here for -- rejected,
rolled back, partially accepted, accepted after a rejected one -- are asserted from the reference's output."""
import dataclasses

import numpy as np
import pytest

import gang_ref as GR

pytestmark = pytest.mark.gpu

_REF = {}


def case(O, n, p, priority=0, domain=1, labels=False, gangs="cycle", half=False, edge=True):
    """(cluster, gang_off, gang_min | None, reference) of a named input, computed once and shared (never modified)."""
    key = (n, p, priority, domain, labels, gangs, half, edge)
    if key not in _REF:
        from ksched import cluster
        cl = cluster.random_small(7, n, p, priority=priority, domain=domain, use_labels=labels, edge=edge)
        off = GR.cycle_gangs(p) if gangs == "cycle" else np.asarray(gangs, dtype=np.int64)
        gmin = GR.half_min(off) if half else None
        _REF[key] = (cl, off, gmin, GR.schedule_gangs(O, cl, off, gmin))
    return _REF[key]


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def run(e, cl, off, gmin=None):
    got = e.schedule_gangs(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, off, gmin)
    return got, e.read_nodes()


def check(cl, off, gmin, want, **kw):
    with engine(cl, **kw) as e:
        got, state = run(e, cl, off, gmin)
        st = e.stats()
    GR.same(got, state, want)
    assert st["pipeline"] == "exact" and st["pods"] == cl.n_pods and st["placed"] == int(want[3].sum())
    assert st["pair_evals"] == cl.n_pods * cl.n_nodes


# ---- 1. parity: every instantiation family, all members required and half of them -----------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_gang_parity(priority, domain, labels, half, gpu_available, oracle_mod):
    cl, off, gmin, want = case(oracle_mod, 64, 256, priority, domain, labels, half=half)
    assert off.shape[0] - 1 == 48
    info = want[5]
    if half:
        assert info["partial"] >= 5 and info["rollbacks"] >= 5, info
    else:
        assert info["rejected"] >= 5 and info["rollbacks"] >= 5 and info["accepted_after_reject"] >= 5, info
    check(cl, off, gmin, want)


# ---- 2. a rollback touches nodes of workgroups other than 0, with uneven per_wg ---------------------------------------
@pytest.mark.parametrize("wgs", [1, 2, 4, 7])
def test_gang_workgroups(wgs, gpu_available, oracle_mod):
    cl, off, gmin, want = case(oracle_mod, 64, 256)
    per_wg = -(-cl.n_nodes // wgs)
    rolled = want[0] == GR.GANG_REJECTED  # (their nodes are not in the outputs: the plain schedule's picks stand in)
    assert want[5]["rollbacks"] >= 5 and rolled.sum() >= 5
    if wgs > 1:  # accepted placements do land beyond workgroup 0's nodes, so rolled-back ones of the same inputs do too
        assert (want[0][want[0] >= 0] >= per_wg).any()
    check(cl, off, gmin, want, exact_wgs=wgs)


# ---- 3. one node, and node counts around the wave size -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
def test_gang_node_counts(n, gpu_available, oracle_mod):
    cl, off, gmin, want = case(oracle_mod, n, 256)
    assert want[5]["rejected"] == {1: 45, 63: 23, 65: 20}[n], want[5]
    check(cl, off, gmin, want)


# ---- 4. two node slots per thread ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", [0, 1])
def test_gang_two_slots(domain, gpu_available, oracle_mod):
    cl, off, gmin, want = case(oracle_mod, 300, 2048, domain=domain)
    assert (want[5]["rejected"], want[5]["rollbacks"]) == ((166, 152), (183, 167))[domain], want[5]
    check(cl, off, gmin, want, exact_wgs=1)


@pytest.mark.parametrize("n", [600, 1100])
def test_gang_four_and_eight_slots(n, gpu_available, oracle_mod):
    """One workgroup of 256 threads: 4 and 8 slots per thread, the widest instantiations (labels, all-node domain)."""
    cl, off, gmin, want = case(oracle_mod, n, 1024, domain=0, labels=True)
    assert want[5]["rollbacks"] >= 5 and want[5]["accepted_after_reject"] >= 5, want[5]
    check(cl, off, gmin, want, exact_wgs=1)


# ---- 5. the cap ---------------------------------------------------------------------------------------------------------
def test_gang_cap_rollback(gpu_available, oracle_mod):
    cl, off, gmin, want = case(oracle_mod, 64, 1100, gangs=(0, 1024, 1100))
    assert want[3][0] == 0 and (want[0][:1024] == GR.GANG_REJECTED).sum() >= 200  # several hundred commits undone
    check(cl, off, gmin, want)


def test_gang_cap_accepted(gpu_available, oracle_mod):
    cl, off, _, _ = case(oracle_mod, 64, 1100, gangs=(0, 1024, 1100))
    gmin = np.array([512, 76], np.int32)
    want = GR.schedule_gangs(oracle_mod, cl, off, gmin)
    assert want[3][0] == 603  # accepted with members that failed
    check(cl, off, gmin, want)


def test_gang_above_cap_is_invalid(gpu_available, oracle_mod):
    from ksched import KschedError
    from ksched import _lib as L
    cl, _, _, _ = case(oracle_mod, 64, 1100, gangs=(0, 1024, 1100))
    with engine(cl) as e:
        for off, gmin in (((0, 1025, 1100), None), ((0, 1024, 1024, 1100), None), ((0, 1024, 1099), None),
                          ((1, 1024, 1100), None), ((0, 1024, 1100), (0, 76)), ((0, 1024, 1100), (1024, 77)),
                          # an offset above p, then back down to p: nothing may be staged from the gangs before it
                          ((0, 1000, 2000, 1100), None), ((0, 1000, 1900, 2800, 1100), (1, 1, 1, 1)),
                          ((0, 1101, 1100), None), ((0, -5, 1100), None), ((0, 1 << 62, 1100), None)):
            with pytest.raises(KschedError) as ei:
                run(e, cl, np.asarray(off, np.int64), None if gmin is None else np.asarray(gmin, np.int32))
            assert ei.value.code == L.E_INVALID, (off, gmin)
            assert all(np.array_equal(a, b) for a, b in zip(e.read_nodes(), cl.node_state()))


def test_gang_offset_above_p_is_invalid(gpu_available):
    """Five pods, gang_off = {0, 800, 5}: gang 0 passes the size cap, and its end lies far beyond the pods."""
    from ksched import KschedError
    from ksched import _lib as L
    cl, _ = GR.worked_example()
    with engine(cl) as e:
        for off in ((0, 800, 5), (0, 6, 5), (0, 3, 900, 5)):
            with pytest.raises(KschedError) as ei:
                run(e, cl, np.asarray(off, np.int64))
            assert ei.value.code == L.E_INVALID, off
            assert all(np.array_equal(a, b) for a, b in zip(e.read_nodes(), cl.node_state()))
        got, state = run(e, cl, np.asarray((0, 2, 4, 5), np.int64))  # and the context still works
        assert got[0].tolist() == [0, 1, GR.GANG_REJECTED, -1, 0] and state[0].tolist() == [0, 400]


# ---- 6. gangs of one are the plain exact schedule ------------------------------------------------------------------------
@pytest.mark.parametrize("priority", [0, 1])
def test_gang_size_one_is_schedule(priority, gpu_available, oracle_mod):
    from ksched import cluster
    cl = cluster.random_small(7, 64, 256, priority=priority, domain=1)
    with engine(cl) as e:
        plain = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        plain_state = e.read_nodes()
    with engine(cl) as e:
        got, state = run(e, cl, np.arange(cl.n_pods + 1))
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1].view(np.int64), plain[1].view(np.int64))
    assert np.array_equal(got[2], plain[2]) and np.array_equal(got[3], (plain[0] >= 0).astype(np.int32))
    assert all(np.array_equal(a, b) for a, b in zip(state, plain_state))
    want = oracle_mod.schedule(cl)
    assert np.array_equal(got[0], want[0]) and (got[0] >= 0).any() and (got[0] < 0).any()


# ---- 7. values below 2^52 everywhere: the FAST53 instantiations ----------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
def test_gang_fast53(domain, half, gpu_available, oracle_mod):
    cl, off, gmin, want = case(oracle_mod, 64, 256, domain=domain, half=half, edge=False)
    assert max(np.abs(cl.alloc_cpu).max(), np.abs(cl.req_cpu).max()) < 1 << 40
    assert want[5]["rollbacks"] >= 5, want[5]
    check(cl, off, gmin, want)


# ---- 8. the worked example ----------------------------------------------------------------------------------------------
def test_gang_worked_example(gpu_available, oracle_mod):
    cl, off = GR.worked_example()
    with engine(cl) as e:
        got, state = run(e, cl, off)
    assert got[0].tolist() == [0, 1, GR.GANG_REJECTED, -1, 0] and got[3].tolist() == [2, 0, 1]
    assert state[0].tolist() == [0, 400]
    GR.same(got, state, GR.schedule_gangs(oracle_mod, cl, off))


# ---- 9. the states --------------------------------------------------------------------------------------------------------
def test_gang_multirank_is_invalid(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    cl, off, gmin, _ = case(oracle_mod, 64, 256)
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0, nranks=2, rank=0,
                nodes_global=2 * cl.n_nodes) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        with pytest.raises(KschedError) as ei:
            run(e, cl, off, gmin)
        assert ei.value.code == L.E_INVALID
        assert all(np.array_equal(a, b) for a, b in zip(e.read_nodes(), cl.node_state()))


def test_gang_then_explain_and_schedule(gpu_available, oracle_mod):
    from ksched import KschedError
    from ksched import _lib as L
    cl, off, gmin, want = case(oracle_mod, 64, 256)
    with engine(cl) as e:
        got, state = run(e, cl, off, gmin)
        GR.same(got, state, want)
        with pytest.raises(KschedError) as ei:
            e.explain_batch()
        assert ei.value.code == L.E_STATE
        with pytest.raises(KschedError) as ei:
            e.explain_pod(0)
        assert ei.value.code == L.E_STATE
        # a plain schedule call goes on from the gang call's final state, and explains itself again
        nxt = dataclasses.replace(cl, alloc_cpu=want[4][0], alloc_mem=want[4][1], alloc_pods=want[4][2])
        ref = oracle_mod.schedule(nxt)
        oi, os_, of = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        assert np.array_equal(oi, ref[0]) and np.array_equal(os_.view(np.int64), ref[1].view(np.int64))
        assert np.array_equal(of, ref[2]) and (oi >= 0).any()
        assert all(np.array_equal(a, b) for a, b in zip(e.read_nodes(), ref[3]))
        assert e.explain_batch()[1] == int((oi == L.NO_FIT).sum())


# ---- 10. FakeCluster.schedule_gangs on Kubernetes JSON --------------------------------------------------------------------
def test_fake_cluster_schedule_gangs(gpu_available):
    from ksched import _lib as L
    from ksched.host import (GROUP_MIN_ANNOTATION, GROUP_NAME_ANNOTATION, PRICE_ANNOTATION, SCHEDULER_ANNOTATION,
                             FakeCluster, FitError, GangRejected)

    def node(name, price):
        return {"metadata": {"name": name, "annotations": {PRICE_ANNOTATION: price}},
                "status": {"capacity": {"cpu": "1", "memory": "1048576Ki", "pods": "110"}}}

    def pod(name, cpu, group=None, need=None):
        ann = {SCHEDULER_ANNOTATION: "hightower"}
        if group:
            ann[GROUP_NAME_ANNOTATION] = group
        if need:
            ann[GROUP_MIN_ANNOTATION] = str(need)
        return {"metadata": {"name": name, "annotations": ann},
                "spec": {"nodeName": "", "containers": [{"name": "c", "resources": {"requests": {"cpu": cpu}}}]}}

    def cluster(need=None):
        # the worked example, its gangs interleaved in the pod list
        nodes = {"items": [node("A", "0.10"), node("B", "0.50")]}
        pods = {"items": [pod("p0", "600m", "job1"), pod("p2", "300m", "job2", need), pod("p1", "600m", "job1"),
                          pod("p3", "600m", "job2"), pod("p4", "400m")]}
        return FakeCluster.from_kube_json(nodes, pods, priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)

    fc = cluster()
    res = fc.schedule_gangs()
    assert [p.name for p, _ in res] == ["p0", "p1", "p2", "p3", "p4"]
    assert [getattr(r, "name", type(r)) for _, r in res] == ["A", "B", GangRejected, FitError, "A"]
    assert [p.node_name for p, _ in res] == ["A", "B", "", "", "A"]
    assert [e["message"] for e in fc.events if e["reason"] == "Scheduled"] == [
        "Successfully assigned p0 to A", "Successfully assigned p1 to B", "Successfully assigned p4 to A"]
    assert [(e["involved"], e["message"]) for e in fc.events if e["reason"] == "FailedScheduling"] == [
        ("p2", "pod (p2) rejected with its gang (job2): 1 of 2 members placed, 2 needed"),
        ("p3", "pod (p3) failed to fit in any node")]
    assert fc.engine.read_nodes()[0].tolist() == [0, 400]
    fc.engine.close()
    # group-min-member 1: job2 is accepted with p2 alone, and p4 lands on B
    fc = cluster(need=1)
    res = fc.schedule_gangs()
    assert [getattr(r, "name", type(r)) for _, r in res] == ["A", "B", "A", FitError, "B"]
    assert [e["involved"] for e in fc.events if e["reason"] == "FailedScheduling"] == ["p3"]
    fc.engine.close()
