"""ksched_schedule_ext on the device against the CPU restatement (ext_ref: the oracle, pod by pod, under the numpy
eligibility mask): idx, score bits, feasible, the final extended-resource table and the final node rows, all exactly.
The classes of pods each case is here for -- narrowed, moved, ext_nofit, zero_req, multi_col, exact_fit, overdrawn --
are asserted from the reference's output before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import ext_ref as ER

pytestmark = pytest.mark.gpu

_REF = {}


def case(O, n, p, R, priority=0, domain=0, labels=False):
    """(inputs, reference) of a named input, computed once and shared (never modified)."""
    key = (n, p, R, priority, domain, labels)
    if key not in _REF:
        a = ER.adversarial(7, n, p, R, priority, domain, labels)
        _REF[key] = (a, ER.schedule_ext(O, *a))
    return _REF[key]


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def run(e, a, lo=0, hi=None):
    cl, _, req_ext = a
    sel = None if cl.selector is None else cl.selector[lo:hi]
    return e.schedule_ext(cl.req_cpu[lo:hi], cl.req_mem[lo:hi], cl.req_pods[lo:hi], sel, req_ext[:, lo:hi])


def check(a, want, **kw):
    cl, node_ext, _ = a
    with engine(cl, **kw) as e:
        e.load_ext(node_ext)
        got = run(e, a)
        st = e.stats()
        ER.same(got, e.read_ext(), e.read_nodes(), want)
    assert st["pipeline"] == "exact" and st["pods"] == cl.n_pods and st["placed"] == int((want[0] >= 0).sum())
    assert st["pair_evals"] == cl.n_pods * cl.n_nodes


def minima(info, priority, domain):
    for k in ("narrowed", "ext_nofit", "zero_req", "multi_col", "exact_fit"):
        assert info[k] >= 10, (k, info)
    if priority == 1 or domain == 1:
        assert info["moved"] >= 10, info
    if priority == 0 and domain == 0:
        assert info["overdrawn"] >= 5, info
    else:  # an ineligible node wins only under resource priority over every node
        assert info["overdrawn"] == 0, info


# ---- 1. families: every instantiation family ------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_ext_families(priority, domain, labels, gpu_available, oracle_mod):
    a, want = case(oracle_mod, 64, 256, 4, priority, domain, labels)
    minima(want[5], priority, domain)
    check(a, want)


def test_ext_one_column(gpu_available, oracle_mod):
    a, want = case(oracle_mod, 64, 256, 1, 0, 1)
    info = want[5]
    assert info["narrowed"] >= 10 and info["moved"] >= 10 and info["zero_req"] >= 10 and info["exact_fit"] >= 10, info
    assert info["multi_col"] == 0 and a[1].shape == (1, 64)
    check(a, want)


# ---- 2. winners that other workgroups own, with uneven per_wg ---------------------------------------------------------------
@pytest.mark.parametrize("wgs", [1, 2, 4, 7])
def test_ext_workgroups(wgs, gpu_available, oracle_mod):
    a, want = case(oracle_mod, 64, 256, 4, 0, 1)
    minima(want[5], 0, 1)
    per_wg = -(-a[0].n_nodes // wgs)
    if wgs > 1:  # placements beyond workgroup 0's nodes
        assert (want[0] >= per_wg).sum() >= 10
    check(a, want, exact_wgs=wgs)


# ---- 3. one node, and node counts around the wave size ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
def test_ext_node_counts(n, gpu_available, oracle_mod):
    a, want = case(oracle_mod, n, 256, 4, 0, 1)
    info = want[5]
    assert info["narrowed"] >= 10 and info["ext_nofit"] >= 10 and info["zero_req"] >= 10 and (want[0] >= 0).sum() >= 10, info
    check(a, want)


# ---- 4. several node slots per thread ----------------------------------------------------------------------------------------
def test_ext_two_slots(gpu_available, oracle_mod):
    a, want = case(oracle_mod, 300, 256, 4, 0, 1)
    info = want[5]
    assert info["narrowed"] >= 10 and info["multi_col"] >= 10 and info["exact_fit"] >= 10, info
    assert (want[0] >= 256).sum() >= 10  # winners in slot k = 1
    check(a, want, exact_wgs=1)


def test_ext_eight_slots(gpu_available, oracle_mod):
    """n = 1025 on one workgroup: NPT = 8 and, with four columns, the largest LDS layout (64 KiB)."""
    a, want = case(oracle_mod, 1025, 512, 4, 0, 1)
    info = want[5]
    assert info["narrowed"] >= 10 and info["multi_col"] >= 10 and info["exact_fit"] >= 10, info
    assert (want[0] >= 1024).sum() >= 10 and (want[0] >= 256).sum() >= 100  # slot k = 4, and slots k >= 1
    assert len({int(w) // 256 for w in want[0] if w >= 0}) >= 4             # ... several different k
    check(a, want, exact_wgs=1)


# ---- 5. the header's worked example, output for output -------------------------------------------------------------------------
def test_ext_worked_example(gpu_available, oracle_mod):
    cl, node_ext, req_ext = ER.worked_example()
    with engine(cl) as e:
        e.load_ext(node_ext)
        idx, score, feas = e.schedule_ext(cl.req_cpu, cl.req_mem, cl.req_pods, None, req_ext)
        assert idx.tolist() == [0, 0, 2, -1] and feas.tolist() == [2, 3, 1, 0]
        assert e.read_ext().tolist() == [[0, 0, 0]]
        assert score.tolist() == [float(np.float32(0.1)), float(np.float32(0.1)), 0.5, 0.0]
    with engine(cl) as e:
        assert e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods)[0].tolist() == [0, 0, 0, 0]


# ---- 6. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("none", [False, True])
@pytest.mark.parametrize("priority", [0, 1])
def test_ext_zero_requests_is_schedule(priority, none, gpu_available, oracle_mod):
    a, _ = case(oracle_mod, 64, 256, 4, priority, 1)
    cl, node_ext, req_ext = a
    with engine(cl) as e:
        plain = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        plain_state, plain_st = e.read_nodes(), e.stats()
    with engine(cl) as e:
        e.load_ext(node_ext)
        got = e.schedule_ext(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, None if none else np.zeros_like(req_ext))
        state, st, table = e.read_nodes(), e.stats(), e.read_ext()
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1].view(np.int64), plain[1].view(np.int64))
    assert np.array_equal(got[2], plain[2]) and all(np.array_equal(x, y) for x, y in zip(state, plain_state))
    for k in ("pods", "placed", "batches", "truncations", "pair_evals", "pipeline", "rescues", "exact_rows", "scan_rows"):
        assert st[k] == plain_st[k], k
    assert np.array_equal(table, node_ext) and (got[0] >= 0).any()
    assert np.array_equal(got[0], oracle_mod.schedule(cl)[0])


def test_ext_table_survives_schedule(gpu_available, oracle_mod):
    a, want = case(oracle_mod, 64, 256, 4, 0, 1)
    cl, node_ext, _ = a
    with engine(cl) as e:
        sched0 = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        state0 = e.read_nodes()
    with engine(cl) as e:
        e.load_ext(node_ext)
        sched = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        assert all(np.array_equal(x, y) for x, y in zip(sched, sched0)) and (sched[0] >= 0).any()
        assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), state0))
        assert np.array_equal(e.read_ext(), node_ext)
        assert e.explain_batch()[1] == int((sched[0] == -1).sum())  # a plain call explains itself


# ---- 7. the table carries over from call to call -----------------------------------------------------------------------------------
def test_ext_two_halves(gpu_available, oracle_mod):
    a, want = case(oracle_mod, 64, 256, 4, 0, 1)
    cl, node_ext, req_ext = a
    half = ER.schedule_ext(oracle_mod, cl, node_ext, req_ext, hi=128)
    with engine(cl) as e:
        e.load_ext(node_ext)
        first = run(e, a, 0, 128)
        mid = e.read_ext()
        second = run(e, a, 128, 256)
        got = tuple(np.concatenate([x, y]) for x, y in zip(first, second))
        ER.same(got, e.read_ext(), e.read_nodes(), want)
    assert np.array_equal(mid, half[3]) and (mid != node_ext).any() and (mid != want[3]).any()


# ---- 8. states and every KSCHED_E_INVALID case: nothing changes, the loaded table survives -----------------------------------------
def test_ext_states(gpu_available, oracle_mod):
    from ksched import KschedError
    from ksched import _lib as L
    a, want = case(oracle_mod, 64, 256, 4, 0, 1)
    cl, node_ext, _ = a
    with engine(cl) as e:
        for call in (lambda: run(e, a), e.read_ext):  # no table yet
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.load_ext(node_ext)
        ER.same(run(e, a), e.read_ext(), e.read_nodes(), want)
        for call in (e.explain_batch, lambda: e.explain_pod(0)):  # they know no extended-resource reason
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.save_state()
        e.restore_state()
        e.sync()
        e.apply_delta([0, 5], [10, -10], [0, 0], [1, -1])
        assert np.array_equal(e.read_ext(), want[3])  # restore_state and apply_delta leave the table alone
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
        for call in (lambda: run(e, a), e.read_ext):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        e.load_ext(node_ext)
        ER.same(run(e, a), e.read_ext(), e.read_nodes(), want)


def test_ext_invalid_arguments(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    a, want = case(oracle_mod, 64, 256, 4, 0, 1)
    cl, node_ext, req_ext = a
    n, p = cl.n_nodes, cl.n_pods

    def with_(arr, i, v):
        out = np.array(arr)
        out.flat[i] = v
        return out

    with engine(cl) as e:
        e.load_ext(node_ext)
        run(e, a, 0, 64)
        rows, table = e.read_nodes(), e.read_ext()
        assert (table != node_ext).any()

        def unchanged():
            assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), rows))
            assert np.array_equal(e.read_ext(), table)

        lb, ptr = L.lib(), L.ptr(np.ascontiguousarray(node_ext), C.c_int64)
        for what, n_ext, arr in (("n_ext 0", 0, ptr), ("n_ext 5", L.EXT_MAX + 1, ptr), ("n_ext -1", -1, ptr),
                                 ("n_ext INT32_MAX", 2**31 - 1, ptr), ("n_ext INT32_MIN", -2**31, ptr),
                                 ("a null node_ext", 4, None)):
            assert lb.ksched_load_ext(e._ctx, n_ext, arr) == L.E_INVALID, what
            unchanged()
        for what, rq in (("a request of -1", with_(req_ext, 7, -1)), ("a request of INT64_MIN", with_(req_ext, 4 * p - 1, -2**63))):
            with pytest.raises(KschedError) as ei:
                e.schedule_ext(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, rq)
            assert ei.value.code == L.E_INVALID, what
            unchanged()
        # the table still works: the rest of the pods from where the first 64 left it
        rest = run(e, a, 64, 256)
        assert np.array_equal(rest[0], want[0][64:]) and np.array_equal(e.read_ext(), want[3])
    # opts.nranks > 1: neither call is served, and the rows stay
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0, nranks=2, rank=0,
                nodes_global=2 * n) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        for call in (lambda: e.load_ext(node_ext), lambda: run(e, a)):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_INVALID
        assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), cl.node_state()))
        with pytest.raises(KschedError) as ei:
            e.read_ext()
        assert ei.value.code == L.E_STATE


# ---- 9. FakeCluster.schedule_ext on Kubernetes JSON ------------------------------------------------------------------------------
def test_fake_cluster_schedule_ext(gpu_available):
    from test_ext_host import GPU, kube_json
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, Node
    nl, pl = kube_json()
    kw = dict(priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)
    fc = FakeCluster.from_kube_json(nl, pl, **kw)
    res = fc.schedule_ext()
    assert [p.name for p, _ in res] == ["g0", "cpu0", "g1", "g2", "g3"]
    # n0 is the cheapest but its one free GPU goes to g0; g1 needs two (n2); g2 takes n2's last two; g3 finds none
    assert [r.name if isinstance(r, Node) else type(r) for _, r in res] == ["n0", "n0", "n2", "n2", FitError]
    assert fc.engine.read_ext().tolist() == [[0, 0, 0]]
    assert len([ev for ev in fc.events if ev["reason"] == "FailedScheduling"]) == 1
    # a second call sees the binds of the first: the table is rebuilt from the bound pods
    res = fc.schedule_ext()
    assert [p.name for p, _ in res] == ["g3"] and isinstance(res[0][1], FitError)
    assert fc.engine.read_ext().tolist() == [[0, 0, 0]]
    assert sum(int(c.requests.get(GPU, 0)) for p in fc.pods if p.node_name == "n2" for c in p.containers) == 4
    fc.engine.close()
    # without the extended resources every pod goes to the cheapest node
    fc = FakeCluster.from_kube_json(nl, pl, **kw)
    assert {r.name for _, r in fc.schedule_pods()} == {"n0"}
    fc.engine.close()
