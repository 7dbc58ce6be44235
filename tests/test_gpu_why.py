"""ksched_schedule_full_why on the device against the CPU restatements: the four ordinary outputs, the node rows and the
three tables against full_ref exactly as test_gpu_full.py compares ksched_schedule_full's (the call IS that call), and
the rows of the pods that fit nowhere against why_ref -- nofit, the pod list, all 14 columns of every row and every byte
of the per-node rows, exactly.  What each case is here for -- enough NO_FIT pods whose codes at their turn differ from
the end state's and from the gang-start variant's -- is asserted from the reference alone in test_why_host.py."""
import ctypes as C

import numpy as np
import pytest

import full_ref as FR
import why_ref as WR
from test_gpu_full import STAT_KEYS, engine, load, tables
from test_why_host import differing, why_case

pytestmark = pytest.mark.gpu


def run(e, c, **kw):
    cl = c.cl
    return e.schedule_full_why(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.gang_off, c.gang_min, c.group, c.enforce,
                               c.req_ext, *c.aff_pods(), **kw)


def fresh(e, c):
    """The engine back at the case's start: the rows reloaded (which drops the tables), then the tables."""
    cl = c.cl
    e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
    load(e, c)


def check(c, ref, why, node_rows=None, **kw):
    """One call with why_rows = p and node_rows (None: every NO_FIT pod's) against both references."""
    nr = why[3] if node_rows is None else node_rows
    with engine(c.cl, **kw) as e:
        load(e, c)
        got = run(e, c, node_rows=nr)
        st = e.stats()
        FR.same(got[:4], *tables(e, c), e.read_nodes(), ref)
    WR.same(got[4], why, node_rows=nr)
    bound = int(ref[3].sum()) if c.gang_off is not None else int((ref[0] >= 0).sum())
    assert st["pipeline"] == "exact" and st["pods"] == c.cl.n_pods and st["placed"] == bound
    assert st["pair_evals"] == c.cl.n_pods * c.cl.n_nodes
    return got


# ---- 1. the header's worked example ---------------------------------------------------------------------------------------------------
def test_why_worked_example(gpu_available, oracle_mod):
    c = FR.worked_example()
    ref = FR.schedule_full(oracle_mod, c)
    got = check(c, ref, WR.why(oracle_mod, c, ref))
    pods, counts, reasons, nofit = got[4]
    assert got[0].tolist() == [-3, -3, -1, 0, 1, 2] and nofit == 1 and pods.tolist() == [2]
    assert reasons.tolist() == [[5, 5, 11, 5]] and counts.tolist() == [[0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 1, 0, 0]]


# ---- 2. families: every instantiation family, all members required and half of them ----------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_why_families(priority, domain, labels, half, gpu_available, oracle_mod):
    check(*why_case(oracle_mod, ("family", priority, domain, labels, half)))


# ---- 3. the workgroups' sums meet in the atomics, with uneven per_wg; every per-node row written ----------------------------------
@pytest.mark.parametrize("wgs", [1, 2, 4, 7])
def test_why_workgroups(wgs, gpu_available, oracle_mod):
    check(*why_case(oracle_mod, "workgroups"), exact_wgs=wgs)


# ---- 4. one node, and node counts around the wave size ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
def test_why_node_counts(n, gpu_available, oracle_mod):
    check(*why_case(oracle_mod, ("nodes", n)))


# ---- 5. several node slots per thread: the slot rows k >= 1 are written -----------------------------------------------------------
def test_why_two_slots(gpu_available, oracle_mod):
    c, ref, why = why_case(oracle_mod, "two_slots")
    assert len(np.unique(why[2][:, 256:])) >= 5  # codes in slot row k = 1
    check(c, ref, why, exact_wgs=1)


def test_why_eight_slots(gpu_available, oracle_mod):
    """n = 1100 on one workgroup with labels, four columns and both tables: NPT = 8, the widest instantiation."""
    c, ref, why = why_case(oracle_mod, "eight_slots")
    assert len(np.unique(why[2][:, 1024:])) >= 5 and c.req_ext.shape[0] == 4
    check(c, ref, why, exact_wgs=1)


def test_why_no_zone_key(gpu_available, oracle_mod):
    c, ref, why = why_case(oracle_mod, "no_zone_key")
    assert c.aff_D == 0 and c.aff_domain is None
    check(c, ref, why)


# ---- 6. the caps ------------------------------------------------------------------------------------------------------------------
def test_why_caps(gpu_available, oracle_mod):
    c, ref, (pods, counts, reasons, nofit) = why_case(oracle_mod, "workgroups")
    p, n = c.cl.n_pods, c.cl.n_nodes
    assert nofit > 7
    with engine(c.cl) as e:
        # why_rows = 7 < nofit, node_rows = 3: the prefix is recorded, nofit is the total
        load(e, c)
        got = run(e, c, why_rows=7, node_rows=3)
        FR.same(got[:4], *tables(e, c), e.read_nodes(), ref)
        WR.same(got[4], (pods[:7], counts[:7], reasons[:7], nofit), node_rows=3)
        # more rows than NO_FIT pods: the rest is -1 / 0 / 0
        fresh(e, c)
        got = run(e, c, why_rows=nofit + 5, node_rows=nofit + 2, trim=False)
        gp, gc, gr, gn = got[4]
        assert gn == nofit and gp.shape == (nofit + 5,) and gc.shape == (nofit + 5, 14) and gr.shape == (nofit + 2, n)
        WR.same((gp[:nofit], gc[:nofit], gr[:nofit], gn), (pods, counts, reasons, nofit))
        assert (gp[nofit:] == -1).all() and (gc[nofit:] == 0).all() and (gr[nofit:] == 0).all()
        # why_rows = 0: only the total
        fresh(e, c)
        got = run(e, c, why_rows=0)
        FR.same(got[:4], *tables(e, c), e.read_nodes(), ref)
        assert got[4][0].shape == (0,) and got[4][1].shape == (0, 14) and got[4][2] is None and got[4][3] == nofit
        # why_rows = p, node_rows = 0 with a NULL byte buffer
        fresh(e, c)
        got = run(e, c, why_rows=p, node_rows=0)
        FR.same(got[:4], *tables(e, c), e.read_nodes(), ref)
        assert got[4][2] is None
        WR.same(got[4], (pods, counts, reasons, nofit), node_rows=0)


# ---- 7. equivalences ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("priority,n", [(0, 8), (1, 16)])
def test_why_all_off_is_explain_pod_of_schedule(priority, n, gpu_available, oracle_mod):
    """With every constraint NULL the rows are Engine.explain_pod's of a plain exact schedule on the same input: the
    at-its-turn explain the plain path already has, codes 0-4 only.  Few nodes, so that the plain predicate alone
    leaves pods without a node (at 64 nodes four pods do): at least 10 here, the label code among their reasons."""
    from test_full_host import case
    c, _ = case(oracle_mod, n, 256, priority=priority, domain=1, labels=True)
    cl = c.cl
    plain = FR.Case(cl)  # every constraint off: the reference is the oracle's schedule, pod by pod
    ref = FR.schedule_full(oracle_mod, plain)
    why = WR.why(oracle_mod, plain, ref)
    assert why[3] >= 10 and why[2].max() <= 4 and (why[2] == 4).any()
    with engine(cl) as e:
        idx, score, feas = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        rows = e.read_nodes()
        nf = np.flatnonzero(idx == -1)
        want = [e.explain_pod(int(i)) for i in nf]
    assert np.array_equal(idx, ref[0])
    with engine(cl) as e:
        got = e.schedule_full_why(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, node_rows=len(nf))
        assert np.array_equal(got[0], idx) and np.array_equal(got[1].view(np.int64), score.view(np.int64)) and np.array_equal(got[2], feas)
        assert all(np.array_equal(a, b) for a, b in zip(e.read_nodes(), rows))
        pods, counts, reasons, nofit = got[4]
    WR.same(got[4], why)
    assert nofit == len(nf) and pods.tolist() == nf.tolist() and (counts[:, 5:] == 0).all()
    for r, (cnt, rs) in enumerate(want):
        assert counts[r, :5].tolist() == cnt.tolist() and np.array_equal(reasons[r], rs), int(nf[r])


@pytest.mark.parametrize("half", [False, True])
def test_why_is_schedule_full(half, gpu_available, oracle_mod):
    """On the same input ksched_schedule_full and ksched_schedule_full_why return identical outputs and leave identical
    state and stats."""
    c, _, _ = why_case(oracle_mod, ("family", 0, 1, True, half))
    cl = c.cl
    out = []
    for why in (False, True):
        with engine(cl) as e:
            load(e, c)
            args = (cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.gang_off, c.gang_min, c.group, c.enforce, c.req_ext,
                    *c.aff_pods())
            got = e.schedule_full_why(*args, node_rows=4)[:4] if why else e.schedule_full(*args)
            out.append((got, e.read_nodes(), e.stats(), e.read_ext(), e.read_spread(), e.read_affinity()))
    a, b = out
    for x, y in zip(list(a[0]) + list(a[1]) + [a[3], a[4]] + list(a[5]), list(b[0]) + list(b[1]) + [b[3], b[4]] + list(b[5])):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    for k in STAT_KEYS:
        assert a[2][k] == b[2][k], k
    assert (a[0][0] == FR.GANG_REJECTED).any() and (a[0][0] == -1).any()


# ---- 8. invalid arguments leave everything alone ------------------------------------------------------------------------------------
def raw(e, c, why_rows, node_rows, pod=True, counts=True, reason=True):
    """The C call itself, for arguments the binding would not pass; buffers of 64 rows."""
    from ksched import _lib as L
    cl = c.cl
    p, n = cl.n_pods, cl.n_nodes
    i32, i64, u8, u64 = C.c_int32, C.c_int64, C.c_uint8, C.c_uint64
    oi = np.empty(p, np.int32); os_ = np.empty(p, np.float64); of = np.empty(p, np.int32); gp = np.empty(p, np.int32)
    wp = np.empty(64, np.int32); wc = np.empty(64 * 14, np.int64); wr = np.empty(64 * n, np.uint8); nf = np.zeros(1, np.int64)
    arr = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)
    keep = [arr(c.gang_off, np.int64), arr(c.gang_min, np.int32), arr(c.group, np.int32), arr(c.enforce, np.uint8),
            arr(c.req_ext, np.int64), arr(c.member, np.uint64), arr(c.anti_host, np.uint64), arr(c.anti_zone, np.uint64),
            arr(c.aff_group, np.int32), arr(c.aff_zone, np.uint8)]
    types = [i64, i32, i32, u8, i64, u64, u64, u64, i32, u8]
    return L.lib().ksched_schedule_full_why(
        e._ctx, p, L.ptr(cl.req_cpu, i64), L.ptr(cl.req_mem, i64), L.ptr(cl.req_pods, i64), L.ptr(cl.selector, u64),
        keep[0].shape[0] - 1, *(L.ptr(a, t) for a, t in zip(keep, types)),
        L.ptr(oi, i32), L.ptr(os_, C.c_double), L.ptr(of, i32), L.ptr(gp, i32),
        why_rows, L.ptr(wp if pod else None, i32), L.ptr(wc if counts else None, i64),
        node_rows, L.ptr(wr if reason else None, u8), L.ptr(nf, i64))


def test_why_errors_leave_everything_alone(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine
    from ksched import _lib as L
    c, ref, why = why_case(oracle_mod, "workgroups")
    cl = c.cl
    rows_equal = lambda xs, ys: all(np.array_equal(x, y) for x, y in zip(xs, ys))
    n = cl.n_nodes
    bad = [("why_rows < 0", dict(why_rows=-1, node_rows=0)),
           ("node_rows < 0", dict(why_rows=4, node_rows=-1)),
           ("node_rows > why_rows", dict(why_rows=4, node_rows=5)),
           ("why_rows = 2^30", dict(why_rows=1 << 30, node_rows=0)),
           ("a NULL out_why_pod", dict(why_rows=4, node_rows=0, pod=False)),
           ("a NULL out_why_counts", dict(why_rows=4, node_rows=0, counts=False)),
           ("a NULL out_why_reason", dict(why_rows=4, node_rows=2, reason=False)),
           ("the per-node bytes above the bound", dict(why_rows=(1 << 28) // n + 1, node_rows=(1 << 28) // n + 1))]
    with engine(cl) as e:
        load(e, c)
        for what, kw in bad:
            assert raw(e, c, **kw) == L.E_INVALID, what
            assert rows_equal(e.read_nodes(), cl.node_state()), what
            assert np.array_equal(e.read_ext(), c.node_ext) and np.array_equal(e.read_spread(), c.counts), what
            assert rows_equal(e.read_affinity(), c.aff_table()[1:]), what
        # ksched_schedule_full's cases come first, with that call's code
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)  # (drops the tables)
        assert raw(e, c, why_rows=-1, node_rows=0) == L.E_STATE
        load(e, c)
        # the context still schedules correctly, and the plain explain calls still know none of the reasons
        got = run(e, c, node_rows=why[3])
        FR.same(got[:4], *tables(e, c), e.read_nodes(), ref)
        WR.same(got[4], why)
        from ksched import KschedError
        for call in (e.explain_batch, lambda: e.explain_pod(0)):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0, nranks=2, rank=0,
                nodes_global=2 * cl.n_nodes) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        assert raw(e, c, why_rows=4, node_rows=0) == L.E_INVALID
        assert rows_equal(e.read_nodes(), cl.node_state())


# ---- 9. at its turn, not now ------------------------------------------------------------------------------------------------------
def test_why_is_not_explain_full_afterwards(gpu_available, oracle_mod):
    """ksched_explain_full after the call answers against the end state: it disagrees with the recorded rows for exactly
    the pods the reference says -- at least 10 of them (asserted without a device in test_why_host.py)."""
    c, ref, why = why_case(oracle_mod, "workgroups")
    cl = c.cl
    pods, counts, reasons, nofit = why
    want = differing(WR.at_end(c, ref, pods), reasons)
    assert want.sum() >= 10
    with engine(cl) as e:
        load(e, c)
        got = run(e, c, node_rows=nofit)
        WR.same(got[4], why)
        after = np.stack([e.explain_full(int(cl.req_cpu[i]), int(cl.req_mem[i]), int(cl.req_pods[i]), 0,
                                         int(c.group[i]), bool(c.enforce[i]), c.req_ext[:, i], int(c.member[i]),
                                         int(c.anti_host[i]), int(c.anti_zone[i]), int(c.aff_group[i]),
                                         bool(c.aff_zone[i]))[1] for i in pods])
    assert np.array_equal(after, WR.at_end(c, ref, pods))
    assert np.array_equal(differing(after, got[4][2]), want)


# ---- 10. FakeCluster.schedule_full_why on Kubernetes JSON --------------------------------------------------------------------------
def test_fake_cluster_schedule_full_why(gpu_available):
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, GangRejected
    from test_full_host import kube_json
    nl, pl = kube_json()
    fc = FakeCluster.from_kube_json(nl, pl, priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)
    res = fc.schedule_full_why()
    assert [getattr(r, "name", type(r)) for _, r in res] == [GangRejected, GangRejected, FitError, "n0", "n1", "n2"]
    msg = [e["message"] for e in fc.events if e["reason"] == "FailedScheduling" and e["involved"] == "p2"]
    assert msg == ["pod (p2) failed to fit in any node\n"
                   "fit failure on node (n0): Insufficient amd.com/gpu\n"
                   "fit failure on node (n1): Insufficient amd.com/gpu\n"
                   "fit failure on node (n2): node(s) didn't match pod affinity rules\n"
                   "fit failure on node (n3): Insufficient amd.com/gpu"]
    fc.engine.close()
