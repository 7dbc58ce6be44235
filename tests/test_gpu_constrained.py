"""ksched_schedule_constrained on the device against the CPU restatement (constrained_ref: the oracle, gang by gang and
pod by pod, under the numpy eligibility mask, with the snapshot restored for a rejected gang): idx, score bits, feasible,
gang_placed, the final node rows, the final extended-resource table and the final spread counts, all exactly, and the
stats.  The classes each case is here for -- rollbacks, rejected gangs that undo extended columns and spread counts,
rollbacks that lower a row's minimum, partially accepted gangs -- are asserted from the reference's output before the
device is touched."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import constrained_ref as CR
import gang_ref as GR

pytestmark = pytest.mark.gpu

_REF = {}
# the generator's seed per family case (priority, domain, labels, half) where 7 misses a minimum below: under resource
# priority over every node an ineligible node can still win, so few members fail and few half-required gangs are rejected
SEEDS = {(0, 0, False, True): (85, 25), (0, 0, True, True): 48}


def case(O, n, p, **kw):
    """(case, reference) of a named input, computed once and shared (never modified)."""
    key = (n, p) + tuple(sorted(kw.items()))
    if key not in _REF:
        c = CR.adversarial(n, p, **kw)
        _REF[key] = (c, CR.schedule_constrained(O, c))
    return _REF[key]


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def load(e, c):
    if c.group is not None:
        e.load_spread(c.node_domain, c.max_skew, c.counts)
    if c.req_ext is not None:
        e.load_ext(c.node_ext)


def run(e, c):
    cl = c.cl
    return e.schedule_constrained(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.gang_off, c.gang_min, c.group,
                                  c.enforce, c.req_ext)


def tables(e, c):
    return (e.read_ext() if c.req_ext is not None else None), (e.read_spread() if c.group is not None else None)


def check(c, want, **kw):
    with engine(c.cl, **kw) as e:
        load(e, c)
        got = run(e, c)
        st = e.stats()
        CR.same(got, *tables(e, c), e.read_nodes(), want)
    bound = int(want[3].sum()) if c.gang_off is not None else int((want[0] >= 0).sum())
    assert st["pipeline"] == "exact" and st["pods"] == c.cl.n_pods and st["placed"] == bound
    assert st["pair_evals"] == c.cl.n_pods * c.cl.n_nodes


def minima(info, half=False):
    if half:
        assert info["rollbacks"] >= 5 and info["partial"] >= 10 and info["undo_spread"] >= 5, info
        assert info["undo_ext"] >= 3 and info["min_fell"] >= 3, info
    else:
        assert info["rollbacks"] >= 10 and info["undo_ext"] >= 10 and info["undo_spread"] >= 10, info
        assert info["min_fell"] >= 5, info


# ---- 1. families: every instantiation family, all members required and half of them ------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_constrained_families(priority, domain, labels, half, gpu_available, oracle_mod):
    seed = SEEDS.get((priority, domain, labels, half), 7)
    c, want = case(oracle_mod, 64, 256, priority=priority, domain=domain, labels=labels, half=half, seed=seed)
    minima(want[7], half)
    check(c, want)


# ---- 2. rollbacks of ext and rows in workgroups other than 0, with uneven per_wg ------------------------------------------------
@pytest.mark.parametrize("wgs", [1, 2, 4, 7])
def test_constrained_workgroups(wgs, gpu_available, oracle_mod):
    c, want = case(oracle_mod, 64, 256, domain=1)
    minima(want[7])
    per_wg = -(-c.cl.n_nodes // wgs)
    if wgs > 1:  # placements beyond workgroup 0's nodes (a rolled-back member's node is not in the outputs)
        assert (want[0] >= per_wg).sum() >= 10
    check(c, want, exact_wgs=wgs)


# ---- 3. one node, and node counts around the wave size -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
def test_constrained_node_counts(n, gpu_available, oracle_mod):
    c, want = case(oracle_mod, n, 256, D=min(3, n), domain=1)  # (one node carries one domain)
    minima(want[7])
    check(c, want)


# ---- 4. several node slots per thread -----------------------------------------------------------------------------------------------
def test_constrained_two_slots(gpu_available, oracle_mod):
    c, want = case(oracle_mod, 300, 1024, domain=1)
    minima(want[7])
    assert (want[0] >= 256).sum() >= 10  # winners in slot k = 1
    check(c, want, exact_wgs=1)


def test_constrained_eight_slots(gpu_available, oracle_mod):
    """n = 1100 on one workgroup: NPT = 8, the widest instantiation (labels), the slots' domains in 8 KiB of LDS and the
    four columns in 64 KiB."""
    c, want = case(oracle_mod, 1100, 1024, domain=1, labels=True)
    minima(want[7])
    assert (want[0] >= 1024).sum() >= 10 and len({int(w) // 256 for w in want[0] if w >= 0}) >= 4  # several k
    check(c, want, exact_wgs=1)


# ---- 5. the larger table: the minimum moves rarely -----------------------------------------------------------------------------
def test_constrained_sixteen_domains(gpu_available, oracle_mod):
    c, want = case(oracle_mod, 64, 256, D=16, S=4, domain=1)
    minima(want[7])
    assert want[7]["undo_spread"] - want[7]["min_fell"] >= 10, want[7]  # ... decrements that leave the minimum alone too
    check(c, want)


# ---- 6. the gang cap: one rejected gang undoes several hundred commits of each kind ----------------------------------------------
def test_constrained_gang_cap_rollback(gpu_available, oracle_mod):
    c, want = case(oracle_mod, 64, 1100, domain=1, gang_off=(0, 1024, 1100))
    rolled = want[0][:1024] == GR.GANG_REJECTED
    assert want[3][0] == 0 and rolled.sum() >= 200
    assert (rolled & (c.req_ext[:, :1024] != 0).any(axis=0)).sum() >= 100 and (rolled & (c.group[:1024] >= 0)).sum() >= 100
    check(c, want)


# ---- 7. the header's worked example, output for output -------------------------------------------------------------------------
def test_constrained_worked_example(gpu_available, oracle_mod):
    c = CR.worked_example()
    with engine(c.cl) as e:
        load(e, c)
        idx, score, feas, placed = run(e, c)
        assert idx.tolist() == [0, 2, 0, -3, -1, 1] and feas.tolist() == [3, 1, 2, 1, 0, 1]
        assert placed.tolist() == [3, 0, 1]
        assert e.read_spread().tolist() == [[2, 1]] and e.read_ext().tolist() == [[0, 0, 0]]
        assert score.tolist() == [float(np.float32(0.1)), 0.5, float(np.float32(0.1)), 0.0, 0.0, float(np.float32(0.2))]
        assert e.read_nodes()[2].tolist() == [108, 109, 109]  # n2's row is restored: it holds p1 only
        CR.same((idx, score, feas, placed), e.read_ext(), e.read_spread(), e.read_nodes(),
                CR.schedule_constrained(oracle_mod, c))


# ---- 8. equivalences: all off is schedule(); one constraint on is its own call, output for output and state for state ------------
STAT_KEYS = ("pods", "placed", "batches", "truncations", "pair_evals", "pipeline", "rescues", "exact_rows", "scan_rows")


def both(c, own, **on):
    """(results, rows, stats, ext, counts) of the constraint's own call and of schedule_constrained with only it on."""
    cl = c.cl
    out = []
    for composed in (False, True):
        with engine(cl) as e:
            load(e, c)
            if composed:
                got = e.schedule_constrained(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, **on)
                got = got if "gang_off" in on else got[:3]
            else:
                got = own(e)
            out.append((got, e.read_nodes(), e.stats(), e.read_ext(), e.read_spread()))
    return out


def identical(a, b, c):
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[0] + tuple(a[1]) + a[3:], b[0] + tuple(b[1]) + b[3:]):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                                     y.view(np.int64) if y.dtype == np.float64 else y)
    for k in STAT_KEYS:
        assert a[2][k] == b[2][k], k
    assert (a[0][0] >= 0).any() and (a[0][0] < 0).any()


@pytest.mark.parametrize("priority", [0, 1])
def test_constrained_all_off_is_schedule(priority, gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, priority=priority, domain=1)
    cl = c.cl
    a, b = both(c, lambda e: e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector))
    identical(a, b, c)
    assert b[0][0].shape == (256,) and np.array_equal(b[3], c.node_ext) and np.array_equal(b[4], c.counts)
    assert np.array_equal(b[0][0], oracle_mod.schedule(cl)[0])


@pytest.mark.parametrize("half", [False, True])
def test_constrained_gangs_alone_is_schedule_gangs(half, gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, domain=1, half=half)
    cl = c.cl
    a, b = both(c, lambda e: e.schedule_gangs(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.gang_off, c.gang_min),
                gang_off=c.gang_off, gang_min=c.gang_min)
    identical(a, b, c)
    if half:  # (on this roomy cluster, without the other two constraints, no half-required gang is rejected)
        assert ((b[0][3] > 0) & (b[0][3] < np.diff(c.gang_off))).any()  # accepted with members that failed
    else:
        assert (b[0][0] == GR.GANG_REJECTED).any() and (b[0][3] == 0).any()
    assert np.array_equal(b[3], c.node_ext) and np.array_equal(b[4], c.counts)


def test_constrained_spread_alone_is_schedule_spread(gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, domain=1)
    cl = c.cl
    a, b = both(c, lambda e: e.schedule_spread(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.group, c.enforce),
                group=c.group, enforce=c.enforce)
    identical(a, b, c)
    assert (b[4] != c.counts).any() and np.array_equal(b[3], c.node_ext)


def test_constrained_ext_alone_is_schedule_ext(gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, domain=1)
    cl = c.cl
    a, b = both(c, lambda e: e.schedule_ext(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.req_ext), req_ext=c.req_ext)
    identical(a, b, c)
    assert (b[3] != c.node_ext).any() and np.array_equal(b[4], c.counts)


# ---- 9. the tables carry over from call to call ---------------------------------------------------------------------------------------
def test_constrained_two_calls(gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, domain=1)
    off = GR.cycle_gangs(128)
    h1 = dataclasses.replace(CR.pods(c, 0, 128), gang_off=off)
    w1 = CR.schedule_constrained(oracle_mod, h1)
    h2 = dataclasses.replace(CR.pods(c, 128, 256), gang_off=off, node_ext=w1[4], counts=w1[5])
    w2 = CR.schedule_constrained(oracle_mod, h2, state=w1[6])
    assert min(w[7][k] for w in (w1, w2) for k in ("rollbacks", "undo_ext", "undo_spread", "min_fell")) >= 5
    assert (w1[4] != c.node_ext).any() and (w1[5] != c.counts).any() and (w2[4] != w1[4]).any() and (w2[5] != w1[5]).any()
    with engine(c.cl) as e:
        load(e, c)
        CR.same(run(e, h1), *tables(e, c), e.read_nodes(), w1)
        CR.same(run(e, h2), *tables(e, c), e.read_nodes(), w2)  # (without reloading: from the first call's tables)


# ---- 10. a constraint that is off needs no table, and leaves a loaded one alone -----------------------------------------------------
def test_constrained_absent_and_unused_tables(gpu_available, oracle_mod):
    from ksched import KschedError
    from ksched import _lib as L
    c, _ = case(oracle_mod, 64, 256, domain=1)
    gangs = dataclasses.replace(c, group=None, enforce=None, req_ext=None)
    want = CR.schedule_constrained(oracle_mod, gangs)
    assert want[7]["rollbacks"] >= 1
    with engine(c.cl) as e:  # no table loaded at all
        CR.same(run(e, gangs), None, None, e.read_nodes(), want)
        for call in (e.read_ext, e.read_spread):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
    for keep in ("spread", "ext"):  # one constraint on, the other's table absent
        one = dataclasses.replace(c, **(dict(req_ext=None) if keep == "spread" else dict(group=None, enforce=None)))
        w = CR.schedule_constrained(oracle_mod, one)
        with engine(c.cl) as e:
            load(e, one)
            CR.same(run(e, one), *tables(e, one), e.read_nodes(), w)
    with engine(c.cl) as e:  # both loaded, neither used: neither read nor moved
        load(e, c)
        CR.same(run(e, gangs), None, None, e.read_nodes(), want)
        assert np.array_equal(e.read_ext(), c.node_ext) and np.array_equal(e.read_spread(), c.counts)
    with engine(c.cl) as e:  # no pods: nothing moves, with every constraint on and with none
        load(e, c)
        for none in (CR.pods(gangs, 0, 0), dataclasses.replace(CR.pods(c, 0, 0), gang_off=np.zeros(1))):
            got = run(e, none)
            assert [x.shape for x in got] == [(0,)] * 4 and e.stats()["pods"] == 0
            assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), c.cl.node_state()))
            assert np.array_equal(e.read_ext(), c.node_ext) and np.array_equal(e.read_spread(), c.counts)


# ---- 11. states and every KSCHED_E_INVALID case: nothing changes, the loaded tables survive -----------------------------------------
def raw(e, c, p=None, n_gangs=None, **over):
    """The C call itself, for arguments the binding would not pass."""
    from ksched import _lib as L
    cl = c.cl
    a = dict(gang_off=c.gang_off, gang_min=c.gang_min, group=c.group, enforce=c.enforce, req_ext=c.req_ext)
    a.update(over)
    arr = {k: None if v is None else np.ascontiguousarray(v, dtype=t) for (k, v), t in
           zip(a.items(), (np.int64, np.int32, np.int32, np.uint8, np.int64))}
    p = cl.n_pods if p is None else p
    oi = np.empty(cl.n_pods, np.int32); os_ = np.empty(cl.n_pods, np.float64); of = np.empty(cl.n_pods, np.int32)
    gp = np.empty(cl.n_pods, np.int32)
    ng = (0 if arr["gang_off"] is None else arr["gang_off"].shape[0] - 1) if n_gangs is None else n_gangs
    return L.lib().ksched_schedule_constrained(
        e._ctx, p, L.ptr(cl.req_cpu, C.c_int64), L.ptr(cl.req_mem, C.c_int64), L.ptr(cl.req_pods, C.c_int64),
        L.ptr(cl.selector, C.c_uint64), ng, L.ptr(arr["gang_off"], C.c_int64), L.ptr(arr["gang_min"], C.c_int32),
        L.ptr(arr["group"], C.c_int32), L.ptr(arr["enforce"], C.c_uint8), L.ptr(arr["req_ext"], C.c_int64),
        L.ptr(oi, C.c_int32), L.ptr(os_, C.c_double), L.ptr(of, C.c_int32), L.ptr(gp, C.c_int32))


def with_(arr, i, v):
    out = np.array(arr)
    out.flat[i] = v
    return out


def test_constrained_invalid_arguments(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    c, _ = case(oracle_mod, 64, 256, domain=1)
    cl, p = c.cl, c.cl.n_pods
    off = GR.cycle_gangs(128)
    h1 = dataclasses.replace(CR.pods(c, 0, 128), gang_off=off)
    w1 = CR.schedule_constrained(oracle_mod, h1)
    h2 = dataclasses.replace(CR.pods(c, 128, 256), gang_off=off, node_ext=w1[4], counts=w1[5])
    w2 = CR.schedule_constrained(oracle_mod, h2, state=w1[6])
    gmin = GR.half_min(c.gang_off)
    with engine(cl) as e:
        for what, kw in (("no spread table", dict(req_ext=None)), ("no ext table", dict(group=None, enforce=None))):
            assert raw(e, c, **kw) == L.E_STATE, what
            assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), cl.node_state()))
        load(e, c)
        CR.same(run(e, h1), *tables(e, c), e.read_nodes(), w1)
        rows, table, counts = e.read_nodes(), e.read_ext(), e.read_spread()
        bad = [("gang_off NULL with n_gangs 1", dict(gang_off=None, n_gangs=1)),
               ("gang_off NULL with n_gangs -1", dict(gang_off=None, n_gangs=-1)),
               ("n_gangs above p", dict(n_gangs=p + 1)), ("n_gangs -1", dict(n_gangs=-1)),
               ("a first offset of 1", dict(gang_off=with_(c.gang_off, 0, 1))),
               ("a last offset short of p", dict(gang_off=with_(c.gang_off, -1, p - 1))),
               ("an offset that repeats", dict(gang_off=with_(c.gang_off, 3, c.gang_off[2]))),
               ("an offset that decreases", dict(gang_off=with_(c.gang_off, 3, c.gang_off[2] - 1))),
               ("an offset above p, then back", dict(gang_off=with_(c.gang_off, 3, 1 << 40))),
               ("a negative offset", dict(gang_off=with_(c.gang_off, 3, -5))),
               ("a minimum of 0", dict(gang_min=with_(gmin, 5, 0))),
               ("a minimum of size + 1", dict(gang_min=with_(gmin, 5, gmin[5] * 2 + 2))),
               ("a spread group of S", dict(group=with_(c.group, 9, 2))),
               ("a spread group of -2", dict(group=with_(c.group, p - 1, -2))),
               ("a request of -1", dict(req_ext=with_(c.req_ext, 7, -1))),
               ("a request of INT64_MIN", dict(req_ext=with_(c.req_ext, 4 * p - 1, -2**63))),
               ("p of -1", dict(p=-1)), ("p of 2^30", dict(p=1 << 30)), ("p of INT64_MAX", dict(p=2**63 - 1))]
        for what, kw in bad:
            assert raw(e, c, **kw) == L.E_INVALID, what
            assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), rows)), what
            assert np.array_equal(e.read_ext(), table) and np.array_equal(e.read_spread(), counts), what
        # a gang above the cap
        big = dataclasses.replace(CR.adversarial(64, 1100, domain=1), gang_off=np.array([0, 1025, 1100]))
        assert raw(e, big) == L.E_INVALID
        assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), rows)) and np.array_equal(e.read_ext(), table)
        for call in (e.explain_batch, lambda: e.explain_pod(0)):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
        # the context still schedules correctly: the second half from where the first left the rows and both tables
        CR.same(run(e, h2), *tables(e, c), e.read_nodes(), w2)
    # opts.nranks > 1: not served, and the rows stay
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0, nranks=2, rank=0,
                nodes_global=2 * cl.n_nodes) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        assert raw(e, c) == L.E_INVALID and raw(e, c, group=None, enforce=None, req_ext=None) == L.E_INVALID
        assert all(np.array_equal(x, y) for x, y in zip(e.read_nodes(), cl.node_state()))


# ---- 12. FakeCluster.schedule_constrained on Kubernetes JSON -----------------------------------------------------------------------
def test_fake_cluster_schedule_constrained(gpu_available):
    from test_constrained_host import kube_json
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, GangRejected
    nl, pl = kube_json()
    fc = FakeCluster.from_kube_json(nl, pl, priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)
    res = fc.schedule_constrained()
    assert [p.name for p, _ in res] == ["p0", "p1", "p2", "p3", "p4", "p5"]
    assert [getattr(r, "name", type(r)) for _, r in res] == ["n0", "n2", "n0", GangRejected, FitError, "n1"]
    assert fc.engine.read_ext().tolist() == [[0, 0, 0]] and fc.engine.read_spread().tolist() == [[2, 1]]
    assert [e["involved"] for e in fc.events if e["reason"] == "FailedScheduling"] == ["p3", "p4"]
    # a second call sees the binds of the first: both tables are rebuilt from the bound pods; job2 still cannot run
    res = fc.schedule_constrained()
    assert [p.name for p, _ in res] == ["p3", "p4"] and isinstance(res[1][1], FitError)
    assert fc.engine.read_ext().tolist() == [[0, 0, 0]] and fc.engine.read_spread().tolist() == [[2, 1]]
    fc.engine.close()
