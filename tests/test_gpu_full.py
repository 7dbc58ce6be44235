"""ksched_schedule_full on the device against the CPU restatement (full_ref: the oracle, gang by gang and pod by pod,
under the numpy eligibility mask, with the snapshot of every table restored for a rejected gang): idx, score bits,
feasible, gang_placed, the final node rows, the extended-resource table, the spread counts and the three affinity
arrays, all exactly, and the stats.  What each case is here for -- a missing undo of the node words, of the zone words or
of the any words would change at least so many pods' results -- is asserted from the reference and its deliberately wrong
variants before the device is touched (test_full_host.conditions; the same cases are checked there without a GPU)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import affinity_ref as AR
import constrained_ref as CR
import full_ref as FR
from test_full_host import case, conditions, family, gpu_cases, kube_json, outside_workgroup_0

pytestmark = pytest.mark.gpu

STAT_KEYS = ("pods", "placed", "batches", "truncations", "pair_evals", "pipeline", "rescues", "exact_rows", "scan_rows")


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def load(e, c, affinity=True):
    if c.group is not None:
        e.load_spread(c.node_domain, c.max_skew, c.counts)
    if c.req_ext is not None:
        e.load_ext(c.node_ext)
    if affinity and c.node_member is not None:
        e.load_affinity(*c.aff_table(), n_domains=c.aff_D)


def run(e, c):
    cl = c.cl
    return e.schedule_full(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.gang_off, c.gang_min, c.group, c.enforce,
                           c.req_ext, *c.aff_pods())


def tables(e, c):
    return ((e.read_ext() if c.req_ext is not None else None), (e.read_spread() if c.group is not None else None),
            (e.read_affinity() if c.member is not None else None))


def check(c, want, **kw):
    with engine(c.cl, **kw) as e:
        load(e, c)
        got = run(e, c)
        st = e.stats()
        FR.same(got, *tables(e, c), e.read_nodes(), want)
    bound = int(want[3].sum()) if c.gang_off is not None else int((want[0] >= 0).sum())
    assert st["pipeline"] == "exact" and st["pods"] == c.cl.n_pods and st["placed"] == bound
    assert st["pair_evals"] == c.cl.n_pods * c.cl.n_nodes


def named(O, name):
    n, p, kw, cond = gpu_cases()[name]
    c, want = case(O, n, p, **kw)
    conditions(O, c, want, **cond)
    return c, want


# ---- 1. the header's worked example, output for output -----------------------------------------------------------------------------
def test_full_worked_example(gpu_available, oracle_mod):
    c = FR.worked_example()
    with engine(c.cl) as e:
        load(e, c)
        idx, score, feas, placed = run(e, c)
        assert idx.tolist() == [-3, -3, -1, 0, 1, 2] and feas.tolist() == [3, 1, 0, 3, 1, 2] and placed.tolist() == [0, 2, 1]
        assert e.read_spread().tolist() == [[2, 1]] and e.read_ext().tolist() == [[0, 0, 1, 0]]
        assert [x.tolist() for x in e.read_affinity()] == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
        assert score.tolist() == [0.0, 0.0, 0.0, float(np.float32(0.1)), float(np.float32(0.2)), float(np.float32(0.3))]
        assert e.read_nodes()[2].tolist() == [109, 109, 109, 110]
        FR.same((idx, score, feas, placed), *tables(e, c), e.read_nodes(), FR.schedule_full(oracle_mod, c))


# ---- 2. families: every instantiation family, all members required and half of them, 12 affinity groups -------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_full_families(priority, domain, labels, half, gpu_available, oracle_mod):
    check(*named(oracle_mod, ("family", priority, domain, labels, half)))


# ---- 3. winners and undone slots in workgroups other than 0, with uneven per_wg; one zone log per workgroup ---------------------
@pytest.mark.parametrize("wgs", [1, 2, 4, 7])
def test_full_workgroups(wgs, gpu_available, oracle_mod):
    c, want = named(oracle_mod, "workgroups")
    if wgs > 1:
        outside_workgroup_0(c, want, wgs)
    check(c, want, exact_wgs=wgs)


# ---- 4. one node, and node counts around the wave size ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
def test_full_node_counts(n, gpu_available, oracle_mod):
    check(*named(oracle_mod, ("nodes", n)))


# ---- 5. several node slots per thread ----------------------------------------------------------------------------------------------
def test_full_two_slots(gpu_available, oracle_mod):
    c, want = named(oracle_mod, "two_slots")
    assert (want[0] >= 256).sum() >= 10  # winners in slot k = 1
    check(c, want, exact_wgs=1)


def test_full_eight_slots(gpu_available, oracle_mod):
    """n = 1100 on one workgroup with labels, four columns and both tables: NPT = 8, the widest instantiation, 46 KB of
    static and 104 KiB of dynamic LDS (the columns, and the affinity words behind them)."""
    c, want = named(oracle_mod, "eight_slots")
    assert (want[0] >= 1024).sum() >= 5 and len({int(w) // 256 for w in want[0] if w >= 0}) >= 4  # several k
    check(c, want, exact_wgs=1)


# ---- 6. the zone table's extremes, and an affinity key that is not the spread key --------------------------------------------------
def test_full_1024_zones(gpu_available, oracle_mod):
    c, want = named(oracle_mod, "zones_1024")
    assert c.aff_D == 1024
    check(c, want)


def test_full_no_zone_key(gpu_available, oracle_mod):
    c, want = named(oracle_mod, "no_zone_key")
    assert c.aff_D == 0 and c.aff_domain is None
    check(c, want)


def test_full_separate_zone_keys(gpu_available, oracle_mod):
    c, want = named(oracle_mod, "other_key")
    assert not np.array_equal(c.node_domain, c.aff_domain) and c.counts.shape[1] == 4 and c.aff_D == 7
    check(c, want)


# ---- 7. the gang cap: one rejected gang undoes several hundred logged members, every slot and zone hit many times ---------------
def test_full_gang_cap_rollback(gpu_available, oracle_mod):
    c, want = named(oracle_mod, "gang_cap")
    rolled = want[0][:1024] == FR.GANG_REJECTED
    assert want[3][0] == 0 and rolled.sum() >= 200 and (rolled & (c.member[:1024] != 0)).sum() >= 100
    assert want[7]["rewaived"] >= 1, want[7]
    check(c, want)


# ---- 8. equivalences on the device, output for output and state for state --------------------------------------------------------
def identical(a, b):
    """a, b: (results, rows, stats, tables...) of two engines."""
    assert len(a[0]) == len(b[0]) and len(a) == len(b)
    flat = lambda r: list(r[0]) + list(r[1]) + [x for t in r[3:] for x in (t if isinstance(t, tuple) else (t,))]
    for x, y in zip(flat(a), flat(b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                                     y.view(np.int64) if y.dtype == np.float64 else y)
    for k in STAT_KEYS:
        assert a[2][k] == b[2][k], k
    assert (a[0][0] >= 0).any() and (a[0][0] < 0).any()


@pytest.mark.parametrize("half", [False, True])
def test_full_affinity_off_is_schedule_constrained(half, gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, **family(0, 1, False, half))
    cl = c.cl
    out = []
    for full in (False, True):
        with engine(cl) as e:
            load(e, c)  # (the affinity table too: with affinity off it is neither read nor moved)
            call = e.schedule_full if full else e.schedule_constrained
            got = call(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.gang_off, c.gang_min, c.group, c.enforce, c.req_ext)
            out.append((got, e.read_nodes(), e.stats(), e.read_ext(), e.read_spread(), e.read_affinity()))
    identical(*out)
    assert (out[1][0][0] == FR.GANG_REJECTED).any()
    assert all(np.array_equal(x, y) for x, y in zip(out[1][5], c.aff_table()[1:]))


@pytest.mark.parametrize("D_aff", [3, 0])
def test_full_affinity_alone_is_schedule_affinity(D_aff, gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, domain=1, D_aff=D_aff)
    cl = c.cl
    out = []
    for full in (False, True):
        with engine(cl) as e:
            load(e, c)  # (spread and ext too: neither read nor moved)
            if full:
                got = e.schedule_full(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, None, None, None, None, None,
                                      *c.aff_pods())
                assert got[3].shape == (0,)
                got = got[:3]
            else:
                got = e.schedule_affinity(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, *c.aff_pods())
            out.append((got, e.read_nodes(), e.stats(), e.read_ext(), e.read_spread(), e.read_affinity()))
    identical(*out)
    assert np.array_equal(out[1][3], c.node_ext) and np.array_equal(out[1][4], c.counts)
    assert any((x != y).any() for x, y in zip(out[1][5], c.aff_table()[1:]))


@pytest.mark.parametrize("priority", [0, 1])
def test_full_all_off_is_schedule(priority, gpu_available, oracle_mod):
    c, _ = case(oracle_mod, 64, 256, priority=priority, domain=1)
    cl = c.cl
    out = []
    for full in (False, True):
        with engine(cl) as e:
            load(e, c)
            got = e.schedule_full(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)[:3] if full else \
                e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
            out.append((got, e.read_nodes(), e.stats(), e.read_ext(), e.read_spread(), e.read_affinity()))
    identical(*out)
    assert np.array_equal(out[1][0][0], oracle_mod.schedule(cl)[0])
    assert np.array_equal(out[1][3], c.node_ext) and np.array_equal(out[1][4], c.counts)
    assert all(np.array_equal(x, y) for x, y in zip(out[1][5], c.aff_table()[1:]))


# ---- 9. carry-over: the second call starts from the words the first call's rejected gang gave back -------------------------------
def split(c, g):
    """Case c as two calls, the first ending with gang g."""
    off = np.asarray(c.gang_off, np.int64)
    cut, p = int(off[g + 1]), c.cl.n_pods
    gm = (None, None) if c.gang_min is None else (c.gang_min[:g + 1], c.gang_min[g + 1:])
    return (dataclasses.replace(FR.pods(c, 0, cut), gang_off=off[:g + 2], gang_min=gm[0]),
            dataclasses.replace(FR.pods(c, cut, p), gang_off=off[g + 1:] - cut, gang_min=gm[1])), cut


def two_calls(c, want, g):
    (h1, h2), cut = split(c, g)
    ng1 = g + 1
    with engine(c.cl) as e:
        load(e, c)
        a = run(e, h1)
        mid = e.read_affinity()
        b = run(e, h2)  # (without reloading: from the first call's tables, zone and any words)
        got = tuple(np.concatenate(x) for x in zip(a, b))
        assert a[3].shape == (ng1,) and np.array_equal(a[0], want[0][:cut])
        FR.same(got, *tables(e, c), e.read_nodes(), want)
    return mid


def test_full_two_calls_worked_example(gpu_available, oracle_mod):
    """The first call is the rejected gang alone: it leaves every word as loaded, and the second call's p3 is waived again
    -- which needs the context's any_zone restored -- and finds zone A's words empty."""
    c = FR.worked_example()
    mid = two_calls(c, FR.schedule_full(oracle_mod, c), 0)
    assert not any(x.any() for x in mid)


def test_full_two_calls(gpu_available, oracle_mod):
    c, want = named(oracle_mod, "workgroups")
    off = np.asarray(c.gang_off)
    # the first call ends in a rejected gang that had placed members with affinity words, near the middle of the pods
    gangs = [g for g in range(len(off) - 1) if want[3][g] == 0 and
             ((want[0][off[g]:off[g + 1]] == FR.GANG_REJECTED) & (c.member[off[g]:off[g + 1]] != 0)).any()]
    g = min(gangs, key=lambda g: abs(int(off[g + 1]) - 128))
    assert 64 <= off[g + 1] <= 192
    two_calls(c, want, g)


# ---- 10. errors leave everything alone ---------------------------------------------------------------------------------------------
def raw(e, c, **over):
    """The C call itself, for arguments the binding would not pass."""
    from ksched import _lib as L
    cl = c.cl
    a = dict(gang_off=c.gang_off, gang_min=c.gang_min, group=c.group, enforce=c.enforce, req_ext=c.req_ext, member=c.member,
             anti_host=c.anti_host, anti_zone=c.anti_zone, aff_group=c.aff_group, aff_zone=c.aff_zone)
    a.update(over)
    types = dict(gang_off=np.int64, gang_min=np.int32, group=np.int32, enforce=np.uint8, req_ext=np.int64, member=np.uint64,
                 anti_host=np.uint64, anti_zone=np.uint64, aff_group=np.int32, aff_zone=np.uint8)
    arr = {k: None if v is None else np.ascontiguousarray(v, dtype=types[k]) for k, v in a.items()}
    ct = {np.int64: C.c_int64, np.int32: C.c_int32, np.uint8: C.c_uint8, np.uint64: C.c_uint64}
    p = cl.n_pods
    oi = np.empty(p, np.int32); os_ = np.empty(p, np.float64); of = np.empty(p, np.int32); gp = np.empty(p, np.int32)
    ng = 0 if arr["gang_off"] is None else arr["gang_off"].shape[0] - 1
    return L.lib().ksched_schedule_full(
        e._ctx, p, L.ptr(cl.req_cpu, C.c_int64), L.ptr(cl.req_mem, C.c_int64), L.ptr(cl.req_pods, C.c_int64),
        L.ptr(cl.selector, C.c_uint64), ng, *(L.ptr(arr[k], ct[types[k]]) for k in types),
        L.ptr(oi, C.c_int32), L.ptr(os_, C.c_double), L.ptr(of, C.c_int32), L.ptr(gp, C.c_int32))


def with_(arr, i, v):
    out = np.array(arr)
    out.flat[i] = v
    return out


def test_full_errors_leave_everything_alone(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    c, want = named(oracle_mod, "workgroups")
    cl = c.cl
    rows_equal = lambda xs, ys: all(np.array_equal(x, y) for x, y in zip(xs, ys))
    only_word = {k: None for k in ("member", "anti_host", "anti_zone", "aff_group", "aff_zone")}
    with engine(cl) as e:
        load(e, c, affinity=False)
        # affinity on -- by any one of its five pointers -- without a loaded table
        for k in only_word:
            assert raw(e, c, **dict(only_word, **{k: getattr(c, k)})) == L.E_STATE, k
            assert rows_equal(e.read_nodes(), cl.node_state())
            assert np.array_equal(e.read_ext(), c.node_ext) and np.array_equal(e.read_spread(), c.counts)
        with pytest.raises(KschedError) as ei:
            e.read_affinity()
        assert ei.value.code == L.E_STATE
        load(e, c)
        bad = [("an affinity group of 64", dict(aff_group=with_(c.aff_group, 5, 64))),
               ("an affinity group of -2", dict(aff_group=with_(c.aff_group, 255, -2))),
               ("a spread group of S", dict(group=with_(c.group, 9, 2))),
               ("a request of -1", dict(req_ext=with_(c.req_ext, 7, -1))),
               ("an offset that repeats", dict(gang_off=with_(c.gang_off, 3, c.gang_off[2])))]
        for what, kw in bad:
            assert raw(e, c, **kw) == L.E_INVALID, what
            assert rows_equal(e.read_nodes(), cl.node_state()), what
            assert np.array_equal(e.read_ext(), c.node_ext) and np.array_equal(e.read_spread(), c.counts), what
            assert rows_equal(e.read_affinity(), c.aff_table()[1:]), what
        # the context still schedules correctly, and the explain calls know none of the reasons
        FR.same(run(e, c), *tables(e, c), e.read_nodes(), want)
        for call in (e.explain_batch, lambda: e.explain_pod(0)):
            with pytest.raises(KschedError) as ei:
                call()
            assert ei.value.code == L.E_STATE
    # opts.nranks > 1: not served, and the rows stay
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0, nranks=2, rank=0,
                nodes_global=2 * cl.n_nodes) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        assert raw(e, c) == L.E_INVALID and raw(e, c, group=None, enforce=None, req_ext=None, **only_word) == L.E_INVALID
        assert rows_equal(e.read_nodes(), cl.node_state())


# ---- 11. FakeCluster.schedule_full on Kubernetes JSON ------------------------------------------------------------------------------
def test_fake_cluster_schedule_full(gpu_available):
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, GangRejected
    nl, pl = kube_json()
    fc = FakeCluster.from_kube_json(nl, pl, priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)
    res = fc.schedule_full()
    assert [p.name for p, _ in res] == ["p0", "p1", "p2", "p3", "p4", "p5"]
    assert [getattr(r, "name", type(r)) for _, r in res] == [GangRejected, GangRejected, FitError, "n0", "n1", "n2"]
    assert fc.engine.read_ext().tolist() == [[0, 0, 1, 0]] and fc.engine.read_spread().tolist() == [[2, 1]]
    assert [x.tolist() for x in fc.engine.read_affinity()] == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
    assert [e["involved"] for e in fc.events if e["reason"] == "FailedScheduling"] == ["p0", "p1", "p2"]
    # a second call sees the binds of the first: the tables are rebuilt from the bound pods, and job1 -- no longer the
    # first of its group, with zone A's hosts taken -- fits nowhere
    res = fc.schedule_full()
    assert [p.name for p, _ in res] == ["p0", "p1", "p2"] and all(isinstance(r, FitError) for _, r in res)
    assert fc.engine.read_ext().tolist() == [[0, 0, 1, 0]]
    assert [x.tolist() for x in fc.engine.read_affinity()] == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
    fc.engine.close()
