"""ksched_preempt_constrained on the device: every output column equal to the plain-Python restatement
(preempt_constrained_ref), over the table's block, span, tile and chunk edges, the columns' edges, directed cases for
each constraint alone, and the call's promises: byte-equal to ksched_preempt with both constraints off, consistent with
ksched_explain_full, victims that do make room under the constraints, and a dry run."""
import dataclasses
import os
import re

import numpy as np
import pytest

import preempt_constrained_ref as PC
import preempt_ref as PR
from conftest import PKG

pytestmark = pytest.mark.gpu

T = 4  # the scan kernel's pod tile, kPreemptCTile (test_tile_constant pins it to the header)
CASES = {1: (1, 129, 48), 2: (2, 211, 96), 3: (3, 65, 24)}
_REF = {}


def case(seed):
    """A generator case and its reference answer at vcap = 1024, computed once, never modified."""
    if seed not in _REF:
        c = PC.gen(*CASES[seed])
        _REF[seed] = (c, PC.preempt(c, 1024))
    return _REF[seed]


def cut(want, vcap):
    return want[:5] + (np.ascontiguousarray(want[5][:, :vcap]),)


def engine(c, labels=None, bound="constrained", spread=True, ext=True):
    """An engine holding c's nodes, its spread and ext tables and its bound-pod table."""
    from ksched import MODE_EXACT, Engine
    e = Engine(mode=MODE_EXACT, device=0, use_labels=labels is not None)
    e.load_nodes(*c.alloc, labels=labels)
    if spread:
        e.load_spread(c.node_domain, c.skew, c.counts)
    if ext:
        e.load_ext(c.node_ext)
    if bound == "constrained":
        e.load_bound_constrained(*c.bound, c.bound_ext, c.bound_spread)
    elif bound == "plain":
        e.load_bound(*c.bound)
    return e


def run(e, c, vcap, spread=True, ext=True, selector=None, prio=None, m=None):
    m = c.m if m is None else m
    return e.preempt_constrained(*(p[:m] for p in c.pods[:3]), None if selector is None else selector[:m],
                                 (c.pods[3] if prio is None else prio)[:m], c.group[:m] if spread else None,
                                 c.enforce[:m] if spread else None, c.req_ext[:, :m] if ext else None, vcap=vcap)


def plain(e, c, vcap, selector=None):
    return e.preempt(*c.pods[:3], selector, c.pods[3], vcap=vcap)


def test_tile_constant():
    txt = open(os.path.join(PKG, "csrc", "ksched_preemptc.h")).read()
    assert int(re.search(r"constexpr int kPreemptCTile = (\d+);", txt).group(1)) == T


# ---- 1. parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_parity(seed, gpu_available):
    c, want = case(seed)
    nofit, novictim, multi = PR.classes(want)
    assert nofit >= 1 and novictim >= 1 and multi >= 1  # every class of answer occurs
    assert want[1].max() > 4  # vcap 1 and 4 do truncate
    assert want[1].max() == {1: 15, 2: 19, 3: 24}[seed]
    no_spread, no_ext = PC.preempt(c, 1024, spread=False), PC.preempt(c, 1024, ext=False)
    assert PC.changed(want, no_spread) >= 11 and PC.changed(want, no_ext) >= 11  # each constraint decides some pod's row
    with engine(c) as e:
        for vcap in (1, 4, 64, 1024):
            got = run(e, c, vcap)
            PR.same(got, cut(want, vcap))
            assert np.array_equal(got[1], want[1])  # the count is the full one at every vcap
        # ---- 2. one constraint at a time
        PR.same(run(e, c, 1024, spread=False), no_spread)
        PR.same(run(e, c, 1024, ext=False), no_ext)


def test_parity_balanced_counts(gpu_available):
    """Counts above the table's own (pods the table does not hold), all rows near their maximum: the skew binds."""
    c = PC.gen(3, 65, 24, balanced=True)
    want = PC.preempt(c, 64)
    assert PC.changed(want, PC.preempt(c, 64, spread=False)) >= 1
    with engine(c) as e:
        PR.same(run(e, c, 64), want)


def test_parity_labels(gpu_available):
    c, base = case(3)
    labels, selector = PR.labels_for(7, c.n, c.m)
    want = PC.preempt(c, 64, labels=labels, selector=selector)
    assert not np.array_equal(want[4], base[4])  # the label check removes candidates
    with engine(c, labels=labels) as e:
        PR.same(run(e, c, 64, selector=selector), want)
        PR.same(run(e, c, 64, selector=selector, spread=False, ext=False), plain(e, c, 64, selector))


# ---- 3. constraints off ----------------------------------------------------------------------------------------------
def test_constraints_off_is_preempt(gpu_available):
    c, _ = case(2)
    with engine(c) as e, engine(c, bound="plain", spread=False, ext=False) as p:
        ref = plain(p, c, 64)
        assert (ref[0] == PR.NO_FIT).any() and (ref[1] > 1).any()
        for got in (run(e, c, 64, spread=False, ext=False), run(p, c, 64, spread=False, ext=False), plain(e, c, 64)):
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, ref))
        # a table from load_bound is the table without columns and masks: spread reads zeros, ext is refused
        p.load_spread(c.node_domain, c.skew, c.counts)
        zero = dataclasses.replace(c, bound_spread=np.zeros_like(c.bound_spread))
        PR.same(run(p, c, 64, ext=False), PC.preempt(zero, 64, ext=False))


# ---- 4. shape edges --------------------------------------------------------------------------------------------------
def first_nodes(c, n):
    """The first n nodes of a case with the bound pods they hold (D = 5 ids sit on the first five nodes)."""
    keep = c.bound[0] < n
    dom = c.node_domain[:n]
    D = int(dom.max()) + 1
    return PC.Case(tuple(a[:n] for a in c.alloc), tuple(b[keep] for b in c.bound), c.pods, c.node_ext[:, :n],
                   c.bound_ext[:, keep], c.req_ext, dom, c.skew, c.counts[:, :D], c.bound_spread[keep], c.group, c.enforce)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_n(n, gpu_available):
    c = PC.head(first_nodes(case(1)[0], n), 24)
    with engine(c) as e:
        PR.same(run(e, c, 16), PC.preempt(c, 16))


def test_many_spans(gpu_available):
    """3000 nodes and one tile of pods: three spans of 1024 rows, the winners in the later spans."""
    c = PC.gen(5, 3000, 8, maxseg=10)
    c.alloc[0][:1100] = 0  # no cpu left on the low nodes
    want = PC.preempt(c, 16)
    assert (want[0] >= 2048).any() and ((want[0] >= 1024) & (want[0] < 2048)).any() and (want[1] > 1).any()
    with engine(c) as e:
        PR.same(run(e, c, 16), want)


def test_pod_tiles(gpu_available):
    c, want = case(3)
    with engine(c) as e:
        for m in (1, T - 1, T, T + 1):
            PR.same(run(e, c, 64, m=m), tuple(w[:m] for w in cut(want, 64)))


def test_chunks(gpu_available):
    """1024 + 5 pods on 20 nodes: the second pair of launches reuses the workspace for a short tail."""
    c = PC.gen(4, 20, 1024 + 5, maxseg=10)
    with engine(c) as e:
        PR.same(run(e, c, 3), PC.preempt(c, 3))


# ---- 5. column edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4])
def test_ext_columns(R, gpu_available):
    from ksched import _lib as L
    assert L.EXT_MAX == 4
    c = PC.gen(6, 65, 24, R=R)
    want = PC.preempt(c, 64)
    assert PC.changed(want, PC.preempt(c, 64, ext=False)) >= 1
    with engine(c) as e:
        PR.same(run(e, c, 64), want)


def test_group_63(gpu_available):
    """S = 64 with group 63 in use: bit 63 of the mask."""
    c = PC.gen(7, 65, 24, S=64, balanced=True)
    c.group[::2] = 63
    c.enforce[::2] = 1
    want = PC.preempt(c, 64)
    only62 = dataclasses.replace(c, bound_spread=c.bound_spread & np.uint64((1 << 63) - 1))
    assert PC.changed(want, PC.preempt(only62, 64)) >= 1  # bit 63 decides some row
    with engine(c) as e:
        PR.same(run(e, c, 64), want)


def test_one_domain(gpu_available):
    """D = 1: there is no other domain, the spread clause passes wherever the key is present."""
    c = PC.gen(8, 65, 24, D=1, nokey=0.3)
    want, off = PC.preempt(c, 64, detail=True), PC.preempt(c, 64, spread=False, detail=True)
    keyed = c.node_domain >= 0
    enforcing = (c.group >= 0) & (c.enforce != 0)
    assert enforcing.any() and not keyed.all()
    assert np.array_equal(want[6][:, keyed], off[6][:, keyed]) and not want[6][enforcing][:, ~keyed].any()
    with engine(c) as e:
        PR.same(run(e, c, 64), want[:6])


def test_1024_domains(gpu_available):
    c = PC.gen(13, 1100, 6, D=1024, S=4, maxseg=4, nokey=0.02)
    assert c.counts.shape == (4, 1024)
    want = PC.preempt(c, 16)
    assert PC.changed(want, PC.preempt(c, 16, spread=False)) >= 1
    with engine(c) as e:
        PR.same(run(e, c, 16), want)


def test_full_segment(gpu_available):
    """One node with exactly KSCHED_BOUND_MAX_PER_NODE pods, every one holding an amount; one more is refused."""
    from ksched import KschedError
    from ksched import _lib as L
    r = np.random.default_rng(11)
    n, nb = 67, L.BOUND_MAX_PER_NODE
    alloc = (np.zeros(n, np.int64), np.full(n, 1 << 20), np.full(n, 4))
    bound = (np.full(nb, 65, np.int32), np.ones(nb, np.int64), np.zeros(nb, np.int64), r.integers(-2, 6, nb).astype(np.int32) * 100)
    pods = (np.array([1, 1, 1]), np.zeros(3, np.int64), np.ones(3, np.int64), np.array([1000, 1000, 1000], np.int32))
    c = PC.Case(alloc, bound, pods, node_ext=np.zeros((1, n), np.int64), bound_ext=np.ones((1, nb), np.int64),
                req_ext=np.array([[700, 1024, 1025]], np.int64), node_domain=np.zeros(n, np.int32), skew=np.ones(1, np.int32),
                counts=np.array([[nb]], np.int32), bound_spread=np.ones(nb, np.uint64), group=np.full(3, -1, np.int32),
                enforce=np.ones(3, np.uint8))
    want = PC.preempt(c, 1024)
    assert want[0].tolist() == [65, 65, PR.NO_FIT] and want[1].tolist() == [700, 1024, 0]
    with engine(c) as e:
        PR.same(run(e, c, 1024), want)
        PR.same(run(e, c, 4), cut(want, 4))
        with pytest.raises(KschedError) as ei:
            e.load_bound_constrained(*(np.concatenate([b, b[:1]]) for b in bound), np.ones((1, nb + 1), np.int64), None)
        assert ei.value.code == L.E_INVALID and "load_bound_constrained" in str(ei.value)
        PR.same(run(e, c, 4), cut(want, 4))  # the refused table left the loaded one in place


# ---- 6. directed, spread alone ---------------------------------------------------------------------------------------
def test_directed_spread(gpu_available):
    alloc = (np.array([100, 100, 0, 0]), np.full(4, 1 << 20), np.full(4, 10))
    bound = (np.array([0, 0, 0, 0, 1, 1, 1], np.int32), np.ones(7, np.int64), np.zeros(7, np.int64),
             np.array([10, 20, 30, 40, 5, 6, 7], np.int32))
    pods = (np.array([1, 1]), np.zeros(2, np.int64), np.ones(2, np.int64), np.array([100, 35], np.int32))
    c = PC.Case(alloc, bound, pods, node_ext=np.zeros((1, 4), np.int64), bound_ext=np.zeros((1, 7), np.int64),
                req_ext=np.zeros((1, 2), np.int64), node_domain=np.array([0, 0, 1, 1], np.int32), skew=np.ones(1, np.int32),
                counts=np.array([[5, 3]], np.int32), bound_spread=np.array([1, 1, 0, 1, 1, 1, 1], np.uint64),
                group=np.zeros(2, np.int32), enforce=np.ones(2, np.uint8))
    want = PC.preempt(c, 4, ext=False)
    assert want[0].tolist() == [1, 1] and want[1].tolist() == [2, 2] and want[2].tolist() == [6, 6]
    assert want[4].tolist() == [2, 2] and want[5].tolist() == [[5, 4, -1, -1]] * 2
    with engine(c) as e:
        PR.same(run(e, c, 4, ext=False), want)
        node, nv = plain(e, c, 4)[:2]
        assert node.tolist() == [0, 0] and nv.tolist() == [0, 0]


# ---- 7. directed, ext alone: the header's worked example -------------------------------------------------------------
def test_worked_example(gpu_available):
    c = PC.worked_example()
    with engine(c) as e:
        got = run(e, c, 2)
        for name, g in zip(("node", "nvictims", "max_prio", "sum_prio", "candidates", "victims"), got):
            assert g.tolist() == PC.WORKED[name], name
        p = plain(e, c, 2)
        assert p[0].tolist() == [0, -1, 0, 0] and p[4].tolist() == [3, 0, 3, 3] and p[5].tolist()[0] == [1, -1]
        # a zero request checks nothing: a negative column does not bar the node
        neg = dataclasses.replace(c, node_ext=np.array([[-5, -5, -5]], np.int64))
        e.load_ext(neg.node_ext)
        want = PC.preempt(neg, 2)
        assert want[0].tolist() == [-1, -1, 1, 0] and want[4].tolist() == [0, 0, 3, 3]
        PR.same(run(e, neg, 2), want)


# ---- 8. nodes without the key ----------------------------------------------------------------------------------------
def test_nodes_without_the_key(gpu_available):
    c = PC.gen(10, 65, 24, nokey=0.5)
    c.group[:] = 0
    c.enforce[:12] = 1
    c.enforce[12:] = 0
    want, off = PC.preempt(c, 16, detail=True), PC.preempt(c, 16, spread=False, detail=True)
    nokey = c.node_domain < 0
    assert nokey.sum() >= 10 and off[6][:12][:, nokey].any()
    assert not want[6][:12][:, nokey].any()               # never a candidate for an enforcing pod
    assert np.array_equal(want[6][12:], off[6][12:])      # a pod that only counts reads no count and no key
    with engine(c) as e:
        got = run(e, c, 16)
        PR.same(got, want[:6])
        assert not nokey[got[0][:12][got[0][:12] >= 0]].any()


# ---- 9. against ksched_explain_full ------------------------------------------------------------------------------------
def test_nobody_may_go_is_explain_full(gpu_available):
    c, _ = case(1)
    low = np.full(c.m, c.bound[3].min(), np.int32)
    with engine(c) as e:
        node, nv, mx, _, cand, _ = run(e, c, 8, prio=low)
        assert not nv.any() and (mx == PR.NO_VICTIM_PRIO).all() and (node >= 0).any() and (node < 0).any()
        for i in range(c.m):
            counts, codes = e.explain_full(int(c.pods[0][i]), int(c.pods[1][i]), int(c.pods[2][i]), 0, int(c.group[i]),
                                           bool(c.enforce[i]), c.req_ext[:, i])
            fit = np.flatnonzero(codes == 0)
            assert cand[i] == counts[0] == len(fit) and node[i] == (fit[0] if len(fit) else PR.NO_FIT), i


# ---- 10. closing the loop ----------------------------------------------------------------------------------------------
def test_victims_make_room(gpu_available):
    """With the victims' amounts returned and their counts taken off the pod is eligible on the chosen node
    (ksched_explain_full); with the last of them left in place it is not."""
    c, want = case(1)
    node, nv, _, _, _, vic = want
    S = len(c.skew)

    def removed(e, j, vs):
        e.apply_delta([j], [c.bound[1][vs].sum()], [c.bound[2][vs].sum()], [len(vs)])
        ext = c.node_ext.copy()
        ext[:, j] += c.bound_ext[:, vs].sum(axis=1)
        e.load_ext(ext)
        counts = c.counts.copy()
        d = c.node_domain[j]
        if d >= 0:
            for s in range(S):
                counts[s, d] -= int(((c.bound_spread[vs] >> np.uint64(s)) & np.uint64(1)).sum())
        e.load_spread(c.node_domain, c.skew, counts)

    with engine(c) as e:
        PR.same(run(e, c, 1024), want)
        checked = 0
        for i in np.flatnonzero(nv > 0):
            j, vs = int(node[i]), vic[i, :nv[i]]
            args = (int(c.pods[0][i]), int(c.pods[1][i]), int(c.pods[2][i]), 0, int(c.group[i]), bool(c.enforce[i]), c.req_ext[:, i])
            removed(e, j, vs)
            assert e.explain_full(*args)[1][j] == 0, i
            e.apply_delta([j], [-c.bound[1][vs].sum()], [-c.bound[2][vs].sum()], [-len(vs)])
            removed(e, j, vs[:-1])
            assert e.explain_full(*args)[1][j] != 0, i
            e.apply_delta([j], [-c.bound[1][vs[:-1]].sum()], [-c.bound[2][vs[:-1]].sum()], [-(len(vs) - 1)])
            checked += 1
        assert checked >= 20
        assert all(np.array_equal(a, b) for a, b in zip(c.alloc, e.read_nodes()))


# ---- 11. a dry run -----------------------------------------------------------------------------------------------------
def test_commits_nothing(gpu_available):
    c, want = case(3)
    gang = np.arange(c.m + 1, dtype=np.int64)
    with engine(c) as e, engine(c, bound=None) as fresh:
        first = e.schedule(*c.pods[:3])
        fresh.schedule(*c.pods[:3])
        before = (e.read_nodes(), e.read_ext(), e.read_spread(), e.explain_batch())
        after_schedule = dataclasses.replace(c, alloc=before[0])
        PR.same(run(e, c, 1024), PC.preempt(after_schedule, 1024))
        after = (e.read_nodes(), e.read_ext(), e.read_spread(), e.explain_batch())
        assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])), "preempt_constrained changed a node row"
        assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
        assert before[3][1] == after[3][1] and np.array_equal(before[3][0], after[3][0])
        assert all(np.array_equal(a, b) for a, b in zip(first, e.results()))
        a = e.schedule_constrained(*c.pods[:3], None, gang, None, c.group, c.enforce, c.req_ext)
        b = fresh.schedule_constrained(*c.pods[:3], None, gang, None, c.group, c.enforce, c.req_ext)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        assert np.array_equal(e.read_ext(), fresh.read_ext()) and np.array_equal(e.read_spread(), fresh.read_spread())


# ---- 12. state and errors ----------------------------------------------------------------------------------------------
def test_state_and_errors(gpu_available):
    import ctypes as C
    from ksched import MODE_EXACT, Engine, KschedError
    from ksched import _lib as L
    c, want = case(3)

    def code(fn):
        with pytest.raises(KschedError) as ei:
            fn()
        return ei.value.code

    def raw_load(e, n_ext, bound_ext, bound_spread):
        ix, bc, bm, bp = (np.ascontiguousarray(a, t) for a, t in zip(c.bound, (np.int32, np.int64, np.int64, np.int32)))
        return L.lib().ksched_load_bound_constrained(e._ctx, len(ix), L.ptr(ix, C.c_int32), L.ptr(bc, C.c_int64),
                                                     L.ptr(bm, C.c_int64), L.ptr(bp, C.c_int32), n_ext,
                                                     L.ptr(bound_ext, C.c_int64), L.ptr(bound_spread, C.c_uint64))

    with Engine(mode=MODE_EXACT, device=0) as e:
        assert code(lambda: e.load_bound_constrained(*c.bound, c.bound_ext, c.bound_spread)) == L.E_STATE  # before load_nodes
        assert code(lambda: run(e, c, 0)) == L.E_INVALID   # the argument rules come before the state
        assert code(lambda: run(e, c, 4)) == L.E_STATE
        e.load_nodes(*c.alloc)
        assert code(lambda: run(e, c, 4, spread=False, ext=False)) == L.E_STATE  # no bound-pod table
        # the load's own cases
        be = np.ascontiguousarray(c.bound_ext)
        assert raw_load(e, -1, be, None) == L.E_INVALID and raw_load(e, L.EXT_MAX + 1, be, None) == L.E_INVALID
        assert raw_load(e, 2, None, None) == L.E_INVALID and raw_load(e, 0, be, None) == L.E_INVALID
        neg = c.bound_ext.copy()
        neg[1, 5] = -1
        assert code(lambda: e.load_bound_constrained(*c.bound, neg, c.bound_spread)) == L.E_INVALID
        for bad in (-1, c.n):
            nodes = c.bound[0].copy()
            nodes[3] = bad
            assert code(lambda: e.load_bound_constrained(nodes, *c.bound[1:], c.bound_ext, c.bound_spread)) == L.E_INVALID
        assert code(lambda: run(e, c, 4, spread=False, ext=False)) == L.E_STATE  # a refused load loads nothing
        e.load_bound_constrained(*c.bound, c.bound_ext, c.bound_spread)
        PR.same(run(e, c, 64, spread=False, ext=False), PC.preempt(c, 64, spread=False, ext=False))
        # a constraint on without its table
        assert code(lambda: run(e, c, 4, ext=False)) == L.E_STATE and code(lambda: run(e, c, 4, spread=False)) == L.E_STATE
        e.load_spread(c.node_domain, c.skew, c.counts)
        e.load_ext(c.node_ext)
        PR.same(run(e, c, 64), cut(want, 64))
        # the call's argument rules
        for vcap in (0, L.BOUND_MAX_PER_NODE + 1):
            assert code(lambda: run(e, c, vcap)) == L.E_INVALID
        for bad in (-2, len(c.skew)):
            g = c.group.copy()
            g[1] = bad
            assert code(lambda: e.preempt_constrained(*c.pods[:3], None, c.pods[3], g, c.enforce, c.req_ext, vcap=4)) == L.E_INVALID
        rq = c.req_ext.copy()
        rq[0, 2] = -1
        assert code(lambda: e.preempt_constrained(*c.pods[:3], None, c.pods[3], c.group, c.enforce, rq, vcap=4)) == L.E_INVALID
        assert run(e, c, 4, m=0)[5].shape == (0, 4)
        # the bound table's n_ext is not the ext table's; a mask names a group the spread table does not hold
        e.load_bound_constrained(*c.bound, c.bound_ext[:1], c.bound_spread)
        assert code(lambda: run(e, c, 4)) == L.E_STATE
        PR.same(run(e, c, 64, ext=False), PC.preempt(c, 64, ext=False))
        e.load_bound(*c.bound)
        assert code(lambda: run(e, c, 4, spread=False)) == L.E_STATE  # (a load_bound table has n_ext 0)
        e.load_bound_constrained(*c.bound, c.bound_ext, c.bound_spread | np.uint64(1 << len(c.skew)))
        assert code(lambda: run(e, c, 4)) == L.E_STATE
        PR.same(run(e, c, 64, spread=False), PC.preempt(c, 64, spread=False))  # the refused call left every table usable
        e.load_bound_constrained(*c.bound, c.bound_ext, c.bound_spread)
        PR.same(run(e, c, 64), cut(want, 64))
        e.load_nodes(*c.alloc)  # a second load_nodes invalidates the table
        assert code(lambda: run(e, c, 4, spread=False, ext=False)) == L.E_STATE


# ---- 13. FakeCluster ---------------------------------------------------------------------------------------------------
def test_fake_cluster_preempt_pod_constrained(gpu_available):
    """The worked example as kube JSON: amd.com/gpu in capacity and requests, one topologySpreadConstraints entry.  The
    example's counted pod outside the table is bound-6 on node-2: a table pod above every preemptor's priority."""
    import kube_json
    from ksched import DOMAIN_FEASIBLE, MODE_EXACT, cluster
    from ksched.host import FakeCluster, FitError
    GPU, ZONE = "amd.com/gpu", "topology.kubernetes.io/zone"
    z = np.zeros(0, np.int64)
    cl = cluster.Cluster(name="hand", alloc_cpu=z, alloc_mem=z, alloc_pods=z, req_cpu=z, req_mem=z, req_pods=z)
    cl.node_names = ["node-0", "node-1", "node-2"]
    # capacity = what is free in the example plus what the node's bound pods hold
    cl.node_capacity = [dict(cpu=cpu, memory="1048576Ki", pods="12", **{GPU: g}) for cpu, g in (("1500m", "2"), ("1000m", "1"), ("1600m", "2"))]
    bound = ((2, "500m", 1, True), (0, "600m", 1, False), (1, "500m", 0, True), (0, "500m", 1, True), (1, "500m", 1, True), (2, "600m", 0, False),
             (2, "100m", 0, True))
    cl.bound_pods = [(f"node-{j}", [dict(cpu=cpu, **({GPU: str(g)} if g else {}))]) for j, cpu, g, _ in bound]
    cl.pending_pods = [[dict(cpu="1000m", **{GPU: "2"})], [dict(cpu="400m")]]
    nl, pl = kube_json.to_kube(cl)
    for item, zone in zip(nl["items"], "ABA"):
        item["metadata"]["labels"] = {ZONE: zone}
    for item, prio in zip(pl["items"], (100, 200, 200, 100, 50, 200, 2000, 1000, 1000)):
        item["spec"]["priority"] = prio
    for item, (_, _, _, grouped) in zip(pl["items"], bound):
        if grouped:
            item["metadata"]["labels"] = {"job": "x"}
    pl["items"][8]["spec"]["topologySpreadConstraints"] = [dict(maxSkew=1, topologyKey=ZONE, whenUnsatisfiable="DoNotSchedule",
                                                                 labelSelector=dict(matchLabels={"job": "x"}))]
    fc = FakeCluster.from_kube_json(nl, pl, domain=DOMAIN_FEASIBLE, mode=MODE_EXACT, device=0)
    a, cpod = fc.unscheduled_pods()
    node, victims = fc.preempt_pod(a)
    assert node.name == "node-0" and [v.name for v in victims] == ["bound-1"]  # one gpu short
    node, victims = fc.preempt_pod_constrained(a)
    assert node.name == "node-0" and [v.name for v in victims] == ["bound-1", "bound-3"]
    assert len(fc.pods) == 9 and not fc.events and not a.node_name  # a dry run
    assert fc.preempt_pod(cpod)[1] == []  # pod C of the example: it fits on node-0 as things stand, but for the skew
    node, victims = fc.preempt_pod_constrained(cpod)
    assert node.name == "node-1" and [v.name for v in victims] == ["bound-4"]
    out = fc.schedule_constrained([a])
    assert isinstance(out[0][1], FitError)
    node, victims = fc.preempt_pod_constrained(a, evict=True)
    assert node.name == "node-0" and [v.name for v in victims] == ["bound-1", "bound-3"]
    assert {"bound-1", "bound-3"}.isdisjoint(p.name for p in fc.pods) and not a.node_name
    assert [ev["involved"] for ev in fc.events if ev["reason"] == "Preempted"] == ["bound-1", "bound-3"]
    assert fc.schedule_constrained([a])[0][1].name == "node-0"  # the victims' cpu and gpus are back on the node
