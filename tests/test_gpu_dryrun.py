"""ksched_rank_full / ksched_explain_full on the device against the CPU restatement (dryrun_ref: the numpy reason codes
in include/ksched.h's order, the ranked lists from oracle.local_topk under the code-0 mask): every column exactly, scores
by bit pattern.  What each case is here for is asserted on the restatement alone, without a GPU, in
test_dryrun_host.py."""
import dataclasses

import numpy as np
import pytest

import affinity_ref as AR
import dryrun_ref as DR
import ext_ref as ER
import full_ref as FR
import rank_ref as RR
import spread_ref as SR
from test_dryrun_host import (WORKED_LISTS, check_fake_cluster, follow_scheduler, kube_objects, main_case, off_case)

pytestmark = pytest.mark.gpu

TILE = 4  # kDryTile (ksched_dryrun.h): pods a scan wave carries


def engine(cl, **kw):
    from ksched import MODE_EXACT
    from ksched.engine import engine_for
    return engine_for(cl, mode=MODE_EXACT, device=0, **kw)


def load(e, c, t=None):
    """c's tables with the contents of t (None: the initial ones)."""
    t = DR.initial(c) if t is None else t
    if c.group is not None:
        e.load_spread(c.node_domain, c.max_skew, t.counts)
    if c.req_ext is not None:
        e.load_ext(t.ext)
    if c.member is not None:
        e.load_affinity(c.aff_domain, *t.words, n_domains=c.aff_D)


def pod_args(c, pods=slice(None)):
    cut = lambda x: None if x is None else np.ascontiguousarray(x[pods])
    cl = c.cl
    return ((cut(cl.req_cpu), cut(cl.req_mem), cut(cl.req_pods), cut(cl.selector)),
            (cut(c.group), cut(c.enforce), None if c.req_ext is None else np.ascontiguousarray(c.req_ext[:, pods]))
            + tuple(cut(x) for x in c.aff_pods()))


def rank(e, c, k, pods=slice(None)):
    req, cons = pod_args(c, pods)
    return e.rank_full(*req, k, *cons)


def explain(e, c, i, per_node=True):
    cl = c.cl
    g = lambda x, d: d if x is None else x[i]
    return e.explain_full(cl.req_cpu[i], cl.req_mem[i], cl.req_pods[i], g(cl.selector, 0) if cl.use_labels else 0,
                          g(c.group, -1), g(c.enforce, 1), None if c.req_ext is None else c.req_ext[:, i],
                          g(c.member, 0), g(c.anti_host, 0), g(c.anti_zone, 0), g(c.aff_group, -1), g(c.aff_zone, 0),
                          per_node=per_node)


def check(O, c, ks=(5,), t=None):
    with engine(c.cl) as e:
        load(e, c, t)
        for k in ks:
            DR.same(rank(e, c, k), DR.rank_full(O, c, k, t)[0])


def snapshot(e, c):
    """Everything the dry runs promise to leave alone, as bytes."""
    out = [x.tobytes() for x in e.read_nodes()]
    if c.group is not None:
        out.append(e.read_spread().tobytes())
    if c.req_ext is not None:
        out.append(e.read_ext().tobytes())
    if c.member is not None:
        out += [x.tobytes() for x in e.read_affinity()]
    return out


# ---- 1. the header's worked example -----------------------------------------------------------------------------------------
def test_dryrun_worked_example(gpu_available, oracle_mod):
    c, t = DR.worked_example()
    cl = dataclasses.replace(c.cl, alloc_cpu=t.state[0], alloc_mem=t.state[1], alloc_pods=t.state[2])
    c = dataclasses.replace(c, cl=cl)
    with engine(cl) as e:
        load(e, c, t)
        idx, score, reason, count, feas, hist = rank(e, c, 4)
        assert idx.tolist() == [[-1] * 4, [-1] * 4, [2, 3, -1, -1], [2, 3, -1, -1]]
        p3, p4 = float(np.float32(0.3)), float(np.float32(0.4))
        assert score.tolist() == [[0.0] * 4, [0.0] * 4, [p3, p4, 0.0, 0.0], [p3, p4, 0.0, 0.0]]
        assert not reason.any() and count.tolist() == [0, 0, 2, 2] and feas.tolist() == [0, 0, 2, 2]
        want = [[5, 5, 11, 5], [12, 12, 11, 11], [13, 13, 0, 0], [10, 10, 0, 0]]
        for i in range(4):
            counts, per_node = explain(e, c, i)
            assert per_node.tolist() == want[i] and counts.tolist() == np.bincount(want[i], minlength=14).tolist()
            assert hist[i].tolist() == counts.tolist()
        DR.same((idx, score, reason, count, feas, hist), DR.rank_full(oracle_mod, c, 4, t)[0])


# ---- 2. families: every instantiation family, against the initial tables and those ksched_schedule_full left -----------------
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("domain", [0, 1])
@pytest.mark.parametrize("priority", [0, 1])
def test_dryrun_families(priority, domain, labels, gpu_available, oracle_mod):
    O = oracle_mod
    c = main_case(priority, domain, labels)
    cl = c.cl
    with engine(cl) as e:
        load(e, c)
        for k in (1, 5, 16, 64):
            DR.same(rank(e, c, k), DR.rank_full(O, c, k)[0])
        # the engine's own run of the case: the counts, columns, words and rows are the ones it left
        got = e.schedule_full(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, c.gang_off, c.gang_min, c.group, c.enforce,
                              c.req_ext, *c.aff_pods())
        end = FR.schedule_full(O, c)
        FR.same(got, e.read_ext(), e.read_spread(), e.read_affinity(), e.read_nodes(), end)
        for k in (1, 5, 16, 64):
            DR.same(rank(e, c, k), DR.rank_full(O, c, k, DR.after(end))[0])


# ---- 3. node counts: one node, around the wave size, three spans, a last span that ends inside a wave --------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1100, 2500])
def test_dryrun_node_counts(n, gpu_available, oracle_mod):
    # 1100: two spans of 768 rows, the last ends 12 lanes into a wave; 2500: three spans of 1024, the last 4 lanes into one
    check(oracle_mod, FR.adversarial(n, 16, D=min(3, n), D_aff=min(3, n), domain=n % 2, labels=True), ks=(5, 64))


# ---- 4. pod tiles, and subsets: a pod's rows do not depend on the pods ranked with it --------------------------------------------
def test_dryrun_pod_tiles_and_subsets(gpu_available, oracle_mod):
    c = main_case(0, 1)
    want = DR.rank_full(oracle_mod, c, 16)[0]
    with engine(c.cl) as e:
        load(e, c)
        full = rank(e, c, 16)
        DR.same(full, want)
        for m in (1, TILE, TILE + 1, 3 * TILE + 1):
            part = rank(e, c, 16, slice(0, m))
            DR.same(part, tuple(x[:m] for x in want))
            assert all(a.tobytes() == b[:m].tobytes() for a, b in zip(part, full)), m
        for pods in ([63], [3, 17, 40], list(range(63, -1, -3))):
            part = rank(e, c, 16, pods)
            assert all(a.tobytes() == b[pods].tobytes() for a, b in zip(part, full)), pods


# ---- 5. chunks: more pods than one pair of launches serves -----------------------------------------------------------------------
def test_dryrun_chunks(gpu_available, oracle_mod):
    check(oracle_mod, FR.adversarial(300, 1024 + 5, domain=1))


# ---- 6. one constraint at a time, at its extremes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4])
def test_dryrun_ext_only(R, gpu_available, oracle_mod):
    cl, node_ext, req_ext = ER.adversarial(7, 700, 64, R, 0, 1, True)
    check(oracle_mod, FR.Case(cl, node_ext=node_ext, req_ext=req_ext), ks=(5, 64))


def test_dryrun_spread_only_64_by_64(gpu_available, oracle_mod):
    sp = SR.adversarial(7, 300, 64, 64, 64, 0, 1, False)
    check(oracle_mod, FR.Case(sp[0], None, None, *sp[1:]), ks=(5, 64))


@pytest.mark.parametrize("D", [1024, 0, 3])
def test_dryrun_affinity_only(D, gpu_available, oracle_mod):
    a = AR.adversarial(7, 2100, 64, D, 12, 0, 1, False)  # 1024 zones, no zone key, a few zones
    check(oracle_mod, FR.Case(a.cl, aff_D=D, aff_domain=a.node_domain, node_member=a.node_member,
                              node_anti_host=a.node_anti_host, node_anti_zone=a.node_anti_zone, member=a.member,
                              anti_host=a.anti_host, anti_zone=a.anti_zone, aff_group=a.aff_group, aff_zone=a.aff_zone),
          ks=(5, 64))


def test_dryrun_separate_zone_keys(gpu_available, oracle_mod):
    c = FR.adversarial(700, 64, D=4, D_aff=7, domain=1)
    assert not np.array_equal(c.node_domain, c.aff_domain) and c.counts.shape[1] != c.aff_D
    check(oracle_mod, c, ks=(5, 64))


# ---- 7. equivalences -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small93", "c5hc"])
def test_dryrun_all_off_is_ksched_rank(name, gpu_available, oracle_mod):
    cl = RR.make(name)
    c = off_case(cl)
    with engine(cl) as e:
        for k in (1, 16, 64):
            full, plain = rank(e, c, k), e.rank(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, k)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(full[:5], plain))
            DR.same(full, DR.rank_full(oracle_mod, c, k)[0])
        sel = lambda i: int(cl.selector[i]) if cl.use_labels else 0
        for i in (0, 7, cl.n_pods - 1):
            counts, _ = e.explain(cl.req_cpu[i], cl.req_mem[i], cl.req_pods[i], sel(i), per_node=False)
            assert full[5][i].tolist() == counts.tolist() + [0] * 9


def test_dryrun_explain_is_the_rank_row(gpu_available, oracle_mod):
    for c, t in ((main_case(0, 0), None), (main_case(1, 1, False), None)):
        ref, per_node, _ = DR.rank_full(oracle_mod, c, 64, t)
        with engine(c.cl) as e:
            load(e, c, t)
            idx, _, reason, count, _, hist = rank(e, c, 64)
            for i in range(0, c.cl.n_pods, 3):
                counts, codes = explain(e, c, i)
                assert counts.tolist() == hist[i].tolist() and codes.tolist() == per_node[i].tolist(), i
                assert codes[idx[i, :count[i]]].tolist() == reason[i, :count[i]].tolist(), i
                assert explain(e, c, i, per_node=False)[0].tolist() == counts.tolist()


# ---- 8. agreement with the scheduler: rank, then schedule that pod alone; the tables evolve between pods ----------------------------
@pytest.mark.parametrize("priority, domain", [(0, 0), (1, 1)])
def test_dryrun_entry_0_is_what_schedule_full_chooses(priority, domain, gpu_available, oracle_mod):
    c = FR.adversarial(2000, 40, priority=priority, domain=domain, labels=True)
    with engine(c.cl) as e:
        load(e, c)

        def schedule(one, t):
            req, cons = pod_args(one)
            idx, score, feas, placed = e.schedule_full(*req, None, None, *cons)
            return (idx, score, feas, placed, e.read_ext(), e.read_spread(), e.read_nodes(), {}) + e.read_affinity()
        out = follow_scheduler(oracle_mod, c, 4, lambda i, t: rank(e, c, 4, [i]), schedule)
        # ... and where the run ended, the engine's tables are the restatement's
        end = FR.schedule_full(oracle_mod, dataclasses.replace(c, gang_off=None, gang_min=None))
        assert out == end[0].tolist() and sum(w >= 0 for w in out) >= 10 and sum(w < 0 for w in out) >= 1, out
        DR.same(rank(e, c, 4), DR.rank_full(oracle_mod, c, 4, DR.after(end))[0])


# ---- 9. the promise: nothing a context holds changes ----------------------------------------------------------------------------------
def test_dryrun_changes_nothing(gpu_available, oracle_mod):
    from ksched import _lib as L
    from ksched._lib import KschedError
    c = main_case(0, 1)
    cl = c.cl
    with engine(cl) as e:
        load(e, c)
        placed = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)  # (a plain call: explain_batch is valid)
        before = snapshot(e, c) + [x.tobytes() for x in e.results()] + [e.explain_batch()[0].tobytes()]
        rank(e, c, 64)
        rank(e, FR.adversarial(700, 1024 + 5, domain=1, labels=True), 5)  # (other pods, two chunks: the staged ones stay)
        for i in range(0, cl.n_pods, 7):
            explain(e, c, i)
        after = snapshot(e, c) + [x.tobytes() for x in e.results()] + [e.explain_batch()[0].tobytes()]
        assert before == after and (placed[0] >= 0).any()
        assert e.explain_pod(int(np.argmax(placed[0] == L.NO_FIT)))[0].sum() == cl.n_nodes
        # after a constrained call the at-its-turn calls stay refused, before and after a dry run
        e.schedule_full(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector, None, None, c.group, c.enforce, c.req_ext, *c.aff_pods())
        before = snapshot(e, c)
        for _ in range(2):
            with pytest.raises(KschedError) as ei:
                e.explain_batch()
            assert ei.value.code == L.E_STATE
            rank(e, c, 5)
            explain(e, c, 0)
        assert snapshot(e, c) == before


# ---- 10. errors: nothing is changed --------------------------------------------------------------------------------------------------
def test_dryrun_errors(gpu_available, oracle_mod):
    from ksched import MODE_EXACT, Engine
    from ksched import _lib as L
    from ksched._lib import KschedError
    c = main_case(0, 1)
    cl = c.cl

    def code(call):
        with pytest.raises(KschedError) as ei:
            call()
        return ei.value.code

    def with_(**kw):
        return dataclasses.replace(c, **kw)

    def at(x, i, v):
        y = np.array(x)
        y[..., i] = v
        return y
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, device=0) as e:
        assert code(lambda: rank(e, c, 5)) == L.E_STATE and code(lambda: explain(e, c, 0)) == L.E_STATE  # before load_nodes
    off = dict(group=None, enforce=None, req_ext=None, member=None, anti_host=None, anti_zone=None, aff_group=None, aff_zone=None)
    only = {"spread": dict(group=c.group, enforce=c.enforce), "ext": dict(req_ext=c.req_ext), "affinity": dict(aff_group=c.aff_group)}
    i_sp = int(np.argmax((c.group >= 0) & (c.enforce != 0)))
    with engine(cl) as e:
        # a constraint that is on without its table; off, it needs none
        DR.same(rank(e, with_(**off), 5), DR.rank_full(oracle_mod, with_(**off), 5)[0])
        for name, kw in only.items():
            assert code(lambda: rank(e, with_(**{**off, **kw}), 5)) == L.E_STATE, name
        assert code(lambda: explain(e, with_(**{**off, **only["spread"]}), i_sp)) == L.E_STATE
        assert code(lambda: explain(e, with_(**{**off, **only["ext"]}), 0)) == L.E_STATE
        assert code(lambda: explain(e, with_(**{**off, "member": np.ones(cl.n_pods, np.uint64)}), 0)) == L.E_STATE
        load(e, c)
        before = snapshot(e, c)
        bad = [with_(group=at(c.group, 3, c.counts.shape[0])), with_(group=at(c.group, 3, -2)),
               with_(req_ext=at(c.req_ext, 3, -1)), with_(aff_group=at(c.aff_group, 3, 64)),
               with_(aff_group=at(c.aff_group, 3, -2))]
        for b in bad:
            assert code(lambda: rank(e, b, 5)) == L.E_INVALID and code(lambda: explain(e, b, 3)) == L.E_INVALID
        for k in (0, -1, 65):
            assert code(lambda: rank(e, c, k)) == L.E_INVALID, k
        assert code(lambda: e.rank_full(cl.req_cpu, cl.req_mem, cl.req_pods, None, 5)) == L.E_INVALID  # use_labels, no selector
        assert snapshot(e, c) == before
        DR.same(rank(e, c, 5), DR.rank_full(oracle_mod, c, 5)[0])
        assert rank(e, c, 5, slice(0, 0))[0].shape == (0, 5)  # no pods: nothing to do
    # opts.nranks > 1: not served
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, device=0, nranks=2, rank=0,
                nodes_global=2 * cl.n_nodes) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels)
        assert code(lambda: rank(e, with_(**off), 5)) == L.E_INVALID and code(lambda: explain(e, with_(**off), 0)) == L.E_INVALID
    # no node: empty lists and zero counts, as ksched_rank answers
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, device=0) as e:
        z = np.zeros(0, np.int64)
        e.load_nodes(z, z, z, labels=np.zeros(0, np.uint64))
        idx, score, reason, count, feas, hist = rank(e, with_(**off), 5)
        assert (idx == -1).all() and not score.any() and not reason.any() and not count.any() and not feas.any() and not hist.any()
        assert not explain(e, with_(**off), 0)[0].any()


# ---- 11. FakeCluster.rank_pod_full / explain_pod_full on Node and Pod objects -------------------------------------------------------
def test_fake_cluster_dry_runs(gpu_available):
    from ksched import _lib as L
    from ksched.host import FakeCluster
    nodes, bound, four = kube_objects()
    fc = FakeCluster(nodes, list(bound), priority=L.PRIORITY_BEST_PRICE, domain=L.DOMAIN_FEASIBLE, device=0)
    check_fake_cluster(fc, four)
    assert [nd.name for nd, _, _ in fc.rank_pod_full(four["Z"], k=1)] == [WORKED_LISTS["Z"][0][0]]
    assert fc.engine.read_spread().tolist() == [[0]] and fc.engine.read_ext().tolist() == [[0, 0, 0, 0]]  # (Z: no constraint)
    assert [x.tolist() for x in fc.engine.read_affinity()] == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]]
