"""Shared by the ksched_schedule_constrained tests: the CPU restatement of gangs, topology spread and extended resources
in one run, built on the oracle as it is.  Gang by gang: the node rows, the extended-resource table and the spread counts
are snapshotted at the gang's start; per member the combined eligibility mask of include/ksched.h's rule (spread_ok &&
ext_ok) is computed in numpy and folded into the oracle's label check through free label bit 62, oracle.schedule places
that one pod against the running state -- so every score is the oracle's, bit for bit -- and the member's extended
requests and spread count are committed in numpy; at the gang's end the state is kept or the snapshot restored."""
import dataclasses

import numpy as np

import ext_ref as ER
import gang_ref as GR
import spread_ref as SR

FREE_BIT = np.uint64(1 << 62)  # free: ksched.cluster.random_small uses bits 0-7 and 63
GANG_REJECTED = GR.GANG_REJECTED


@dataclasses.dataclass
class Case:
    """One input of ksched_schedule_constrained; a constraint is off where its fields are None."""
    cl: object
    gang_off: object = None
    gang_min: object = None
    node_domain: object = None
    max_skew: object = None
    counts: object = None
    group: object = None
    enforce: object = None
    node_ext: object = None
    req_ext: object = None


def worked_example():
    """include/ksched.h's example: best-price, feasible domain; n0 (zone A, 0.1, gpu 2), n1 (A, 0.2, gpu 1), n2 (B, 0.5,
    gpu 1) with ample room; one group, max_skew 1, counts 0; gangs {p0, p1, p2}, {p3, p4}, {p5}, every member required;
    p0-p4 in the group and enforcing, p5 in none; gpu requests 1, 1, 1, 0, 2, 1."""
    from ksched import cluster
    cl = cluster.Cluster(
        name="constrained-example", alloc_cpu=np.full(3, 64000, np.int64), alloc_mem=np.full(3, 1 << 30, np.int64),
        alloc_pods=np.full(3, 110, np.int64), req_cpu=np.full(6, 100, np.int64), req_mem=np.zeros(6, np.int64),
        req_pods=np.ones(6, np.int64), price=np.array([0.1, 0.2, 0.5], np.float32),
        priority=cluster.PRIORITY_BEST_PRICE, domain=cluster.DOMAIN_FEASIBLE)
    return Case(cl, gang_off=np.array([0, 3, 5, 6], np.int64), node_domain=np.array([0, 0, 1], np.int32),
                max_skew=np.array([1], np.int32), counts=np.zeros((1, 2), np.int32),
                group=np.array([0, 0, 0, 0, 0, -1], np.int32), enforce=np.ones(6, np.uint8),
                node_ext=np.array([[2, 1, 1]], np.int64), req_ext=np.array([[1, 1, 1, 0, 2, 1]], np.int64))


def adversarial(n, p, R=4, D=3, S=2, priority=0, domain=0, labels=False, half=False, seed=7, gang_off=None):
    """The existing generators composed: the cluster, node_ext and req_ext of ext_ref.adversarial(seed, n, p, R, ...),
    the table, groups and enforce flags of spread_ref.adversarial(seed, n, p, D, S, ...), and gang_ref.cycle_gangs(p)
    (or gang_off), every member required or -- half -- ceil(size / 2) of them.  seed: one for both generators, or
    (ext_ref's, spread_ref's)."""
    ext_seed, spread_seed = seed if isinstance(seed, tuple) else (seed, seed)
    cl, node_ext, req_ext = ER.adversarial(ext_seed, n, p, R, priority, domain, labels)
    _, dom, max_skew, counts, group, enforce = SR.adversarial(spread_seed, n, p, D, S, priority, domain, labels)
    off = GR.cycle_gangs(p) if gang_off is None else np.asarray(gang_off, np.int64)
    return Case(cl, off, GR.half_min(off) if half else None, dom, max_skew, counts, group, enforce, node_ext, req_ext)


def pods(c, lo, hi):
    """Pods [lo, hi) of case c as a case of their own (the gangs are not sliced: pass gang_off for the slice)."""
    cl = c.cl
    sub = dataclasses.replace(cl, req_cpu=cl.req_cpu[lo:hi], req_mem=cl.req_mem[lo:hi], req_pods=cl.req_pods[lo:hi],
                              selector=None if cl.selector is None else cl.selector[lo:hi])
    return dataclasses.replace(c, cl=sub, gang_off=None, gang_min=None,
                               group=None if c.group is None else c.group[lo:hi],
                               enforce=None if c.enforce is None else c.enforce[lo:hi],
                               req_ext=None if c.req_ext is None else c.req_ext[:, lo:hi])


def schedule_constrained(O, c, state=None):
    """Case c from the node rows `state` (None: the cluster's) and c's tables.  Returns (idx int32[p], score f64[p],
    feasible int32[p], gang_placed int32[g] (empty without gangs), final ext int64[R, n] | None, final counts int32[S, D]
    | None, final (cpu, mem, pods), info).  info counts: rejected gangs, rejected gangs that undid a commit (rollbacks),
    accepted gangs with a failed member (partial), accepted gangs after the first rejected one (accepted_after_reject),
    rejected gangs that had taken an extended column (undo_ext), that had raised a count (undo_spread), whose rollback
    lowered some row's minimum (min_fell); pods with fewer spread-eligible than fitting nodes (narrowed_spread) and with
    fewer ext-eligible than fitting nodes (narrowed_ext)."""
    cl = c.cl
    p, n = cl.n_pods, cl.n_nodes
    off = np.arange(p + 1, dtype=np.int64) if c.gang_off is None else np.asarray(c.gang_off, np.int64)
    ng = off.shape[0] - 1
    assert off[0] == 0 and off[ng] == p and np.all(np.diff(off) > 0)
    spread, extd = c.group is not None, c.req_ext is not None
    if spread:
        dom = np.asarray(c.node_domain, np.int64)
        cnt = np.array(c.counts, np.int64)
        D = cnt.shape[1]
        assert D > dom.max() and set(range(D)) <= set(dom.tolist()), "domain ids must be compact and carried"
        has_key = dom >= 0
        group = np.asarray(c.group, np.int64)
        enforce = np.ones(p, bool) if c.enforce is None else np.asarray(c.enforce) != 0
    else:
        cnt = None
    if extd:
        ext = np.array(c.node_ext, np.int64)
        req = np.asarray(c.req_ext, np.int64)
        assert ext.shape[1] == n and req.shape == (ext.shape[0], p) and (req >= 0).all()
    else:
        ext = None
    base_lab = np.zeros(n, np.uint64) if cl.labels is None else np.asarray(cl.labels, np.uint64)
    assert not (base_lab & FREE_BIT).any()
    assert cl.selector is None or not (np.asarray(cl.selector, np.uint64) & FREE_BIT).any()
    state = tuple(np.ascontiguousarray(x, dtype=np.int64).copy()
                  for x in ((cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods) if state is None else state))
    idx = np.empty(p, np.int32); score = np.empty(p, np.float64); feas = np.empty(p, np.int32)
    placed = np.zeros(ng, np.int32)
    info = dict(rejected=0, rollbacks=0, partial=0, accepted_after_reject=0, undo_ext=0, undo_spread=0, min_fell=0,
                narrowed_spread=0, narrowed_ext=0)
    for g in range(ng):
        lo, hi = int(off[g]), int(off[g + 1])
        snap = (state, None if ext is None else ext.copy(), None if cnt is None else cnt.copy())
        took_ext = raised = False
        for i in range(lo, hi):
            sel = np.uint64(0) if cl.selector is None or not cl.use_labels else np.uint64(cl.selector[i])
            one = dict(alloc_cpu=state[0], alloc_mem=state[1], alloc_pods=state[2], req_cpu=cl.req_cpu[i:i + 1],
                       req_mem=cl.req_mem[i:i + 1], req_pods=cl.req_pods[i:i + 1],
                       selector=None if cl.selector is None else cl.selector[i:i + 1])
            fit = (state[0] >= cl.req_cpu[i]) & (state[1] >= cl.req_mem[i]) & (state[2] >= cl.req_pods[i])
            if cl.use_labels:
                fit &= (base_lab & sel) == sel
            ok = np.ones(n, bool)
            s = int(group[i]) if spread else -1
            if s >= 0 and enforce[i]:
                sp_ok = has_key & (cnt[s][np.where(has_key, dom, 0)] + 1 - cnt[s].min() <= int(c.max_skew[s]))
                info["narrowed_spread"] += int((fit & sp_ok).sum()) < int(fit.sum())
                ok &= sp_ok
            q = req[:, i] if extd else None
            if extd and (q != 0).any():
                ext_ok = ((q[:, None] == 0) | (q[:, None] <= ext)).all(axis=0)
                info["narrowed_ext"] += int((fit & ext_ok).sum()) < int(fit.sum())
                ok &= ext_ok
            if ok.all():
                oi, os_, of, after = O.schedule(dataclasses.replace(cl, **one))
            else:
                one["selector"] = np.array([sel | FREE_BIT], np.uint64)
                oi, os_, of, after = O.schedule(dataclasses.replace(
                    cl, labels=base_lab | np.where(ok, FREE_BIT, np.uint64(0)), use_labels=True, **one))
            assert int(of[0]) == int((fit & ok).sum()), (i, int(of[0]), int((fit & ok).sum()))
            idx[i], score[i], feas[i] = oi[0], os_[0], of[0]
            state = after
            w = int(oi[0])
            if w >= 0:
                if extd and (q != 0).any():
                    took_ext = True
                    with np.errstate(over="ignore"):
                        ext[:, w] = (ext[:, w].view(np.uint64) - q.view(np.uint64)).view(np.int64)
                if s >= 0 and dom[w] >= 0:
                    raised = True
                    cnt[s, dom[w]] += 1
        n_placed = int((idx[lo:hi] >= 0).sum())
        need = hi - lo if c.gang_min is None or c.gang_off is None else int(c.gang_min[g])
        if n_placed >= need:
            placed[g] = n_placed
            info["partial"] += n_placed < hi - lo
            info["accepted_after_reject"] += info["rejected"] > 0
        else:
            idx[lo:hi] = np.where(idx[lo:hi] >= 0, GANG_REJECTED, idx[lo:hi])
            score[lo:hi] = 0.0
            info["rejected"] += 1
            info["rollbacks"] += n_placed > 0
            info["undo_ext"] += took_ext
            info["undo_spread"] += raised
            if cnt is not None:
                info["min_fell"] += bool((snap[2].min(axis=1) < cnt.min(axis=1)).any())
            state, ext, cnt = snap
    if c.gang_off is None:
        placed = placed[:0]
    return idx, score, feas, placed, ext, None if cnt is None else cnt.astype(np.int32), state, info


def same(got, got_ext, got_counts, got_state, ref):
    """got: Engine.schedule_constrained's result; got_ext / got_counts: Engine.read_ext() / read_spread() (None where
    the constraint is off); got_state: Engine.read_nodes() after it; ref: schedule_constrained() above.  Every column
    exactly, scores by bit pattern."""
    names = ["idx", "score", "feasible", "gang_placed", "cpu", "mem", "pods"]
    g = [got[0], np.ascontiguousarray(got[1]).view(np.int64), got[2], got[3]] + list(got_state)
    r = [ref[0], np.ascontiguousarray(ref[1]).view(np.int64), ref[2], ref[3]] + list(ref[6])
    for nm, a, b in (("ext", got_ext, ref[4]), ("counts", got_counts, ref[5])):
        assert (a is None) == (b is None), nm
        if a is not None:
            names.append(nm); g.append(a); r.append(b)
    for nm, a, b in zip(names, g, r):
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
