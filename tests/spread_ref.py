"""Shared by the ksched_schedule_spread tests: the CPU restatement of topology spread scheduling, built on the
oracle as it is.  Per pod the eligibility mask of include/ksched.h's rule is computed in numpy and folded into the
oracle's label check -- a label bit the cluster does not use is ORed into the eligible nodes' labels and into the
pod's selector -- and oracle.schedule places that one pod against the running state, so every score is the
oracle's, bit for bit."""
import dataclasses

import numpy as np

SPREAD_BIT = np.uint64(1 << 62)  # free: ksched.cluster.random_small uses bits 0-7 and 63


def worked_example():
    """include/ksched.h's example: best-price, feasible domain; n0 (zone A, 0.1), n1 (A, 0.2), n2 (B, 0.5) with ample
    room; one group, max_skew 1, counts 0; four enforcing pods.  Returns (cluster, node_domain, max_skew, counts,
    group, enforce)."""
    from ksched import cluster
    cl = cluster.Cluster(
        name="spread-example", alloc_cpu=np.full(3, 64000, np.int64), alloc_mem=np.full(3, 1 << 30, np.int64),
        alloc_pods=np.full(3, 110, np.int64), req_cpu=np.full(4, 100, np.int64), req_mem=np.zeros(4, np.int64),
        req_pods=np.ones(4, np.int64), price=np.array([0.1, 0.2, 0.5], np.float32),
        priority=cluster.PRIORITY_BEST_PRICE, domain=cluster.DOMAIN_FEASIBLE)
    return (cl, np.array([0, 0, 1], np.int32), np.array([1], np.int32), np.zeros((1, 2), np.int32),
            np.zeros(4, np.int32), np.ones(4, np.uint8))


def adversarial(seed, n, p, D, S, priority=0, domain=0, labels=False):
    """random_small(7, n, p) under a random table: shuffled domains, every 11th node without the key (where its
    domain keeps another carrier), skews 1-2, counts 0-2, groups in [-1, S), three pods in four enforcing."""
    from ksched import cluster
    rng = np.random.default_rng(seed + 1000)
    dom = (np.arange(n) % D).astype(np.int32)
    rng.shuffle(dom)
    for j in range(0, n, 11):
        if (dom == dom[j]).sum() > 1:
            dom[j] = -1
    max_skew = rng.integers(1, 3, S).astype(np.int32)
    counts = rng.integers(0, 3, (S, D)).astype(np.int32)
    group = rng.integers(-1, S, p).astype(np.int32)
    enforce = (rng.random(p) < 0.75).astype(np.uint8)
    cl = cluster.random_small(7, n, p, priority=priority, domain=domain, use_labels=labels)
    return cl, dom, max_skew, counts, group, enforce


def healthy(seed, n, p, D, S):
    """Roomy nodes and small pods (resource priority, feasible domain), so the constraint and not the resources
    decides: max_skew 1, counts 0, 90 % of the pods in group 0 and 90 % enforcing; the first D nodes carry domains
    0..D-1, the rest any of [-1, D)."""
    from ksched import cluster
    rng = np.random.default_rng(seed + 2000)
    cl = cluster.Cluster(
        name=f"healthy{seed}", alloc_cpu=rng.choice(np.array([4000, 8000, 16000], np.int64), size=n),
        alloc_mem=np.full(n, 64 << 20, np.int64), alloc_pods=np.full(n, 110, np.int64),
        req_cpu=rng.choice(np.array([100, 250, 500], np.int64), size=p),
        req_mem=rng.choice(np.array([1024, 65536], np.int64), size=p), req_pods=np.ones(p, np.int64),
        priority=cluster.PRIORITY_RESOURCE, domain=cluster.DOMAIN_FEASIBLE)
    dom = np.concatenate([np.arange(D), rng.integers(-1, D, n - D)]).astype(np.int32)
    group = np.where(rng.random(p) < 0.9, 0, rng.integers(-1, S, p)).astype(np.int32)
    enforce = (rng.random(p) < 0.9).astype(np.uint8)
    return cl, dom, np.ones(S, np.int32), np.zeros((S, D), np.int32), group, enforce


def schedule_spread(O, cl, node_domain, max_skew, counts, group, enforce=None, state=None):
    """Returns (idx int32[p], score f64[p], feasible int32[p], final counts int32[S, D], final (cpu, mem, pods),
    info).  info counts, over the enforcing pods unless noted: narrowed (fewer eligible than fitting nodes), moved
    (the pick differs from the pick with the constraint off, same state), spread_nofit (no eligible node but fitting
    ones), min_rose (increments of any pod that raised their row's minimum), count_only (placed pods that only
    count), off_domain (placed group pods on a node without the key)."""
    p = cl.n_pods
    dom = np.asarray(node_domain, np.int64)
    cnt = np.array(counts, np.int64)
    S, D = cnt.shape
    group = np.asarray(group, np.int64)
    enforce = np.ones(p, bool) if enforce is None else np.asarray(enforce) != 0
    base_lab = np.zeros(cl.n_nodes, np.uint64) if cl.labels is None else np.asarray(cl.labels, np.uint64)
    assert not (base_lab & SPREAD_BIT).any()
    assert cl.selector is None or not (np.asarray(cl.selector, np.uint64) & SPREAD_BIT).any()
    assert D > dom.max() and set(range(D)) <= set(dom.tolist()), "domain ids must be compact and carried"
    state = tuple(np.ascontiguousarray(x, dtype=np.int64).copy()
                  for x in ((cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods) if state is None else state))
    idx = np.empty(p, np.int32); score = np.empty(p, np.float64); feas = np.empty(p, np.int32)
    info = dict(narrowed=0, moved=0, spread_nofit=0, min_rose=0, count_only=0, off_domain=0)
    has_key = dom >= 0
    for i in range(p):
        s, e = int(group[i]), bool(enforce[i]) and group[i] >= 0
        sel = np.uint64(0) if cl.selector is None or not cl.use_labels else np.uint64(cl.selector[i])
        one = dict(alloc_cpu=state[0], alloc_mem=state[1], alloc_pods=state[2], req_cpu=cl.req_cpu[i:i + 1],
                   req_mem=cl.req_mem[i:i + 1], req_pods=cl.req_pods[i:i + 1],
                   selector=None if cl.selector is None else cl.selector[i:i + 1])
        plain = dataclasses.replace(cl, **one)
        if e:
            fit = (state[0] >= cl.req_cpu[i]) & (state[1] >= cl.req_mem[i]) & (state[2] >= cl.req_pods[i])
            if cl.use_labels:
                fit &= (base_lab & sel) == sel
            ok = has_key & (cnt[s][np.where(has_key, dom, 0)] + 1 - cnt[s].min() <= int(max_skew[s]))
            elig = fit & ok
            one["selector"] = np.array([sel | SPREAD_BIT], np.uint64)
            sub = dataclasses.replace(cl, labels=base_lab | np.where(ok, SPREAD_BIT, np.uint64(0)), use_labels=True,
                                      **one)
            oi, os_, of, after = O.schedule(sub)
            assert int(of[0]) == int(elig.sum()), (i, int(of[0]), int(elig.sum()))
            info["narrowed"] += int(elig.sum()) < int(fit.sum())
            info["spread_nofit"] += int(elig.sum()) == 0 and int(fit.sum()) > 0
            info["moved"] += int(O.schedule(plain)[0][0]) != int(oi[0])
        else:
            oi, os_, of, after = O.schedule(plain)
        idx[i], score[i], feas[i] = oi[0], os_[0], of[0]
        state = after
        w = int(oi[0])
        if w >= 0 and s >= 0:
            info["count_only"] += not e
            if dom[w] >= 0:
                before = cnt[s].min()
                cnt[s, dom[w]] += 1
                info["min_rose"] += cnt[s].min() > before
            else:
                info["off_domain"] += 1
    return idx, score, feas, cnt.astype(np.int32), state, info


def same(got, got_counts, got_state, ref):
    """got: Engine.schedule_spread's result, got_counts: Engine.read_spread(), got_state: Engine.read_nodes() after
    it, ref: schedule_spread() above.  Every column exactly, scores by bit pattern."""
    names = ("idx", "score", "feasible", "counts", "cpu", "mem", "pods")
    g = (got[0], np.ascontiguousarray(got[1]).view(np.int64), got[2], got_counts) + tuple(got_state)
    r = (ref[0], np.ascontiguousarray(ref[1]).view(np.int64), ref[2], ref[3]) + tuple(ref[4])
    for nm, a, b in zip(names, g, r):
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
