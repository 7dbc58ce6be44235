"""Shared by the ksched_schedule_ext tests: the CPU restatement of scheduling under extended resources, built on the
oracle as it is.  Per pod the eligibility mask of include/ksched.h's rule -- every column the pod asks for holds at
least the request; a zero request is not checked -- is computed in numpy and folded into the oracle's label check: a
label bit the cluster does not use is ORed into the eligible nodes' labels and into the pod's selector, and
oracle.schedule places that one pod against the running state, so every score is the oracle's, bit for bit.  The
extended columns are then committed in numpy (a wrapping subtraction)."""
import dataclasses

import numpy as np

EXT_BIT = np.uint64(1 << 62)  # free: ksched.cluster.random_small uses bits 0-7 and 63


def worked_example():
    """include/ksched.h's example: best-price, feasible domain, one resource; n0 (0.1, gpu 1), n1 (0.2, gpu 0), n2
    (0.5, gpu 2) with ample room; the pods ask for gpu 1, 0, 2, 1.  Returns (cluster, node_ext, req_ext)."""
    from ksched import cluster
    cl = cluster.Cluster(
        name="ext-example", alloc_cpu=np.full(3, 64000, np.int64), alloc_mem=np.full(3, 1 << 30, np.int64),
        alloc_pods=np.full(3, 110, np.int64), req_cpu=np.full(4, 100, np.int64), req_mem=np.zeros(4, np.int64),
        req_pods=np.ones(4, np.int64), price=np.array([0.1, 0.2, 0.5], np.float32),
        priority=cluster.PRIORITY_BEST_PRICE, domain=cluster.DOMAIN_FEASIBLE)
    return cl, np.array([[1, 0, 2]], np.int64), np.array([[1, 0, 2, 1]], np.int64)


def adversarial(seed, n, p, R, priority=0, domain=0, labels=False):
    """random_small(7, n, p) with its later nodes made roomy in cpu, memory and pod slots, the last one most of all (so
    that the extended columns, not the three core ones, decide most pods, and the highest node index wins some), under
    a random table: columns of 0-4 with a few negative and a few huge entries (the last node: 6 of each); a fifth of
    the pods ask for nothing, the others for 1-3 of each column with probability 0.45.  Returns (cluster, node_ext
    int64[R, n], req_ext int64[R, p])."""
    from ksched import cluster
    rng = np.random.default_rng(seed + 3000)
    cl = cluster.random_small(7, n, p, priority=priority, domain=domain, use_labels=labels)
    roomy = np.arange(n) >= n // 2
    last = np.arange(n) == n - 1  # the roomiest of all: the highest node index wins its share
    cl.alloc_cpu = np.where(roomy, 64000 + 1000 * (np.arange(n) % 7) + 64000 * last, cl.alloc_cpu).astype(np.int64)
    cl.alloc_mem = np.where(roomy, (64 << 20) * (1 + last), cl.alloc_mem).astype(np.int64)
    cl.alloc_pods = np.where(roomy, 110, cl.alloc_pods).astype(np.int64)
    node_ext = rng.integers(0, 5, (R, n)).astype(np.int64)
    node_ext[rng.random((R, n)) < 0.05] = -3
    node_ext[rng.random((R, n)) < 0.03] = (1 << 62) + 5
    node_ext[:, n - 1] = 6
    req_ext = np.where(rng.random((R, p)) < 0.45, rng.integers(1, 4, (R, p)), 0).astype(np.int64)
    req_ext[:, rng.random(p) < 0.2] = 0
    return cl, node_ext, req_ext


def schedule_ext(O, cl, node_ext, req_ext=None, state=None, lo=0, hi=None):
    """Pods [lo, hi) of cl, in order, from the node rows `state` (None: the cluster's) and the table node_ext.
    Returns (idx int32, score f64, feasible int32, final table int64[R, n], final (cpu, mem, pods), info).  info
    counts: narrowed (fewer eligible than fitting nodes), moved (the pick differs from the pick with the constraint
    off, on the same state), ext_nofit (fitting nodes exist, none eligible), zero_req (pods asking for no column),
    multi_col (pods asking for two or more), exact_fit (placements where a request equalled the column, leaving 0),
    overdrawn (placements that took a column they asked for below zero)."""
    hi = cl.n_pods if hi is None else hi
    ext = np.array(node_ext, np.int64)
    R, n = ext.shape
    assert n == cl.n_nodes
    req = np.zeros((R, cl.n_pods), np.int64) if req_ext is None else np.asarray(req_ext, np.int64)
    assert req.shape == (R, cl.n_pods) and (req >= 0).all()
    base_lab = np.zeros(n, np.uint64) if cl.labels is None else np.asarray(cl.labels, np.uint64)
    assert not (base_lab & EXT_BIT).any()
    assert cl.selector is None or not (np.asarray(cl.selector, np.uint64) & EXT_BIT).any()
    state = tuple(np.ascontiguousarray(x, dtype=np.int64).copy()
                  for x in ((cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods) if state is None else state))
    m = hi - lo
    idx = np.empty(m, np.int32); score = np.empty(m, np.float64); feas = np.empty(m, np.int32)
    info = dict(narrowed=0, moved=0, ext_nofit=0, zero_req=0, multi_col=0, exact_fit=0, overdrawn=0)
    for i in range(lo, hi):
        q = req[:, i]
        sel = np.uint64(0) if cl.selector is None or not cl.use_labels else np.uint64(cl.selector[i])
        one = dict(alloc_cpu=state[0], alloc_mem=state[1], alloc_pods=state[2], req_cpu=cl.req_cpu[i:i + 1],
                   req_mem=cl.req_mem[i:i + 1], req_pods=cl.req_pods[i:i + 1],
                   selector=None if cl.selector is None else cl.selector[i:i + 1])
        plain = dataclasses.replace(cl, **one)
        fit = (state[0] >= cl.req_cpu[i]) & (state[1] >= cl.req_mem[i]) & (state[2] >= cl.req_pods[i])
        if cl.use_labels:
            fit &= (base_lab & sel) == sel
        ok = ((q[:, None] == 0) | (q[:, None] <= ext)).all(axis=0)
        elig = fit & ok
        one["selector"] = np.array([sel | EXT_BIT], np.uint64)
        sub = dataclasses.replace(cl, labels=base_lab | np.where(ok, EXT_BIT, np.uint64(0)), use_labels=True, **one)
        oi, os_, of, after = O.schedule(sub)
        assert int(of[0]) == int(elig.sum()), (i, int(of[0]), int(elig.sum()))
        info["narrowed"] += int(elig.sum()) < int(fit.sum())
        info["ext_nofit"] += int(elig.sum()) == 0 and int(fit.sum()) > 0
        info["moved"] += int(O.schedule(plain)[0][0]) != int(oi[0])
        info["zero_req"] += int((q != 0).sum()) == 0
        info["multi_col"] += int((q != 0).sum()) >= 2
        idx[i - lo], score[i - lo], feas[i - lo] = oi[0], os_[0], of[0]
        state = after
        w = int(oi[0])
        if w >= 0:
            info["exact_fit"] += bool(((q > 0) & (q == ext[:, w])).any())
            with np.errstate(over="ignore"):
                ext[:, w] = (ext[:, w].view(np.uint64) - q.view(np.uint64)).view(np.int64)
            info["overdrawn"] += bool(((q > 0) & (ext[:, w] < 0)).any())
    return idx, score, feas, ext, state, info


def same(got, got_ext, got_state, ref):
    """got: Engine.schedule_ext's result, got_ext: Engine.read_ext(), got_state: Engine.read_nodes() after it, ref:
    schedule_ext() above.  Every column exactly, scores by bit pattern."""
    names = ("idx", "score", "feasible", "ext", "cpu", "mem", "pods")
    g = (got[0], np.ascontiguousarray(got[1]).view(np.int64), got[2], got_ext) + tuple(got_state)
    r = (ref[0], np.ascontiguousarray(ref[1]).view(np.int64), ref[2], ref[3]) + tuple(ref[4])
    for nm, a, b in zip(names, g, r):
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
