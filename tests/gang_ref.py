"""Shared by the ksched_schedule_gangs tests: the CPU restatement of gang scheduling from the oracle.  Gangs in
order; each gang's slice goes through oracle.schedule against the current node state, and the state it returns
is kept when enough members found a node and dropped otherwise (include/ksched.h has the rules)."""
import dataclasses

import numpy as np

GANG_REJECTED = -3
SIZE_CYCLE = (1, 2, 3, 5, 8, 13)


def worked_example():
    """Best-price, feasible domain: node A (price 0.1) and B (0.5), 1000 cpu each, memory and pods ample; pods by
    cpu 600, 600, 300, 600, 400 in the gangs {p0, p1}, {p2, p3}, {p4}."""
    from ksched import cluster
    return cluster.Cluster(
        name="gang-example", alloc_cpu=np.array([1000, 1000], np.int64), alloc_mem=np.full(2, 1 << 30, np.int64),
        alloc_pods=np.full(2, 110, np.int64), req_cpu=np.array([600, 600, 300, 600, 400], np.int64),
        req_mem=np.zeros(5, np.int64), req_pods=np.ones(5, np.int64), price=np.array([0.1, 0.5], np.float32),
        priority=cluster.PRIORITY_BEST_PRICE, domain=cluster.DOMAIN_FEASIBLE), np.array([0, 2, 4, 5], np.int64)


def cycle_gangs(p, sizes=SIZE_CYCLE):
    """CSR offsets of gangs whose sizes cycle through `sizes`, the last one cut at p."""
    off = [0]
    k = 0
    while off[-1] < p:
        off.append(min(p, off[-1] + sizes[k % len(sizes)]))
        k += 1
    return np.asarray(off, dtype=np.int64)


def half_min(off):
    """gang_min = ceil(size / 2)."""
    size = np.diff(off)
    return ((size + 1) // 2).astype(np.int32)


def schedule_gangs(O, cl, gang_off, gang_min=None):
    """Returns (idx int32[p], score f64[p], feasible int32[p], gang_placed int32[g], final (cpu, mem, pods),
    info) -- info counts the classes the tests assert: rejected gangs, rejected gangs that undid a commit
    (rollbacks), accepted gangs with a failed member (partial), accepted gangs after the first rejected one."""
    off = np.asarray(gang_off, dtype=np.int64)
    ng = off.shape[0] - 1
    p = cl.n_pods
    assert off[0] == 0 and off[ng] == p and np.all(np.diff(off) > 0)
    state = tuple(np.ascontiguousarray(x, dtype=np.int64).copy() for x in (cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods))
    idx = np.empty(p, np.int32); score = np.empty(p, np.float64); feas = np.empty(p, np.int32)
    placed = np.zeros(ng, np.int32)
    info = dict(rejected=0, rollbacks=0, partial=0, accepted_after_reject=0)
    for g in range(ng):
        lo, hi = int(off[g]), int(off[g + 1])
        sub = dataclasses.replace(cl, alloc_cpu=state[0], alloc_mem=state[1], alloc_pods=state[2],
                                  req_cpu=cl.req_cpu[lo:hi], req_mem=cl.req_mem[lo:hi], req_pods=cl.req_pods[lo:hi],
                                  selector=None if cl.selector is None else cl.selector[lo:hi])
        oi, os_, of, after = O.schedule(sub)
        n_placed = int((oi >= 0).sum())
        need = hi - lo if gang_min is None else int(gang_min[g])
        feas[lo:hi] = of
        if n_placed >= need:
            idx[lo:hi] = oi; score[lo:hi] = os_
            placed[g] = n_placed
            state = after
            info["partial"] += n_placed < hi - lo
            info["accepted_after_reject"] += info["rejected"] > 0
        else:
            idx[lo:hi] = np.where(oi >= 0, GANG_REJECTED, oi)
            score[lo:hi] = 0.0
            info["rejected"] += 1
            info["rollbacks"] += n_placed > 0
    return idx, score, feas, placed, state, info


def same(got, state, ref):
    """got: Engine.schedule_gangs' result, state: Engine.read_nodes() after it, ref: schedule_gangs() above.
    Every column exactly, scores by bit pattern."""
    names = ("idx", "score", "feasible", "gang_placed", "cpu", "mem", "pods")
    g = (got[0], np.ascontiguousarray(got[1]).view(np.int64), got[2], got[3]) + tuple(state)
    r = (ref[0], np.ascontiguousarray(ref[1]).view(np.int64), ref[2], ref[3]) + tuple(ref[4])
    for nm, a, b in zip(names, g, r):
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
