"""ksched_preempt restated in plain Python (include/ksched.h has the rules), and the clusters its tests share.

Per pod and node: the table's pods below the pod's priority are the potential victims; with all of them gone the pod
must fit, or the node is no candidate; then they are walked most important first (priority descending, table index
ascending) and each one the pod still fits without is given back.  The rest are the victims; the node's key is
(max victim prio, sum of prio + 2^31, count), the smallest key wins, then the lowest node index."""
import numpy as np

NO_FIT = -1
NO_VICTIM_PRIO = -(1 << 31)
M64 = (1 << 64) - 1


def wrap(v):
    """int64 wrap-around of a Python int."""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def gen(seed, n, m, maxseg=70):
    r = np.random.default_rng(seed)
    seg = r.integers(0, maxseg + 1, n); seg[r.random(n) < 0.1] = 0
    node = np.repeat(np.arange(n), seg); node = node[r.permutation(node.size)].astype(np.int32); nb = node.size
    bc = r.integers(1, 40, nb) * 50; bm = r.integers(0, 64, nb) * (1 << 10); bp = r.integers(-2, 6, nb).astype(np.int32) * 100
    alloc = r.integers(0, 4000, n), r.integers(0, 1 << 20, n), r.integers(0, 4, n)
    pods = r.integers(1, 400, m) * 50, r.integers(0, 1 << 20, m), r.integers(1, 4, m), r.integers(-3, 8, m).astype(np.int32) * 100
    return alloc, (node, bc, bm, bp), pods


def labels_for(seed, n, m):
    """Node labels and pod selectors drawn as ksched.cluster.random_small draws them."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 1 << 8, size=n, dtype=np.uint64) | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63))
    selector = rng.choice(np.array([0, 1, 2, 3, 1 << 7, (1 << 63) | 1], dtype=np.uint64), size=m)
    return labels, selector


def fits(req, free, sel=0, lab=0, use_labels=False):
    ok = free[0] >= req[0] and free[1] >= req[1] and free[2] >= req[2]
    return ok and (not use_labels or (lab & sel) == sel)


def node_key(req, prio, alloc, seg, sel=0, lab=0, use_labels=False):
    """One pod on one node.  seg: the node's table pods as (table index, cpu, mem, prio).  None when the node is no
    candidate, else ((max prio, sum, count), [victim table indices in the walk's order])."""
    pot = sorted((e for e in seg if e[3] < prio), key=lambda e: (-e[3], e[0]))
    free = [wrap(alloc[0] + sum(e[1] for e in pot)), wrap(alloc[1] + sum(e[2] for e in pot)), wrap(alloc[2] + len(pot))]
    if not fits(req, free, sel, lab, use_labels):
        return None
    victims = []
    for t, c, mm, _ in pot:
        less = [wrap(free[0] - c), wrap(free[1] - mm), wrap(free[2] - 1)]
        if fits(req, less, sel, lab, use_labels):
            free = less
        else:
            victims.append(t)
    by = {e[0]: e[3] for e in seg}
    mx = max((by[t] for t in victims), default=NO_VICTIM_PRIO)
    return (mx, wrap(sum(by[t] + (1 << 31) for t in victims)), len(victims)), victims


def preempt(alloc, bound, pods, vcap, lo=0, hi=None, labels=None, selector=None):
    """The six columns of ksched_preempt for nodes [lo, hi) of the cluster (a shard; the whole cluster by default).
    Node indices, in `bound` and in the answer, are the cluster's (global); victim indices are positions in `bound`
    as given."""
    ac, am, ap = (np.asarray(x) for x in alloc)
    bn, bc, bm, bp = (np.asarray(x) for x in bound)
    rc, rm, rp, pr = (np.asarray(x) for x in pods)
    hi = len(ac) if hi is None else hi
    use_labels = labels is not None
    segs = {j: [] for j in range(lo, hi)}
    for t in range(len(bn)):
        if lo <= int(bn[t]) < hi:
            segs[int(bn[t])].append((t, int(bc[t]), int(bm[t]), int(bp[t])))
    m = len(rc)
    node = np.full(m, NO_FIT, np.int32); nv = np.zeros(m, np.int32); mx = np.full(m, NO_VICTIM_PRIO, np.int32)
    sm = np.zeros(m, np.int64); cand = np.zeros(m, np.int32); vic = np.full((m, vcap), -1, np.int32)
    for i in range(m):
        best = None
        req = (int(rc[i]), int(rm[i]), int(rp[i]))
        for j in range(lo, hi):
            r = node_key(req, int(pr[i]), (int(ac[j]), int(am[j]), int(ap[j])), segs[j],
                         int(selector[i]) if use_labels else 0, int(labels[j]) if use_labels else 0, use_labels)
            if r is None:
                continue
            cand[i] += 1
            if best is None or r[0] < best[0]:  # strict: the lowest index keeps a tie
                best = (r[0], j, r[1])
        if best is not None:
            (mx[i], sm[i], nv[i]), j, victims = best
            node[i] = j
            vic[i, :min(vcap, len(victims))] = victims[:vcap]
    return node, nv, mx, sm, cand, vic


def same(got, want):
    names = ("node", "nvictims", "max_prio", "sum_prio", "candidates", "victims")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if len(g) else []
        assert len(bad) == 0, (name, "first differing pod", int(bad[0]), g[bad[0]], w[bad[0]])


def classes(want):
    """(NO_FIT pods, pods that need no victim, pods with more than one victim) of an answer."""
    node, nv = want[0], want[1]
    return int((node == NO_FIT).sum()), int(((node >= 0) & (nv == 0)).sum()), int((nv > 1).sum())
