"""ksched_preempt_constrained restated in plain Python (include/ksched.h has the rules), built on preempt_ref, and the
clusters its tests share.

Per pod and node ksched_preempt's walk, with one eligibility in the place of fits: the pod fits into what is free, every
non-zero extended request is covered by the node's column plus what the removed pods held, and -- for a pod that
enforces a spread group, on a node that carries the key -- c + 1 - min(mo, c) <= max_skew, where c is the loaded count
of the node's domain less the removed pods the group counts and mo the smallest loaded count of the other domains."""
import dataclasses

import numpy as np

import preempt_ref as PR

NO_FIT, NO_VICTIM_PRIO, wrap, fits = PR.NO_FIT, PR.NO_VICTIM_PRIO, PR.wrap, PR.fits


@dataclasses.dataclass
class Case:
    alloc: tuple               # (cpu, mem, pods) int64[n]
    bound: tuple               # (node int32[nb], cpu, mem, prio int32[nb])
    pods: tuple                # (cpu, mem, pods, prio int32[m])
    node_ext: np.ndarray       # int64[R, n]
    bound_ext: np.ndarray      # int64[R, nb]
    req_ext: np.ndarray        # int64[R, m]
    node_domain: np.ndarray    # int32[n], -1: no key
    skew: np.ndarray           # int32[S]
    counts: np.ndarray         # int32[S, D]
    bound_spread: np.ndarray   # uint64[nb], bit s: counted in group s
    group: np.ndarray          # int32[m], -1: none
    enforce: np.ndarray        # uint8[m]

    @property
    def n(self):
        return len(self.alloc[0])

    @property
    def m(self):
        return len(self.pods[0])


def table_counts(node, node_domain, bound_spread, S, D):
    """counts[s, d] = the table's pods with bit s on a node of domain d."""
    counts = np.zeros((S, D), np.int32)
    for t in range(len(node)):
        d = int(node_domain[node[t]])
        if d >= 0:
            for s in range(S):
                counts[s, d] += (int(bound_spread[t]) >> s) & 1
    return counts


def extend(seed, alloc, bound, pods, R=2, D=5, S=3, balanced=False, nokey=0.08):
    """The constraint columns for a preempt_ref cluster: R ext columns (node amounts 0-2, bound amounts 0-2 on about
    40 % of the pods, requests 1-4 on about half the pods per column), D zones (about `nokey` of the nodes without the
    key, every id carried), S groups (each bound pod in each group at 0.35), counts equal to the table's per-domain
    counts or -- balanced -- the row maximum plus 0-2, skews 1-3, pod groups in [-1, S), enforcing at 0.8."""
    r = np.random.default_rng(seed + 1000)
    n, nb, m = len(alloc[0]), len(bound[0]), len(pods[0])
    node_ext = r.integers(0, 3, (R, n)).astype(np.int64)
    bound_ext = (r.integers(0, 3, (R, nb)) * (r.random((R, nb)) < 0.4)).astype(np.int64)
    req_ext = (r.integers(1, 5, (R, m)) * (r.random((R, m)) < 0.5)).astype(np.int64)
    D = min(D, n)
    dom = r.integers(0, D, n).astype(np.int32)
    dom[:D] = np.arange(D)  # every id carried (by a node that keeps the key)
    drop = np.flatnonzero(r.random(n) < nokey)
    dom[drop[drop >= D]] = -1
    mask = np.zeros(nb, np.uint64)
    for s in range(S):
        mask |= (r.random(nb) < 0.35).astype(np.uint64) << np.uint64(s)
    counts = table_counts(bound[0], dom, mask, S, D)
    if balanced:
        counts = (counts.max(axis=1, keepdims=True) + r.integers(0, 3, (S, D))).astype(np.int32)
    skew = r.integers(1, 4, S).astype(np.int32)
    group = r.integers(-1, S, m).astype(np.int32)
    enforce = (r.random(m) < 0.8).astype(np.uint8)
    return Case(alloc, bound, pods, node_ext, bound_ext, req_ext, dom, skew, counts, mask, group, enforce)


def gen(seed, n, m, balanced=False, maxseg=70, **kw):
    return extend(seed, *PR.gen(seed, n, m, maxseg=maxseg), balanced=balanced, **kw)


def elig(req, req_ext, free, fext, rem, sp, sel=0, lab=0, use_labels=False):
    """include/ksched.h's elig.  sp: None (the pod enforces no group, or spread is off), or (d, C, mo, max_skew) with
    d the node's domain and mo None where there is no other domain."""
    if not fits(req, free, sel, lab, use_labels):
        return False
    if any(q != 0 and q > f for q, f in zip(req_ext, fext)):
        return False
    if sp is None:
        return True
    d, C, mo, skew = sp
    if d < 0:
        return False
    c = C - rem
    return c + 1 - (c if mo is None else min(mo, c)) <= skew


def node_key(req, req_ext, prio, alloc, ext, seg, sp, s, sel=0, lab=0, use_labels=False):
    """One pod on one node.  seg: the node's table pods as (table index, cpu, mem, prio, ext amounts, mask); s: the
    enforced group or None.  None when the node is no candidate, else ((max prio, sum, count), victims in the walk's
    order)."""
    pot = sorted((e for e in seg if e[3] < prio), key=lambda e: (-e[3], e[0]))
    bit = (lambda e: (e[5] >> s) & 1) if s is not None else (lambda e: 0)
    free = [wrap(alloc[0] + sum(e[1] for e in pot)), wrap(alloc[1] + sum(e[2] for e in pot)), wrap(alloc[2] + len(pot))]
    fext = [wrap(x + sum(e[4][r] for e in pot)) for r, x in enumerate(ext)]
    rem = sum(bit(e) for e in pot)
    if not elig(req, req_ext, free, fext, rem, sp, sel, lab, use_labels):
        return None
    victims = []
    for e in pot:
        less = [wrap(free[0] - e[1]), wrap(free[1] - e[2]), wrap(free[2] - 1)]
        lext = [wrap(f - v) for f, v in zip(fext, e[4])]
        if elig(req, req_ext, less, lext, rem - bit(e), sp, sel, lab, use_labels):
            free, fext, rem = less, lext, rem - bit(e)
        else:
            victims.append(e[0])
    by = {e[0]: e[3] for e in seg}
    mx = max((by[t] for t in victims), default=NO_VICTIM_PRIO)
    return (mx, wrap(sum(by[t] + (1 << 31) for t in victims)), len(victims)), victims


def preempt(c, vcap, spread=True, ext=True, labels=None, selector=None, prio=None, detail=False):
    """The six columns of ksched_preempt_constrained on case c (spread / ext False: that argument NULL).  detail: also
    the per-(pod, node) candidate matrix."""
    ac, am, ap = (np.asarray(x) for x in c.alloc)
    bn, bc, bm, bp = (np.asarray(x) for x in c.bound)
    rc, rm, rp, pr = (np.asarray(x) for x in c.pods)
    if prio is not None:
        pr = np.asarray(prio)
    n, m = len(ac), len(rc)
    R = c.node_ext.shape[0] if ext else 0
    use_labels = labels is not None
    segs = {j: [] for j in range(n)}
    for t in range(len(bn)):
        segs[int(bn[t])].append((t, int(bc[t]), int(bm[t]), int(bp[t]), tuple(int(c.bound_ext[r, t]) for r in range(R)),
                                 int(c.bound_spread[t]) if spread else 0))
    D = c.counts.shape[1]
    node = np.full(m, NO_FIT, np.int32); nv = np.zeros(m, np.int32); mx = np.full(m, NO_VICTIM_PRIO, np.int32)
    sm = np.zeros(m, np.int64); cand = np.zeros(m, np.int32); vic = np.full((m, vcap), -1, np.int32)
    is_cand = np.zeros((m, n), bool)
    others = {}  # (s, d) -> the smallest loaded count of the other domains

    def min_others(s, d):
        if (s, d) not in others:
            others[s, d] = int(np.delete(c.counts[s], d).min())
        return others[s, d]
    for i in range(m):
        best = None
        req = (int(rc[i]), int(rm[i]), int(rp[i]))
        rx = tuple(int(c.req_ext[r, i]) for r in range(R))
        s = int(c.group[i]) if spread and c.group[i] >= 0 and c.enforce[i] else None
        for j in range(n):
            sp = None
            if s is not None:
                d = int(c.node_domain[j])
                row = c.counts[s]
                mo = None if D == 1 or d < 0 else min_others(s, d)
                sp = (d, int(row[d]) if d >= 0 else 0, mo, int(c.skew[s]))
            r = node_key(req, rx, int(pr[i]), (int(ac[j]), int(am[j]), int(ap[j])),
                         tuple(int(c.node_ext[q, j]) for q in range(R)), segs[j], sp, s,
                         int(selector[i]) if use_labels else 0, int(labels[j]) if use_labels else 0, use_labels)
            if r is None:
                continue
            cand[i] += 1
            is_cand[i, j] = True
            if best is None or r[0] < best[0]:  # strict: the lowest index keeps a tie
                best = (r[0], j, r[1])
        if best is not None:
            (mx[i], sm[i], nv[i]), j, victims = best
            node[i] = j
            vic[i, :min(vcap, len(victims))] = victims[:vcap]
    out = (node, nv, mx, sm, cand, vic)
    return out + (is_cand,) if detail else out


def head(c, m):
    """Case c with its first m pods only."""
    return dataclasses.replace(c, pods=tuple(p[:m] for p in c.pods), req_ext=c.req_ext[:, :m], group=c.group[:m],
                               enforce=c.enforce[:m])


def changed(a, b):
    """Pods whose row differs between two answers."""
    return int(sum(any((x[i] != y[i]).any() if x.ndim > 1 else x[i] != y[i] for x, y in zip(a[:6], b[:6])) for i in range(len(a[0]))))


def worked_example():
    """include/ksched.h's worked example: tests/test_preempt_host.py's cluster with one gpu column and one spread group."""
    alloc = (np.array([400, 0, 400]), np.full(3, 1 << 20), np.full(3, 10))
    bound = (np.array([2, 0, 1, 0, 1, 2], np.int32), np.array([500, 600, 500, 500, 500, 600]), np.zeros(6, np.int64),
             np.array([100, 200, 200, 100, 50, 200], np.int32))
    pods = (np.array([1000, 1000, 400, 400]), np.zeros(4, np.int64), np.ones(4, np.int64), np.array([1000, 150, 1000, 1000], np.int32))
    return Case(alloc, bound, pods, node_ext=np.array([[0, 0, 1]], np.int64), bound_ext=np.array([[1, 1, 0, 1, 1, 0]], np.int64),
                req_ext=np.array([[2, 0, 0, 0]], np.int64), node_domain=np.array([0, 1, 0], np.int32),
                skew=np.array([1], np.int32), counts=np.array([[3, 2]], np.int32),
                bound_spread=np.array([1, 0, 1, 1, 1, 0], np.uint64), group=np.array([-1, -1, 0, 0], np.int32),
                enforce=np.array([1, 1, 1, 0], np.uint8))


WORKED = dict(node=[0, -1, 1, 0], nvictims=[2, 0, 1, 0], max_prio=[200, NO_VICTIM_PRIO, 50, NO_VICTIM_PRIO],
              sum_prio=[4294967596, 0, 2147483698, 0], candidates=[2, 0, 3, 3], victims=[[1, 3], [-1, -1], [4, -1], [-1, -1]])
