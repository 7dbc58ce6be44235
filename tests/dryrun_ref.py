"""Shared by the ksched_rank_full / ksched_explain_full tests: the CPU restatement of the dry runs under constraints.
Per pod the FailedScheduling codes of include/ksched.h are computed in numpy, in its order -- cpu, memory, pods, labels,
the extended columns, the spread key, the spread skew, the pod's affinity term, its own anti-affinity, the bound pods'
anti-affinity -- against a Tables value: the node rows and the three tables as they stand.  The ranked list is
oracle.local_topk's, with "code 0" folded into its label check through free label bit 62 (full_ref's trick), one call
per pod since the labels differ per pod: every score is the oracle's, bit for bit.  The reason column of the ranked
entries and the histogram come from the numpy codes."""
import dataclasses

import numpy as np

import full_ref as FR

FREE_BIT = FR.FREE_BIT
U0 = np.uint64(0)
NUM_REASONS_FULL = 14
EXT0, SPREAD_NO_KEY, SPREAD_SKEW, AFFINITY, ANTI_AFFINITY, EXISTING_ANTI_AFFINITY = 5, 9, 10, 11, 12, 13


@dataclasses.dataclass
class Tables:
    """What a dry run reads: the node rows and, where the constraint is loaded, the spread counts [S, D], the extended
    columns [R, n] and the three affinity node arrays."""
    state: tuple
    counts: object = None
    ext: object = None
    words: object = None  # (node_member, node_anti_host, node_anti_zone)


def initial(c):
    """The rows and tables of case c (a full_ref.Case) before any pod is scheduled."""
    cl = c.cl
    return Tables((cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods), c.counts if c.group is not None else None,
                  c.node_ext if c.req_ext is not None else None, c.aff_table()[1:] if c.member is not None else None)


def after(ref):
    """The rows and tables full_ref.schedule_full left (its result tuple)."""
    return Tables(ref[6], ref[5], ref[4], None if ref[8] is None else tuple(ref[8:11]))


def worked_example():
    """include/ksched.h's example: the end state of ksched_schedule_full's own worked example (its cluster with one pod
    slot taken on n0, n1 and n2; counts A 2, B 1; gpu column {0, 0, 1, 0}; node_member = node_anti_host = {1, 1, 0, 0})
    and the four pods X, Y, Z, W.  Returns (case, tables); Y has no spread group and Z, W no extended request -- a zero
    request is not checked."""
    base = FR.worked_example()
    cl = dataclasses.replace(base.cl, name="dryrun-example", req_cpu=np.full(4, 100, np.int64),
                             req_mem=np.zeros(4, np.int64), req_pods=np.ones(4, np.int64))
    train, z = np.array([1, 1, 1, 0], np.uint64), np.zeros(4, np.uint64)
    c = dataclasses.replace(base, cl=cl, gang_off=None, gang_min=None, group=np.array([0, -1, -1, 0], np.int32),
                            enforce=np.ones(4, np.uint8), req_ext=np.array([[1, 0, 0, 0]], np.int64),
                            member=train, anti_host=np.array([1, 1, 0, 0], np.uint64), anti_zone=z,
                            aff_group=np.array([0, 0, -1, -1], np.int32), aff_zone=np.array([1, 1, 0, 0], np.uint8))
    w = np.array([1, 1, 0, 0], np.uint64)
    t = Tables((cl.alloc_cpu - np.array([100, 100, 100, 0]), cl.alloc_mem, np.array([109, 109, 109, 110], np.int64)), np.array([[2, 1]], np.int32),
               np.array([[0, 0, 1, 0]], np.int64), (w, w.copy(), z.copy()))
    return c, t


def codes(c, i, t):
    """Pod i of case c against t: (reason uint8[n], waived) -- the first failing check per node, 0: eligible."""
    cl = c.cl
    n = cl.n_nodes
    r = np.zeros(n, np.uint8)

    def first(mask, code):
        r[(r == 0) & mask] = code

    a0, a1, a2 = (np.asarray(x, np.int64) for x in t.state)
    first(a0 < cl.req_cpu[i], 1); first(a1 < cl.req_mem[i], 2); first(a2 < cl.req_pods[i], 3)
    if cl.use_labels:
        sel = np.uint64(cl.selector[i])
        first((np.asarray(cl.labels, np.uint64) & sel) != sel, 4)
    if c.req_ext is not None:
        ext = np.asarray(t.ext, np.int64)
        for col in range(ext.shape[0]):
            q = int(c.req_ext[col][i])
            if q != 0:
                first(q > ext[col], EXT0 + col)
    if c.group is not None and c.group[i] >= 0 and (c.enforce is None or c.enforce[i]):
        s = int(c.group[i])
        dom = np.asarray(c.node_domain, np.int64)
        cnt = np.asarray(t.counts, np.int64)[s]
        first(dom < 0, SPREAD_NO_KEY)
        first((dom >= 0) & (cnt[np.where(dom >= 0, dom, 0)] + 1 - cnt.min() > int(c.max_skew[s])), SPREAD_SKEW)
    waived = False
    if c.member is not None:
        nm, nah, naz = (np.asarray(x, np.uint64) for x in t.words)
        adom = np.full(n, -1, np.int64) if c.aff_domain is None else np.asarray(c.aff_domain, np.int64)
        ahas = adom >= 0
        adz = np.where(ahas, adom, 0)
        zm, za = np.zeros(max(int(c.aff_D), 1), np.uint64), np.zeros(max(int(c.aff_D), 1), np.uint64)
        np.bitwise_or.at(zm, adom[ahas], nm[ahas])
        np.bitwise_or.at(za, adom[ahas], naz[ahas])
        any_host = np.bitwise_or.reduce(nm) if n else U0
        any_zone = np.bitwise_or.reduce(zm)
        mem, ah, az = np.uint64(c.member[i]), np.uint64(c.anti_host[i]), np.uint64(c.anti_zone[i])
        ag, zs = int(c.aff_group[i]), bool(c.aff_zone[i])
        if ag >= 0:
            a = np.uint64(1) << np.uint64(ag)
            if not (a & (any_zone if zs else any_host)) and (a & mem):
                waived = True
            else:
                first(~((ahas & ((zm[adz] & a) != 0)) if zs else ((nm & a) != 0)), AFFINITY)
        first(~(((nm & ah) == 0) & (~ahas | ((zm[adz] & az) == 0))), ANTI_AFFINITY)
        first(~(((nah & mem) == 0) & (~ahas | ((za[adz] & mem) == 0))), EXISTING_ANTI_AFFINITY)
    return r, waived


def rank_full(O, c, k, t=None, pods=None):
    """ksched_rank_full of pods `pods` (None: all) of case c against t (None: initial(c)).  Returns ((idx[m, k], score
    bits int64[m, k], reason[m, k], count[m], feasible[m], reason_counts int64[m, 14]), per-node codes uint8[m, n],
    waived bool[m])."""
    cl = c.cl
    t = initial(c) if t is None else t
    pods = range(cl.n_pods) if pods is None else pods
    m, n = len(pods), cl.n_nodes
    idx = np.full((m, k), -1, np.int32); score = np.zeros((m, k), np.float64); reason = np.zeros((m, k), np.uint8)
    count = np.zeros(m, np.int32); feas = np.zeros(m, np.int32); hist = np.zeros((m, NUM_REASONS_FULL), np.int64)
    per_node = np.zeros((m, n), np.uint8); waived = np.zeros(m, bool)
    base_lab = np.zeros(n, np.uint64) if cl.labels is None else np.asarray(cl.labels, np.uint64)
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    price = None if cl.price is None else np.ascontiguousarray(cl.price)
    for row, i in enumerate(pods):
        r, waived[row] = codes(c, i, t)
        per_node[row] = r
        hist[row] = np.bincount(r, minlength=NUM_REASONS_FULL)
        if n == 0:
            continue
        sel = U0 if cl.selector is None or not cl.use_labels else np.uint64(cl.selector[i])
        lab, use = base_lab, cl.use_labels
        if (r >= EXT0).any():
            # a node is left to the oracle's own predicate unless a constraint refuses it: codes 1-4 are the oracle's too
            assert not (base_lab & FREE_BIT).any() and not (sel & FREE_BIT)
            lab, sel, use = base_lab | np.where(r < EXT0, FREE_BIT, U0), sel | FREE_BIT, True
        recs, fc = O.local_topk((cl.priority, cl.domain, use), k, 0, i64(t.state[0]), i64(t.state[1]), i64(t.state[2]),
                                np.ascontiguousarray(lab), price, i64(cl.req_cpu[i:i + 1]), i64(cl.req_mem[i:i + 1]),
                                i64(cl.req_pods[i:i + 1]), np.array([sel], np.uint64))
        assert int(fc[0]) == int(hist[row, 0]), (i, int(fc[0]), int(hist[row, 0]))
        rr = recs.reshape(k)
        valid = rr["valid"] != 0
        idx[row] = np.where(valid, rr["idx"], -1)
        score[row] = np.where(valid, rr["key"] if cl.priority == 0 else 0.0 - rr["key"], 0.0)
        reason[row, valid] = r[idx[row, valid]]
        count[row], feas[row] = valid.sum(), fc[0]
    return (idx, np.ascontiguousarray(score).view(np.int64), reason, count, feas, hist), per_node, waived


def same(got, ref):
    """got: an Engine.rank_full result; ref: rank_full()[0].  Every column, scores by bit pattern."""
    names = ("idx", "score", "reason", "count", "feasible", "reason_counts")
    g = (got[0], np.ascontiguousarray(got[1]).view(np.int64)) + tuple(got[2:])
    for nm, a, b in zip(names, g, ref):
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
