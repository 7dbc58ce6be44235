"""Shared by the ksched_schedule_full tests: the CPU restatement of gangs, topology spread, extended resources and
inter-pod affinity in one run, built on constrained_ref, affinity_ref and the oracle as they are.  Gang by gang: the node
rows, the extended-resource table, the spread counts and every affinity word (the three node arrays, the zone words and
the any words) are snapshotted at the gang's start; per member the combined eligibility mask of include/ksched.h's rule
(spread_ok && ext_ok && affinity_ok) is computed in numpy and folded into the oracle's label check through free label
bit 62, oracle.schedule places that one pod against the running state -- so every score is the oracle's, bit for bit --
and the member's commits are made in numpy; at the gang's end the state is kept or the snapshot restored.

skip_undo: a deliberately WRONG reference that leaves the named kinds of affinity word ("node", "zone", "any") as the
rejected gang set them.  The tests use it on the CPU only, to prove that a case can see each kind of missing undo."""
import dataclasses

import numpy as np

import affinity_ref as AR
import constrained_ref as CR

FREE_BIT = CR.FREE_BIT
GANG_REJECTED = CR.GANG_REJECTED
U0 = np.uint64(0)


@dataclasses.dataclass
class Case(CR.Case):
    """One input of ksched_schedule_full: constrained_ref.Case and the affinity table and pod words of
    affinity_ref.Case; affinity is off where member is None.  aff_domain is the affinity table's own zone key (None: no
    zone key), independent of the spread table's node_domain."""
    aff_D: int = 0
    aff_domain: object = None
    node_member: object = None
    node_anti_host: object = None
    node_anti_zone: object = None
    member: object = None
    anti_host: object = None
    anti_zone: object = None
    aff_group: object = None
    aff_zone: object = None

    def aff_table(self):
        return self.aff_domain, self.node_member, self.node_anti_host, self.node_anti_zone

    def aff_pods(self):
        return self.member, self.anti_host, self.anti_zone, self.aff_group, self.aff_zone


def worked_example():
    """include/ksched.h's example: best-price, feasible domain; n0 (zone A, 0.1, gpu 1), n1 (A, 0.2, gpu 1), n2 (B, 0.3,
    gpu 1), n3 (B, 0.4, gpu 0), both tables on the same zones; one spread group, max_skew 1, counts 0: p0-p4 count, p5
    enforces; group train = bit 0, an empty table; gangs {p0, p1, p2}, {p3, p4}, {p5}, every member required; p0-p4:
    member train, anti_host train, affinity train at zone scope, gpu 1; p5: no words, gpu 0."""
    from ksched import cluster
    cl = cluster.Cluster(
        name="full-example", alloc_cpu=np.full(4, 64000, np.int64), alloc_mem=np.full(4, 1 << 30, np.int64),
        alloc_pods=np.full(4, 110, np.int64), req_cpu=np.full(6, 100, np.int64), req_mem=np.zeros(6, np.int64),
        req_pods=np.ones(6, np.int64), price=np.array([0.1, 0.2, 0.3, 0.4], np.float32),
        priority=cluster.PRIORITY_BEST_PRICE, domain=cluster.DOMAIN_FEASIBLE)
    zones = np.array([0, 0, 1, 1], np.int32)
    z = np.zeros(4, np.uint64)
    train = np.array([1, 1, 1, 1, 1, 0], np.uint64)
    return Case(cl, gang_off=np.array([0, 3, 5, 6], np.int64), node_domain=zones, max_skew=np.array([1], np.int32),
                counts=np.zeros((1, 2), np.int32), group=np.zeros(6, np.int32),
                enforce=np.array([0, 0, 0, 0, 0, 1], np.uint8), node_ext=np.array([[1, 1, 1, 0]], np.int64),
                req_ext=np.array([[1, 1, 1, 1, 1, 0]], np.int64), aff_D=2, aff_domain=zones.copy(), node_member=z,
                node_anti_host=z.copy(), node_anti_zone=z.copy(), member=train, anti_host=train.copy(),
                anti_zone=np.zeros(6, np.uint64), aff_group=np.array([0, 0, 0, 0, 0, -1], np.int32),
                aff_zone=np.array([1, 1, 1, 1, 1, 0], np.uint8))


def adversarial(n, p, S_aff=12, D_aff=3, aff_seed=7, **kw):
    """constrained_ref.adversarial(n, p, **kw) composed with the table and pod words of affinity_ref.adversarial(aff_seed,
    n, p, D_aff, S_aff, ...) under the same priority, domain and labels.  The affinity table's zones are that generator's
    own (shuffled, every 11th node without the key): a key different from the spread table's."""
    c = CR.adversarial(n, p, **kw)
    a = AR.adversarial(aff_seed, n, p, D_aff, S_aff, kw.get("priority", 0), kw.get("domain", 0), kw.get("labels", False))
    return Case(**{f.name: getattr(c, f.name) for f in dataclasses.fields(CR.Case)}, aff_D=D_aff, aff_domain=a.node_domain,
                node_member=a.node_member, node_anti_host=a.node_anti_host, node_anti_zone=a.node_anti_zone,
                member=a.member, anti_host=a.anti_host, anti_zone=a.anti_zone, aff_group=a.aff_group, aff_zone=a.aff_zone)


def without_affinity(c):
    """c with affinity off, as a constrained_ref.Case."""
    return CR.Case(**{f.name: getattr(c, f.name) for f in dataclasses.fields(CR.Case)})


def affinity_only(c):
    """c's cluster, affinity table and pod words as an affinity_ref.Case (every other constraint dropped)."""
    return AR.Case(c.cl, c.aff_D, c.aff_domain, c.node_member, c.node_anti_host, c.node_anti_zone, c.member, c.anti_host,
                   c.anti_zone, c.aff_group, c.aff_zone)


def pods(c, lo, hi):
    """Pods [lo, hi) of case c as a case of their own (the gangs are not sliced: pass gang_off for the slice)."""
    sub = CR.pods(c, lo, hi)
    cut = lambda x: None if x is None else x[lo:hi]
    return dataclasses.replace(sub, member=cut(c.member), anti_host=cut(c.anti_host), anti_zone=cut(c.anti_zone),
                               aff_group=cut(c.aff_group), aff_zone=cut(c.aff_zone))


def schedule_full(O, c, state=None, table=None, skip_undo=()):
    """Case c from the node rows `state` (None: the cluster's), c's spread and ext tables and the affinity node arrays
    `table` (None: c's).  Returns (idx int32[p], score f64[p], feasible int32[p], gang_placed int32[g] (empty without
    gangs), final ext int64[R, n] | None, final counts int32[S, D] | None, final (cpu, mem, pods), info, final
    node_member, node_anti_host, node_anti_zone uint64[n] | None).  info counts: rejected gangs, rejected gangs that undid
    a commit (rollbacks), accepted gangs with a failed member (partial), rejected gangs that had taken an extended column
    (undo_ext), raised a count (undo_spread), changed a node word (undo_node_word), a zone word (undo_zone_word), an any
    word (undo_any); the nodes of the rolled-back winners, one entry per rolled-back member, in rolled_nodes, and of those
    whose member carried an affinity word -- the slots whose words the undo restores -- in rolled_aff_nodes; waivers
    granted (waived), and of those the ones for a (group, scope) whose earlier waiver a rolled-back gang had spent
    (rewaived); pods with a fitting node lost to the affinity clause only (aff_narrowed)."""
    cl = c.cl
    p, n = cl.n_pods, cl.n_nodes
    skip_undo = frozenset(skip_undo)
    assert skip_undo <= {"node", "zone", "any"}
    off = np.arange(p + 1, dtype=np.int64) if c.gang_off is None else np.asarray(c.gang_off, np.int64)
    ng = off.shape[0] - 1
    assert off[0] == 0 and off[ng] == p and np.all(np.diff(off) > 0)
    spread, extd, aff = c.group is not None, c.req_ext is not None, c.member is not None
    cnt = ext = None
    if spread:
        dom = np.asarray(c.node_domain, np.int64)
        cnt = np.array(c.counts, np.int64)
        D = cnt.shape[1]
        assert D > dom.max() and set(range(D)) <= set(dom.tolist()), "domain ids must be compact and carried"
        has_key = dom >= 0
        group = np.asarray(c.group, np.int64)
        enforce = np.ones(p, bool) if c.enforce is None else np.asarray(c.enforce) != 0
    if extd:
        ext = np.array(c.node_ext, np.int64)
        req = np.asarray(c.req_ext, np.int64)
        assert ext.shape[1] == n and req.shape == (ext.shape[0], p) and (req >= 0).all()
    nm = nah = naz = None
    if aff:
        adom = np.full(n, -1, np.int64) if c.aff_domain is None else np.asarray(c.aff_domain, np.int64)
        AD = int(c.aff_D)
        assert adom.min(initial=-1) >= -1 and adom.max(initial=-1) < AD and set(range(AD)) <= set(adom.tolist())
        nm, nah, naz = (np.array(x, np.uint64) for x in (c.aff_table()[1:] if table is None else table))
        ahas = adom >= 0
        adz = np.where(ahas, adom, 0)
        zm, za = np.zeros(max(AD, 1), np.uint64), np.zeros(max(AD, 1), np.uint64)
        np.bitwise_or.at(zm, adom[ahas], nm[ahas])
        np.bitwise_or.at(za, adom[ahas], naz[ahas])
        any_host = np.bitwise_or.reduce(nm) if n else U0
        any_zone = np.bitwise_or.reduce(zm)
    base_lab = np.zeros(n, np.uint64) if cl.labels is None else np.asarray(cl.labels, np.uint64)
    assert not (base_lab & FREE_BIT).any()
    assert cl.selector is None or not (np.asarray(cl.selector, np.uint64) & FREE_BIT).any()
    state = tuple(np.ascontiguousarray(x, dtype=np.int64).copy()
                  for x in ((cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods) if state is None else state))
    idx = np.empty(p, np.int32); score = np.empty(p, np.float64); feas = np.empty(p, np.int32)
    placed = np.zeros(ng, np.int32)
    info = dict(rejected=0, rollbacks=0, partial=0, undo_ext=0, undo_spread=0, undo_node_word=0, undo_zone_word=0,
                undo_any=0, waived=0, rewaived=0, aff_narrowed=0, rolled_nodes=[], rolled_aff_nodes=[])
    spent_rolled = set()  # (group, zone scope) of waivers granted inside gangs that were then rolled back
    for g in range(ng):
        lo, hi = int(off[g]), int(off[g + 1])
        snap = (state, None if ext is None else ext.copy(), None if cnt is None else cnt.copy())
        if aff:
            asnap = (nm.copy(), nah.copy(), naz.copy(), zm.copy(), za.copy(), any_host, any_zone)
        took_ext = raised = False
        waivers = []
        for i in range(lo, hi):
            sel = U0 if cl.selector is None or not cl.use_labels else np.uint64(cl.selector[i])
            one = dict(alloc_cpu=state[0], alloc_mem=state[1], alloc_pods=state[2], req_cpu=cl.req_cpu[i:i + 1],
                       req_mem=cl.req_mem[i:i + 1], req_pods=cl.req_pods[i:i + 1],
                       selector=None if cl.selector is None else cl.selector[i:i + 1])
            fit = (state[0] >= cl.req_cpu[i]) & (state[1] >= cl.req_mem[i]) & (state[2] >= cl.req_pods[i])
            if cl.use_labels:
                fit &= (base_lab & sel) == sel
            ok = np.ones(n, bool)
            s = int(group[i]) if spread else -1
            if s >= 0 and enforce[i]:
                ok &= has_key & (cnt[s][np.where(has_key, dom, 0)] + 1 - cnt[s].min() <= int(c.max_skew[s]))
            q = req[:, i] if extd else None
            if extd and (q != 0).any():
                ok &= ((q[:, None] == 0) | (q[:, None] <= ext)).all(axis=0)
            if aff:
                mem, ah, az = np.uint64(c.member[i]), np.uint64(c.anti_host[i]), np.uint64(c.anti_zone[i])
                ag, zs = int(c.aff_group[i]), bool(c.aff_zone[i])
                if mem or ah or az or ag >= 0:
                    c1 = ((nm & ah) == 0) & (~ahas | ((zm[adz] & az) == 0))
                    c2 = ((nah & mem) == 0) & (~ahas | ((za[adz] & mem) == 0))
                    c3 = np.ones(n, bool)
                    if ag >= 0:
                        a = np.uint64(1) << np.uint64(ag)
                        if not (a & (any_zone if zs else any_host)) and (a & mem):
                            info["waived"] += 1
                            info["rewaived"] += (ag, zs) in spent_rolled
                            spent_rolled.discard((ag, zs))
                            waivers.append((ag, zs))
                        else:
                            c3 = (ahas & ((zm[adz] & a) != 0)) if zs else ((nm & a) != 0)
                    info["aff_narrowed"] += bool((fit & ok & c1 & c2 & ~c3).any())
                    ok &= c1 & c2 & c3
            if ok.all():
                oi, os_, of, after = O.schedule(dataclasses.replace(cl, **one))
            else:
                one["selector"] = np.array([sel | FREE_BIT], np.uint64)
                oi, os_, of, after = O.schedule(dataclasses.replace(
                    cl, labels=base_lab | np.where(ok, FREE_BIT, U0), use_labels=True, **one))
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
                if aff:
                    nm[w] |= mem; nah[w] |= ah; naz[w] |= az
                    any_host |= mem
                    if adom[w] >= 0:
                        zm[adom[w]] |= mem; za[adom[w]] |= az
                        any_zone |= mem
        n_placed = int((idx[lo:hi] >= 0).sum())
        need = hi - lo if c.gang_min is None or c.gang_off is None else int(c.gang_min[g])
        if n_placed >= need:
            placed[g] = n_placed
            info["partial"] += n_placed < hi - lo
        else:
            for i in range(lo, hi):
                if idx[i] >= 0:
                    info["rolled_nodes"].append(int(idx[i]))
                    if aff and (c.member[i] or c.anti_host[i] or c.anti_zone[i] or c.aff_group[i] >= 0):
                        info["rolled_aff_nodes"].append(int(idx[i]))
            idx[lo:hi] = np.where(idx[lo:hi] >= 0, GANG_REJECTED, idx[lo:hi])
            score[lo:hi] = 0.0
            info["rejected"] += 1
            info["rollbacks"] += n_placed > 0
            info["undo_ext"] += took_ext
            info["undo_spread"] += raised
            state, ext, cnt = snap
            if aff:
                differs = lambda xs, ys: any((x != y).any() for x, y in zip(xs, ys))
                info["undo_node_word"] += differs((nm, nah, naz), asnap[:3])
                info["undo_zone_word"] += differs((zm, za), asnap[3:5])
                info["undo_any"] += bool(any_host != asnap[5] or any_zone != asnap[6])
                if n_placed > 0:
                    spent_rolled.update(waivers)
                if "node" not in skip_undo:
                    nm, nah, naz = asnap[:3]
                if "zone" not in skip_undo:
                    zm, za = asnap[3:5]
                if "any" not in skip_undo:
                    any_host, any_zone = asnap[5:]
    if c.gang_off is None:
        placed = placed[:0]
    return (idx, score, feas, placed, ext, None if cnt is None else cnt.astype(np.int32), state, info, nm, nah, naz)


def diff(ref, mutant):
    """Pods whose idx or feasible differs between two results of schedule_full."""
    return int(((ref[0] != mutant[0]) | (ref[2] != mutant[2])).sum())


def same(got, got_ext, got_counts, got_table, got_state, ref):
    """got: Engine.schedule_full's result; got_ext / got_counts / got_table: Engine.read_ext() / read_spread() /
    read_affinity() (None where the constraint is off); got_state: Engine.read_nodes() after it; ref: schedule_full()
    above.  Every column exactly, scores by bit pattern."""
    CR.same(got, got_ext, got_counts, got_state, ref)
    assert (got_table is None) == (ref[8] is None), "affinity table"
    if got_table is not None:
        for nm, a, b in zip(("node_member", "node_anti_host", "node_anti_zone"), got_table, ref[8:11]):
            assert a.shape == b.shape, (nm, a.shape, b.shape)
            bad = np.argwhere(a != b)
            assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
