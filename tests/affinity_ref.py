"""Shared by the ksched_schedule_affinity tests: the CPU restatement of required inter-pod affinity and anti-affinity,
built on the oracle as it is.  Per pod the eligibility mask of include/ksched.h's three clauses is computed in numpy and
folded into the oracle's label check -- a label bit the cluster does not use is ORed into the eligible nodes' labels
and into the pod's selector -- and oracle.schedule places that one pod against the running state, so every score is
the oracle's, bit for bit.  The words of the table are kept in numpy."""
import dataclasses
from typing import Optional

import numpy as np

AFF_BIT = np.uint64(1 << 62)  # free: ksched.cluster.random_small uses bits 0-7 and 63
U0 = np.uint64(0)


@dataclasses.dataclass
class Case:
    """One input: the cluster, the table (node_domain None: no zone key) and the pods' words."""
    cl: object
    D: int
    node_domain: Optional[np.ndarray]
    node_member: np.ndarray
    node_anti_host: np.ndarray
    node_anti_zone: np.ndarray
    member: np.ndarray
    anti_host: np.ndarray
    anti_zone: np.ndarray
    aff_group: np.ndarray
    aff_zone: np.ndarray

    def table(self):
        return self.node_domain, self.node_member, self.node_anti_host, self.node_anti_zone

    def pods(self, lo=0, hi=None):
        return tuple(x[lo:hi] for x in (self.member, self.anti_host, self.anti_zone, self.aff_group, self.aff_zone))


def worked_example():
    """include/ksched.h's example: best-price, feasible domain, ample room; n0 (zone A, 0.1), n1 (B, 0.2), n2 (A, 0.3),
    n3 (no key, 0.4); web = bit 0, cache = bit 1, db = bit 2; an empty table; nine pods."""
    from ksched import cluster
    WEB, CACHE, DB = 1, 2, 4
    #          member anti_host anti_zone aff_group aff_zone
    pods = [(WEB, WEB, 0, -1, 0), (WEB, WEB, 0, -1, 0),
            (CACHE, 0, CACHE, 0, 1), (CACHE, 0, CACHE, 0, 1), (CACHE, 0, CACHE, 0, 1),
            (WEB, WEB, 0, -1, 0), (WEB, 0, 0, -1, 0), (DB, 0, 0, 2, 0), (DB, 0, 0, 2, 1)]
    p = len(pods)
    cl = cluster.Cluster(
        name="affinity-example", alloc_cpu=np.full(4, 64000, np.int64), alloc_mem=np.full(4, 1 << 30, np.int64),
        alloc_pods=np.full(4, 110, np.int64), req_cpu=np.full(p, 100, np.int64), req_mem=np.zeros(p, np.int64),
        req_pods=np.ones(p, np.int64), price=np.array([0.1, 0.2, 0.3, 0.4], np.float32),
        priority=cluster.PRIORITY_BEST_PRICE, domain=cluster.DOMAIN_FEASIBLE)
    col = lambda k, t: np.array([x[k] for x in pods], t)
    z = np.zeros(4, np.uint64)
    return Case(cl, 2, np.array([0, 1, 0, -1], np.int32), z, z.copy(), z.copy(), col(0, np.uint64), col(1, np.uint64),
                col(2, np.uint64), col(3, np.int32), col(4, np.uint8))


def _pods(rng, p, S, p_member, p_anti_host, p_anti_zone, p_aff, zone_share, self_share, zones=True):
    """Random pod words over S groups: a pod is in one group (p_member), names one group per anti scope (p_anti_host,
    p_anti_zone) and carries one affinity term (p_aff) -- towards its own group (self_share: the waiver's case) or any
    -- at zone scope (zone_share).  zones False: host scope only."""
    bit = lambda g: np.uint64(1) << g.astype(np.uint64)
    own = rng.integers(0, S, p)
    member = np.where(rng.random(p) < p_member, bit(own), U0)
    anti_host = np.where(rng.random(p) < p_anti_host, bit(rng.integers(0, S, p)), U0)
    anti_zone = np.where((rng.random(p) < p_anti_zone) & zones, bit(rng.integers(0, S, p)), U0)
    to_self = (rng.random(p) < self_share) & (member != 0)
    aff_group = np.where(rng.random(p) < p_aff, np.where(to_self, own, rng.integers(0, S, p)), -1).astype(np.int32)
    aff_zone = ((rng.random(p) < zone_share) & zones).astype(np.uint8)
    return member, anti_host, anti_zone, aff_group, aff_zone


def _domains(rng, n, D):
    """Shuffled domains, every 11th node without the key (where its domain keeps another carrier)."""
    dom = (np.arange(n) % D).astype(np.int32)
    rng.shuffle(dom)
    for j in range(0, n, 11):
        if (dom == dom[j]).sum() > 1:
            dom[j] = -1
    return dom


def adversarial(seed, n, p, D, S, priority=0, domain=0, labels=False):
    """random_small(7, n, p) under shuffled domains, every 11th node without the key, a random pre-bound table and random
    members, terms and scopes (the table: one node in 20 with a member bit, one in 25 / 50 with an anti bit, so that the
    pods and not the table fill the zone words).  D == 0: no zone key (node_domain None, host scope only)."""
    from ksched import cluster
    rng = np.random.default_rng(seed + 3000)
    cl = cluster.random_small(7, n, p, priority=priority, domain=domain, use_labels=labels)
    dom = _domains(rng, n, D) if D > 0 else None
    # (the last group has no bound pod: its first self-affine pod is the waiver's case)
    sparse = lambda q: np.where(rng.random(n) < q, np.uint64(1) << rng.integers(0, max(S - 1, 1), n).astype(np.uint64), U0)
    nm, nah, naz = sparse(0.05), sparse(0.04), sparse(0.02 if D > 0 else 0.0)
    member, anti_host, anti_zone, aff_group, aff_zone = _pods(rng, p, S, 0.7, 0.15, 0.06, 0.35, 0.5, 0.5, zones=D > 0)
    # pod 0 is self-affine to the last group, which nothing is bound to yet: the waiver, whatever the draw
    member[0] = np.uint64(1) << np.uint64(S - 1)
    aff_group[0] = S - 1
    return Case(cl, D, dom, nm, nah, naz, member, anti_host, anti_zone, aff_group, aff_zone)


def healthy(seed, n, p, D, S):
    """Roomy nodes and small pods (resource priority, feasible domain), so the constraint and not the resources
    decides; the first D nodes carry zones 0..D-1, the rest any of [-1, D); an empty table."""
    from ksched import cluster
    rng = np.random.default_rng(seed + 4000)
    cl = cluster.Cluster(
        name=f"healthy{seed}", alloc_cpu=rng.choice(np.array([4000, 8000, 16000], np.int64), size=n),
        alloc_mem=np.full(n, 64 << 20, np.int64), alloc_pods=np.full(n, 110, np.int64),
        req_cpu=rng.choice(np.array([100, 250, 500], np.int64), size=p),
        req_mem=rng.choice(np.array([1024, 65536], np.int64), size=p), req_pods=np.ones(p, np.int64),
        priority=cluster.PRIORITY_RESOURCE, domain=cluster.DOMAIN_FEASIBLE)
    dom = np.concatenate([np.arange(D), rng.integers(-1, D, n - D)]).astype(np.int32)
    z = np.zeros(n, np.uint64)
    return Case(cl, D, dom, z, z.copy(), z.copy(), *_pods(rng, p, S, 0.9, 0.3, 0.1, 0.4, 0.6, 0.6))


def schedule_affinity(O, c, state=None, table=None):
    """Returns (idx int32[p], score f64[p], feasible int32[p], final node_member, node_anti_host, node_anti_zone
    uint64[n], final (cpu, mem, pods), info).  state / table: the rows / the three node arrays to start from (the
    case's by default).  info counts pods: own_anti (a fitting node lost to clause 1), symmetric (one lost to clause 2
    only), aff_narrowed (one lost to clause 3 only), waived, aff_nofit (fitting nodes but no eligible one), zone_moved
    (placements that added a bit to a zone word; zone_moved_at lists their pods), off_domain (a pod with a group placed on a node without the key),
    moved (the pick differs from the pick with the constraint off, same state)."""
    cl = c.cl
    n, p = cl.n_nodes, cl.n_pods
    dom = np.full(n, -1, np.int64) if c.node_domain is None else np.asarray(c.node_domain, np.int64)
    D = int(c.D)
    assert dom.min(initial=-1) >= -1 and dom.max(initial=-1) < D and set(range(D)) <= set(dom.tolist())
    nm, nah, naz = (np.array(x, np.uint64) for x in (c.table()[1:] if table is None else table))
    has = dom >= 0
    dz = np.where(has, dom, 0)
    zm, za = np.zeros(max(D, 1), np.uint64), np.zeros(max(D, 1), np.uint64)
    np.bitwise_or.at(zm, dom[has], nm[has])
    np.bitwise_or.at(za, dom[has], naz[has])
    any_host = np.bitwise_or.reduce(nm) if n else U0
    any_zone = np.bitwise_or.reduce(zm)
    base_lab = np.zeros(n, np.uint64) if cl.labels is None else np.asarray(cl.labels, np.uint64)
    assert not (base_lab & AFF_BIT).any()
    assert cl.selector is None or not (np.asarray(cl.selector, np.uint64) & AFF_BIT).any()
    state = tuple(np.ascontiguousarray(x, dtype=np.int64).copy()
                  for x in ((cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods) if state is None else state))
    idx = np.empty(p, np.int32); score = np.empty(p, np.float64); feas = np.empty(p, np.int32)
    info = dict(own_anti=0, symmetric=0, aff_narrowed=0, waived=0, aff_nofit=0, zone_moved=0, off_domain=0, moved=0)
    moved_at = []  # the pods behind zone_moved
    for i in range(p):
        mem, ah, az = np.uint64(c.member[i]), np.uint64(c.anti_host[i]), np.uint64(c.anti_zone[i])
        g, zs = int(c.aff_group[i]), bool(c.aff_zone[i])
        sel = U0 if cl.selector is None or not cl.use_labels else np.uint64(cl.selector[i])
        one = dict(alloc_cpu=state[0], alloc_mem=state[1], alloc_pods=state[2], req_cpu=cl.req_cpu[i:i + 1],
                   req_mem=cl.req_mem[i:i + 1], req_pods=cl.req_pods[i:i + 1],
                   selector=None if cl.selector is None else cl.selector[i:i + 1])
        plain = dataclasses.replace(cl, **one)
        if mem or ah or az or g >= 0:
            fit = (state[0] >= cl.req_cpu[i]) & (state[1] >= cl.req_mem[i]) & (state[2] >= cl.req_pods[i])
            if cl.use_labels:
                fit &= (base_lab & sel) == sel
            c1 = ((nm & ah) == 0) & (~has | ((zm[dz] & az) == 0))
            c2 = ((nah & mem) == 0) & (~has | ((za[dz] & mem) == 0))
            c3 = np.ones(n, bool)
            if g >= 0:
                a = np.uint64(1) << np.uint64(g)
                if not (a & (any_zone if zs else any_host)) and (a & mem):
                    info["waived"] += 1
                else:
                    c3 = (has & ((zm[dz] & a) != 0)) if zs else ((nm & a) != 0)
            ok = c1 & c2 & c3
            elig = fit & ok
            one["selector"] = np.array([sel | AFF_BIT], np.uint64)
            sub = dataclasses.replace(cl, labels=base_lab | np.where(ok, AFF_BIT, U0), use_labels=True, **one)
            oi, os_, of, after = O.schedule(sub)
            assert int(of[0]) == int(elig.sum()), (i, int(of[0]), int(elig.sum()))
            info["own_anti"] += bool((fit & ~c1).any())
            info["symmetric"] += bool((fit & c1 & c3 & ~c2).any())
            info["aff_narrowed"] += bool((fit & c1 & c2 & ~c3).any())
            info["aff_nofit"] += not elig.any() and bool(fit.any())
            info["moved"] += int(O.schedule(plain)[0][0]) != int(oi[0])
        else:
            oi, os_, of, after = O.schedule(plain)
        idx[i], score[i], feas[i] = oi[0], os_[0], of[0]
        state = after
        w = int(oi[0])
        if w >= 0:
            nm[w] |= mem; nah[w] |= ah; naz[w] |= az
            any_host |= mem
            if dom[w] >= 0:
                d = dom[w]
                if (mem & ~zm[d]) | (az & ~za[d]):
                    info["zone_moved"] += 1
                    moved_at.append(i)
                zm[d] |= mem; za[d] |= az
                any_zone |= mem
            else:
                info["off_domain"] += bool(mem)
    info["zone_moved_at"] = moved_at
    return idx, score, feas, nm, nah, naz, state, info


def same(got, got_table, got_state, ref):
    """got: Engine.schedule_affinity's result, got_table: Engine.read_affinity(), got_state: Engine.read_nodes() after
    it, ref: schedule_affinity() above.  Every column exactly, scores by bit pattern."""
    names = ("idx", "score", "feasible", "node_member", "node_anti_host", "node_anti_zone", "cpu", "mem", "pods")
    g = (got[0], np.ascontiguousarray(got[1]).view(np.int64), got[2]) + tuple(got_table) + tuple(got_state)
    r = (ref[0], np.ascontiguousarray(ref[1]).view(np.int64), ref[2]) + tuple(ref[3:6]) + tuple(ref[6])
    for nm, a, b in zip(names, g, r):
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
