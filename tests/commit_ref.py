"""CPU statements and case generators of the list-consuming stages run alone (ksched_selftest_rank_merge and
ksched_selftest_commit in include/ksched.h): the rank merge k_merge and the two commits k_commit / k_commit_spc.

commit_ref is the rule of oracle/cpu_ref.c's commit_batch_impl with the touched table pre-filled from the inherited
export as in commit_inherit and with an EXPLICIT cut flag per pod (the oracle infers "cut" from a full list, so it
cannot state a cut list shorter than K); rank_merge_ref is the comment above k_merge.  Keys and predicate counts are
never restated: they come from the oracle's own pair_key / fits, reached through oracle.local_topk over the touched
nodes' states.  State arithmetic is Python ints with an explicit 64-bit wrap.

tests/test_commit_ref_host.py anchors both statements to the oracle and asserts the generators' coverage on the CPU;
tests/test_gpu_commit_alone.py compares the device with them."""
import dataclasses

import numpy as np

NO_IDX = 0x7FFFFFFF
NO_FIT, NO_POSITIVE_SCORE = -1, -2
COMMIT_SEQUENTIAL, COMMIT_SPECULATIVE = 1, 3
PRIO_RESOURCE, PRIO_PRICE = 0, 1
DOM_ALL, DOM_FEASIBLE = 0, 1

XREC_DTYPE = np.dtype([("idx", "<i4"), ("pad", "<i4"), ("cur", "<i8", 3), ("sb", "<i8", 3), ("labels", "<u8"),
                       ("price", "<f4"), ("pad2", "<i4"), ("pad3", "<i8")])
assert XREC_DTYPE.itemsize == 80
XHDR_BYTES = 16

KS = (4, 8, 16)
# (kernel, batch size): k_commit_spc at 64, k_commit at 48 and 128 -- and k_commit at 64 on the speculative kernel's
# own cases, so that the two kernels are also compared with each other
CONFIGS = ((COMMIT_SPECULATIVE, 64), (COMMIT_SEQUENTIAL, 64), (COMMIT_SEQUENTIAL, 48), (COMMIT_SEQUENTIAL, 128))
BATCHES = (64, 48, 128)
# the dispatch ladder (KSCHED_DISPATCH): (priority, domain), labels, fast53
LADDER = [(p, d, lab, f53) for (p, d) in ((PRIO_RESOURCE, DOM_ALL), (PRIO_RESOURCE, DOM_FEASIBLE), (PRIO_PRICE, DOM_FEASIBLE))
          for lab in (False, True) for f53 in (False, True)]
REMAPS = ("identity", "spc", "thash", "low16")
FAMILIES = ("natural", "truncate", "short", "same", "stops", "beaten", "inherit", "every0", "flip")
MERGE_RANKS = (1, 2, 3, 8, 64)


def wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def better(ka, ia, kb, ib):
    """the candidate order everywhere: key descending, then node index ascending"""
    return ka > kb or (ka == kb and ia < ib)


def touched_beats_untouched(tk, ti, uk, ui):
    """the one comparison between t* and u* (a name of its own so that a test can flip its tie-break alone)"""
    return better(tk, ti, uk, ui)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


# ---- the commit's statement ---------------------------------------------------------------------------------------
class _Touched:
    """the touched table: numpy columns (what the oracle reads) beside Python-int states (what the commit updates)"""

    def __init__(self, cap):
        self.n = 0
        self.idx = np.zeros(cap, np.int64)
        self.cur = np.zeros((3, cap), np.int64)
        self.s0 = np.zeros((3, cap), np.int64)
        self.sb = [None] * cap
        self.labels = np.zeros(cap, np.uint64)
        self.price = np.zeros(cap, np.float32)
        self.mine = [False] * cap
        self.slot = {}
        self.order = np.zeros(0, np.int64)

    def open(self, idx, s0, sb, cur, labels, price):
        t = self.n
        self.n += 1
        self.idx[t] = idx
        for r in range(3):
            self.s0[r, t] = s0[r]
            self.cur[r, t] = cur[r]
        self.sb[t] = tuple(int(v) for v in sb)
        self.labels[t] = labels
        self.price[t] = price
        self.slot[int(idx)] = t
        self.order = np.argsort(self.idx[:self.n], kind="stable")  # by node index: ties then break by position
        return t


def _best_and_count(O, opts, T, which, rc, rm, rp, sel):
    """the oracle over the touched nodes at state `which`: (its best eligible node as (key, slot) or None, how many
    fit) -- pair_key and fits are the oracle's, the order (key descending, index ascending) is local_topk's"""
    od = T.order
    st = T.cur if which == "cur" else T.s0
    lab = np.ascontiguousarray(T.labels[od]) if opts[2] else None
    pr = np.ascontiguousarray(T.price[od]) if opts[0] == PRIO_PRICE else None
    recs, fc = O.local_topk(opts, 1, 0, np.ascontiguousarray(st[0, od]), np.ascontiguousarray(st[1, od]),
                            np.ascontiguousarray(st[2, od]), lab, pr, _c64([rc]), _c64([rm]), _c64([rp]),
                            np.array([sel], np.uint64) if opts[2] else None)
    best = (float(recs["key"][0]), int(od[int(recs["idx"][0])])) if recs["valid"][0] else None
    return best, int(fc[0])


def commit_trace(O, opts, K, pods, lists, cut, fc0, xin):
    """commit_ref and what it passed through: per pod its kind -- 'list' (winner from the list), 'touched' (a node
    this batch touched before), 'inherited' (a slot of xin), 'nofit', 'nofit_delta' (only the touched nodes' deltas
    brought the count to 0), 'nopos' -- whether a cut list was exhausted and the best touched node beat its last entry
    ('beaten'), and the touched table in slot order."""
    rc, rm, rp, sel = pods
    nb = len(rc)
    lists = lists.reshape(nb, K)
    T = _Touched(len(xin) + nb + 1)
    for x in xin:
        cur = [int(v) for v in x["cur"]]
        T.open(int(x["idx"]), [int(v) for v in x["sb"]], cur, cur, x["labels"], x["price"])
    nin = T.n
    idx = np.full(nb, NO_FIT, np.int32)
    score = np.zeros(nb, np.float64)
    feas = np.zeros(nb, np.int32)
    kinds, beaten, neg_wins, done, flip1 = [], [], [], nb, False
    for i in range(nb):
        r = (int(rc[i]), int(rm[i]), int(rp[i]))
        s = int(sel[i]) if (opts[2] and sel is not None) else 0
        tbest, fc = None, int(fc0[i])
        if T.n:
            tbest, f1 = _best_and_count(O, opts, T, "cur", *r, s)
            fc += f1 - _best_and_count(O, opts, T, "s0", *r, s)[1]
        feas[i] = np.int64(fc).astype(np.int32)
        if fc == 0:
            idx[i], score[i] = NO_FIT, 0.0
            kinds.append("nofit" if int(fc0[i]) == 0 else "nofit_delta")
            neg_wins.append(False)
            flip1 = flip1 or int(fc0[i]) == 1  # its only feasible node was filled by an earlier pod
            beaten.append(False)
            continue
        L = lists[i]
        cnt = 0
        while cnt < K and L["valid"][cnt]:
            cnt += 1
        u = next((q for q in range(cnt) if int(L["idx"][q]) not in T.slot), None)
        tk, ti = (tbest[0], int(T.idx[tbest[1]])) if tbest else (None, None)
        win, beat = None, False  # win: ('t', slot, key) or ('u', q, key)
        if u is not None:
            uk, ui = float(L["key"][u]), int(L["idx"][u])
            win = ("t", tbest[1], tk) if tbest and touched_beats_untouched(tk, ti, uk, ui) else ("u", u, uk)
        elif not cut[i]:
            win = ("t", tbest[1], tk) if tbest else None
        else:
            assert cnt > 0, "a cut list keeps at least its cutoff entry"
            if tbest and better(tk, ti, float(L["key"][cnt - 1]), int(L["idx"][cnt - 1])):
                win, beat = ("t", tbest[1], tk), True
            else:
                done = i  # the best untouched node may lie beyond the list: the batch stops before pod i
                break
        beaten.append(beat)
        if win is None:
            idx[i], score[i] = NO_POSITIVE_SCORE, 0.0
            kinds.append("nopos")
            continue
        if win[0] == "u":
            e = L[win[1]]
            a = [int(e["a_cpu"]), int(e["a_mem"]), int(e["a_pods"])]
            t = T.open(int(e["idx"]), a, a, a, e["labels"], e["price"])
            kinds.append("list")
        else:
            t = win[1]
            kinds.append("inherited" if t < nin and not T.mine[t] else "touched")
            neg_wins.append(bool((T.cur[:, t] < 0).any()))  # chosen, so keyed, at a state already driven negative
        T.mine[t] = True
        for k, d in enumerate((r[0], r[1], 1)):
            T.cur[k, t] = wrap64(int(T.cur[k, t]) - d)
        idx[i] = T.idx[t]
        score[i] = 0.0 - win[2] if opts[0] == PRIO_PRICE else win[2]
    mine = [t for t in range(T.n) if T.mine[t]]
    xout = np.zeros(len(mine), XREC_DTYPE)
    for o, t in zip(xout, mine):
        o["idx"] = T.idx[t]
        o["cur"] = T.cur[:, t]
        o["sb"] = T.sb[t]
        o["labels"] = T.labels[t]
        o["price"] = T.price[t]
    xout = xout[np.argsort(xout["idx"], kind="stable")]
    return dict(done=done, idx=idx, score=score, feas=feas, xout=xout, kinds=kinds, beaten=beaten, nin=nin,
                neg_wins=any(neg_wins), flip1=flip1, table=[int(v) for v in T.idx[:T.n]])


def commit_ref(O, opts, K, pods, lists, cut, fc0, xin):
    """(done, idx, score, feas, xout) of ONE commit of the batch `pods` = (rc, rm, rp, sel) over `lists`
    (oracle.REC_DTYPE [nb * K]) with the explicit cut flags `cut`, the lists' feasible counts `fc0` and the inherited
    export `xin` (XREC_DTYPE).  opts = (priority, domain, use_labels).  Pods at or past `done` are unspecified.  xout
    holds every slot a pod of this batch committed to, sorted by node index."""
    t = commit_trace(O, opts, K, pods, lists, cut, fc0, xin)
    return t["done"], t["idx"], t["score"], t["feas"], t["xout"]


def commit_stats(done, idx, nb):
    """Ctl after the commit: [cursor, batches committed, truncated, pods placed, the plan of batch 2]"""
    trunc = done < nb
    return [done, 1, int(trunc), int((idx[:done] >= 0).sum()), done if trunc else -1]


# ---- the rank merge's statement -----------------------------------------------------------------------------------
def _invalid_rec(O):
    r = np.zeros((), O.REC_DTYPE)
    r["key"] = -np.inf
    r["idx"] = NO_IDX
    return r


def rank_merge_ref(O, K, blocks):
    """blocks: per rank (recs REC_DTYPE [nb * K] with the cut flag in entry 0's pad, fc [nb]).  K rounds of best head
    over the R sorted lists; fc is the sum of the input counts; the output is cut when an input was, or when entries
    were left over; every output entry that the best cutoff (the best last valid entry over the cut inputs) ranks
    strictly above is dropped.  (recs [nb * K] with the flag in entry 0's pad, cut [nb], fc [nb])"""
    nb = len(blocks[0][1])
    out = np.zeros(nb * K, O.REC_DTYPE).reshape(nb, K)
    cut = np.zeros(nb, np.int32)
    fc = np.zeros(nb, np.int64)
    for b in range(nb):
        ls = [blk[0].reshape(nb, K)[b] for blk in blocks]
        n = [int(np.count_nonzero(l["valid"])) for l in ls]
        for l, c in zip(ls, n):
            assert l["valid"][:c].all(), "valid entries first"
        fc[b] = sum(int(blk[1][b]) for blk in blocks)
        anycut = any(int(l["pad"][0]) != 0 for l in ls)
        ck, ci = -np.inf, NO_IDX
        for l, c in zip(ls, n):
            if int(l["pad"][0]) != 0 and c > 0 and better(float(l["key"][c - 1]), int(l["idx"][c - 1]), ck, ci):
                ck, ci = float(l["key"][c - 1]), int(l["idx"][c - 1])
        head = [0] * len(ls)
        for q in range(K):
            br = None
            for r, l in enumerate(ls):
                if head[r] < n[r] and (br is None or better(float(l["key"][head[r]]), int(l["idx"][head[r]]),
                                                            float(ls[br]["key"][head[br]]), int(ls[br]["idx"][head[br]]))):
                    br = r
            e = _invalid_rec(O)
            if br is not None:
                e = ls[br][head[br]].copy()
                head[br] += 1
                if anycut and better(ck, ci, float(e["key"]), int(e["idx"])):
                    e = _invalid_rec(O)  # below the best cutoff: an unlisted candidate could precede it
            out[b, q] = e
            out[b, q]["pad"] = 0
        left = any(head[r] < n[r] for r in range(len(ls)))
        cut[b] = 1 if (anycut or left) else 0
        out[b, 0]["pad"] = cut[b]
    return out.reshape(-1), cut, fc


# ---- the hashes of the two touched sets, and their probe sequences ----------------------------------------------
def spc_hash(idx):
    return (np.asarray(idx).astype(np.uint32) * np.uint32(2654435761)) >> np.uint32(32 - 11)


def thash(idx):
    return (np.asarray(idx).astype(np.uint32) * np.uint32(2654435761)) >> np.uint32(32 - 9)


def probe_table(keys, hashes, size, reserved=None):
    """open addressing with linear probing as spc_pos_insert / touched_insert do it (position `reserved` is never
    used): (distinct keys stored, the longest probe sequence of an insertion)"""
    slots, longest = {}, 0
    for k, h in zip(keys, hashes):
        h, steps = int(h), 1
        while True:
            if h != reserved:
                if h not in slots:
                    slots[h] = k
                    break
                if slots[h] == k:
                    break
            h = (h + 1) % size
            steps += 1
            assert steps <= size, "the table is full"
        longest = max(longest, steps)
    return len(slots), longest


def table_stats(case, trace):
    """the two kernels' tables for one case, emulated: k_commit_spc hashes every valid list entry and the inherited
    export (11 bits, position 2047 reserved), k_commit the inherited export and every slot the batch opens (9 bits)"""
    L = case.lists
    spc_keys = [int(v) for v in L["idx"][L["valid"] != 0]] + [int(v) for v in case.xin["idx"]]
    n_spc, c_spc = probe_table(spc_keys, spc_hash(np.array(spc_keys, np.int64)), 2048, 2047)
    n_t, c_t = probe_table(trace["table"], thash(np.array(trace["table"], np.int64)), 512)
    assert n_spc <= 64 * case.K + 64 <= 2047 and n_t <= 2 * case.B <= 512
    return dict(spc_chain=c_spc, thash_chain=c_t, spc_entries=n_spc, thash_entries=n_t)


_MAPS = {}


def index_map(kind, n=1200):
    """a strictly increasing map of node indices 0..n-1 into [0, 2^31 - 2]: every tie-break survives it"""
    if kind == "identity":
        return np.arange(n, dtype=np.int64)
    if kind not in _MAPS:
        if kind == "low16":  # pairwise equal in their low 16 bits: every index aliases in k_commit's filter
            m = 0x1234 + np.arange(n, dtype=np.int64) * 65536
        else:
            cand = np.arange(7, (1 << 31) - 1, 521, dtype=np.int64)
            if kind == "spc":  # around the reserved position 2047 and the wrap to 0
                hit = np.isin(spc_hash(cand), [2044, 2045, 2046, 2047, 0, 1])
            else:
                hit = np.isin(thash(cand), [510, 511, 0])
            cand = cand[hit]
            m = cand[np.linspace(0, cand.size - 1, n).astype(np.int64)]
        assert m.size == n and (np.diff(m) > 0).all() and m[0] >= 0 and m[-1] <= (1 << 31) - 2
        _MAPS[kind] = m
    return _MAPS[kind]


# ---- cases --------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    family: str
    seed: int
    K: int
    B: int
    nb: int
    opts: tuple          # (priority, domain, use_labels)
    f53: bool
    remap: str
    pods: tuple          # rc, rm, rp, sel
    lists: np.ndarray    # REC_DTYPE [nb * K], the cut flag in entry 0's pad
    cut: np.ndarray
    fc0: np.ndarray
    xin: np.ndarray      # XREC_DTYPE

    @property
    def name(self):
        p, d, lab = self.opts
        return (f"{self.family} seed={self.seed} K={self.K} B={self.B} nb={self.nb} prio={p} dom={d} lab={int(lab)} "
                f"f53={int(self.f53)} remap={self.remap}")


class _Universe:
    """a small node universe (at most 1200 nodes) and a pool of pods over it"""

    def __init__(self, opts, ac, am, ap, labels, price, rc, rm, rp, sel):
        self.opts = opts
        self.ac, self.am, self.ap = _c64(ac), _c64(am), _c64(ap)
        self.labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint64)
        self.price = None if price is None else np.ascontiguousarray(price, dtype=np.float32)
        self.rc, self.rm, self.rp = _c64(rc), _c64(rm), _c64(rp)
        self.sel = None if sel is None else np.ascontiguousarray(sel, dtype=np.uint64)
        assert self.ac.size <= 1200

    def pods(self, sl):
        sel = np.zeros(len(self.rc[sl]), np.uint64) if self.sel is None else np.ascontiguousarray(self.sel[sl])
        return (np.ascontiguousarray(self.rc[sl]), np.ascontiguousarray(self.rm[sl]), np.ascontiguousarray(self.rp[sl]), sel)

    def topk(self, O, K, pods, lo=0, hi=None):
        hi = self.ac.size if hi is None else hi
        return O.local_topk(self.opts, K, lo, self.ac[lo:hi].copy(), self.am[lo:hi].copy(), self.ap[lo:hi].copy(),
                            None if self.labels is None else self.labels[lo:hi].copy(),
                            None if self.price is None else self.price[lo:hi].copy(), pods[0], pods[1], pods[2],
                            pods[3] if self.opts[2] else None)

    def xrec(self, j, cur):
        x = np.zeros((), XREC_DTYPE)
        x["idx"] = j
        x["sb"] = (self.ac[j], self.am[j], self.ap[j])
        x["cur"] = cur
        x["labels"] = 0 if self.labels is None else self.labels[j]
        x["price"] = 0 if self.price is None else self.price[j]
        return x


def _random_universe(seed, n, npods, opts, f53):
    """states and pods from ksched.cluster.random_small's edge generators.  Its huge values (2^53 and up) break
    fast53's precondition, so under f53 they are left out and the same share of nodes and pods gets values that
    keep every reachable magnitude below 2^52 instead: allocatables of 2^51 + 3, 2^50 + 1 and -2^40, requests of -5
    and 2^20 + 1"""
    from ksched import cluster
    cl = cluster.random_small(seed, n_nodes=n, n_pods=npods, priority=opts[0], domain=opts[1], use_labels=opts[2],
                              edge=not f53)
    if f53:
        rng = np.random.default_rng([seed, n, 53])
        kn, kp = max(1, n // 16), max(1, npods // 32)
        cl.alloc_cpu[rng.integers(0, n, size=kn)] = rng.choice(np.array([(1 << 51) + 3, (1 << 50) + 1, -(1 << 40)], dtype=np.int64), size=kn)
        cl.req_cpu[rng.integers(0, npods, size=kp)] = rng.choice(np.array([-5, (1 << 20) + 1], dtype=np.int64), size=kp)
    return _Universe(opts, cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, cl.labels, cl.price, cl.req_cpu, cl.req_mem,
                     cl.req_pods, cl.selector)


def _crafted(opts, rng, nodes, npods, pod=(100, 65536, 1), zero_mix=False):
    """nodes: rows (cpu, mem, pods, price); identical pods, every third one without cpu / memory when zero_mix"""
    nodes = np.array(nodes, dtype=np.float64)
    n = nodes.shape[0]
    i = np.arange(npods)
    z = (i % 3 == 0) if zero_mix else np.zeros(npods, bool)
    full = np.uint64((1 << 63) | 0xFF)
    return _Universe(opts, nodes[:, 0].astype(np.int64), nodes[:, 1].astype(np.int64), nodes[:, 2].astype(np.int64),
                     np.full(n, full, np.uint64) if opts[2] else None,
                     nodes[:, 3].astype(np.float32) if opts[0] == PRIO_PRICE else None,
                     np.where(z, 0, pod[0]), np.where(z, 0, pod[1]), np.full(npods, pod[2]),
                     rng.choice(np.array([0, 1, 3, (1 << 63) | 1], dtype=np.uint64), size=npods) if opts[2] else None)


def _true_lists(O, u, K, pods):
    """the universe's true lists: cut exactly as the oracle infers it, from a full list"""
    recs, fc = u.topk(O, K, pods)
    cut = (recs["valid"].reshape(-1, K) != 0).all(axis=1).astype(np.int32)
    return recs, cut, fc


def _export_of(O, u, K, pods):
    """the export of a previous batch over the same universe: commit_ref on its true lists"""
    if len(pods[0]) == 0:
        return np.zeros(0, XREC_DTYPE)
    recs, cut, fc = _true_lists(O, u, K, pods)
    return commit_ref(O, u.opts, K, pods, recs, cut, fc, np.zeros(0, XREC_DTYPE))[4]


def _history(O, u, count):
    """an export of exactly `count` nodes (fewer if the universe gives no more): the sequential schedule of the pool's
    pods up to the pod that touches the count-th distinct node; sb is the universe's state, cur the state after"""
    import types
    cl = types.SimpleNamespace(alloc_cpu=u.ac, alloc_mem=u.am, alloc_pods=u.ap, req_cpu=u.rc, req_mem=u.rm, req_pods=u.rp,
                               labels=u.labels, selector=u.sel, price=u.price, priority=u.opts[0], domain=u.opts[1],
                               use_labels=u.opts[2], n_pods=len(u.rc))
    oi = O.schedule(cl)[0]
    cur = {}
    for i, j in enumerate(oi):
        j = int(j)
        if j < 0:
            continue
        if j not in cur:
            if len(cur) == count:
                break
            cur[j] = [int(u.ac[j]), int(u.am[j]), int(u.ap[j])]
        for k, d in enumerate((int(u.rc[i]), int(u.rm[i]), 1)):
            cur[j][k] = wrap64(cur[j][k] - d)
    return np.array([u.xrec(j, c) for j, c in sorted(cur.items())], XREC_DTYPE).reshape(-1)


def _truncate(recs, cut, K, b, c):
    """keep the first c entries of pod b's list and flag it cut: everything unlisted ranks below entry c - 1"""
    L = recs.reshape(-1, K)
    assert 1 <= c <= int(np.count_nonzero(L["valid"][b]))
    keep = L[b, :c].copy()
    L[b] = np.zeros((), recs.dtype)
    L["idx"][b] = -1
    L[b, :c] = keep
    cut[b] = 1


def make_case(O, family, seed, K, B, nb, variant, remap, sub):
    """sub in 0..11 picks a family's sub-variants: sub // 3 independently of nb (which follows sub % 3); the two-way
    pick follows the ladder's labels bit at K = 4 and 16 and its complement at K = 8"""
    prio, dom, lab, f53 = variant
    pick4, pick3, pick2 = sub // 3, (sub // 3) % 3, (sub // 2 + K // 8) % 2
    opts = (prio, dom, bool(lab))
    rng = np.random.default_rng([seed, K, B, nb])
    big = 64 << 20
    trunc = []  # (pod, entries kept)
    if family in ("natural", "truncate"):
        u = _random_universe(seed, 300, 2 * B, opts, f53)
        xin = _export_of(O, u, K, u.pods(slice(0, (0, 1, B // 2, B)[pick4])))
        pods = u.pods(slice(B, B + nb))
    elif family == "short":
        if pick3 == 0 and prio == PRIO_RESOURCE:  # nodes that fit exactly: feasible, key 0, so no list entry at all
            u = _crafted(opts, rng, [(100, 65536, 1, 1.0)] * 5, B + 2)
        else:  # fewer than K eligible nodes
            u = _random_universe(seed, int(rng.integers(1, K)), 2 * B, opts, f53)
        xin = _export_of(O, u, K, u.pods(slice(0, 0 if pick3 == 0 else pick2 + 1)))
        pods = u.pods(slice(B, B + nb)) if len(u.rc) >= 2 * B else u.pods(slice(2, 2 + nb))
    elif family in ("same", "stops"):
        n = (K - 1, K, 2 * K + 1)[pick3] if family == "same" else K - 1  # stops: uncut lists but the one below
        # same: identical pods on identical nodes, in half of the cases with zero-request pods mixed in
        zero_mix = family == "same" and (sub // 3 + sub) % 2 == 0
        u = _crafted(opts, rng, [(4000, 8388608, 110, 1.5)] * n, B + 3, pod=(200, 65536, 1), zero_mix=zero_mix)
        xin = _export_of(O, u, K, u.pods(slice(0, 3 if (family == "stops" or pick2) else 0)))
        pods = u.pods(slice(3, 3 + nb))
        if family == "stops":  # entry 0 is inherited: cut after it, the batch stops at this pod
            trunc = [((0, nb - 1, nb // 2)[pick3], 1)]
    elif family == "beaten":
        nodes = [(64000, big, 110, 1.0), (4000, 8 << 20, 110, 2.0)] + [(500, 1 << 20, 110, 3.0 + q) for q in range(K + 1)]
        u = _crafted(opts, rng, nodes, B)
        xin = np.array([u.xrec(0, (64000 - 100, big - 65536, 109)), u.xrec(1, (4000 - 100, (8 << 20) - 65536, 109))], XREC_DTYPE)
        pods = u.pods(slice(0, nb))
        trunc = [(b, 2) for b in range(nb)]
    elif family == "inherit":
        # a full export.  The universe is 300 nodes twice over and the export the history of a run over the first half
        # alone, so that every listed node it touched has an untouched twin further down the lists: the batch goes on
        # to open slots of its own beside the inherited ones
        h = _random_universe(seed, 300, 6 * B, opts, f53)
        twice = lambda a: None if a is None else np.concatenate([a, a])
        u = _Universe(opts, twice(h.ac), twice(h.am), twice(h.ap), twice(h.labels), twice(h.price), h.rc, h.rm, h.rp, h.sel)
        cap = min(B, 64) if pick2 == 0 or B <= 64 else B  # 64 for either kernel, 128 for k_commit at 128
        pods = u.pods(slice(5 * B, 5 * B + nb))
        recs0 = u.topk(O, K, pods)[0]
        listed = set(int(v) for v in recs0["idx"][recs0["valid"] != 0])
        xin = _history(O, h, cap - 2)
        have = set(int(v) for v in xin["idx"])
        free = [j for j in range(u.ac.size) if j not in listed and j not in have][:cap - len(xin)]
        extra = [u.xrec(j, (wrap64(int(u.ac[j]) - 50), wrap64(int(u.am[j]) - 1024), wrap64(int(u.ap[j]) - 1))) for j in free]
        xin = np.concatenate([xin, np.array(extra, XREC_DTYPE).reshape(-1)])  # ... two of them nodes in no list
        xin = xin[np.argsort(xin["idx"])]
    elif family == "every0":
        base = _random_universe(seed, 200, 2 * B, opts, f53)
        ac, am, ap = base.ac.copy(), base.am.copy(), base.ap.copy()
        ac[7], am[7], ap[7] = 1 << 30, 1 << 40, 1 << 20  # one node that every pod ranks first
        labels, price = base.labels, base.price
        if labels is not None:
            labels = labels.copy(); labels[7] = np.uint64((1 << 63) | 0xFF)
        if price is not None:
            price = price.copy(); price[7] = 0.125
        u = _Universe(opts, ac, am, ap, labels, price, base.rc, base.rm, base.rp, base.sel)
        xin = _export_of(O, u, K, u.pods(slice(0, 2)))
        pods = u.pods(slice(B, B + nb))
    elif family == "flip":
        if pick2 == 0:  # one feasible node, room for one pod: the second pod's count reaches 0 by the delta alone
            nodes = [(50, big, 110, 2.0)] * 3 + [(150, big, 110, 1.0)] + [(50, big, 110, 2.0)] * 3
        else:  # nodes one pod fills, beside nodes that fit exactly (feasible, key 0): the count stays positive while the
               # filled nodes are driven negative -- keyed still in the all-node domain, ineligible in the feasible one
            nodes = [(150, big, 110, 1.0)] * (K - 1) + [(100, 65536, 1, 2.0)] * 4
        u = _crafted(opts, rng, nodes, B)
        xin = np.zeros(0, XREC_DTYPE)
        pods = u.pods(slice(0, nb))
    else:
        raise ValueError(family)
    recs, cut, fc0 = _true_lists(O, u, K, pods)
    if family == "truncate":
        cnt = np.count_nonzero(recs["valid"].reshape(-1, K), axis=1)
        trunc = [(b, int(rng.integers(1, cnt[b] + 1))) for b in range(nb) if cnt[b] and rng.random() < 0.6]
        if cnt[nb - 1]:
            trunc.append((nb - 1, 1))
    for b, c in trunc:
        if np.count_nonzero(recs["valid"].reshape(-1, K)[b]) >= c:
            _truncate(recs, cut, K, b, c)
    recs["pad"] = 0
    recs["pad"].reshape(-1, K)[:, 0] = cut
    m = index_map(remap)
    v = recs["valid"] != 0
    recs["idx"][v] = m[recs["idx"][v]]
    xin = xin.copy()
    xin["idx"] = m[xin["idx"]]
    assert len(xin) <= min(B, 64) or (B > 64 and len(xin) <= B)
    return Case(family, seed, K, B, nb, opts, bool(f53), remap, pods, recs, cut, _c64(fc0), xin)


_CASES = {}


def commit_cases(O, B):
    """every family for every K, every nb in {1, 37, B} and each of the ladder's 12 variants; the 4 index maps are
    cycled over the variants and shifted with nb, so that each family and K also meets every (nb, map) pair;
    deterministic"""
    if B not in _CASES:
        out = []
        for fi, fam in enumerate(FAMILIES):
            for ki, K in enumerate(KS):
                for ni, nb in enumerate((1, 37, B)):
                    for j, variant in enumerate(LADDER):
                        out.append(make_case(O, fam, 100 * fi + 12 * ki + j, K, B, nb, variant, REMAPS[(j + ni) % 4], j))
        _CASES[B] = out
    return _CASES[B]


_TRACES = {}


def case_trace(O, case):
    key = (case.family, case.seed, case.K, case.B, case.nb)
    if key not in _TRACES:
        _TRACES[key] = commit_trace(O, case.opts, case.K, case.pods, case.lists, case.cut, case.fc0, case.xin)
    return _TRACES[key]


OUTCOMES = ("list", "touched", "inherited", "nofit_delta", "nopos", "stop_first", "stop_last", "stop_between",
            "beaten_complete")


def outcomes(case, t):
    """which of the coverage conditions' outcomes one case shows"""
    got = set(t["kinds"]) & set(OUTCOMES)
    d, nb = t["done"], case.nb
    if d < nb:
        got.add("stop_first" if d == 0 else "stop_last" if d == nb - 1 else "stop_between")  # (nb = 1: the first only)
    elif any(t["beaten"]):
        got.add("beaten_complete")
    return got


# ---- the rank merge's cases --------------------------------------------------------------------------------------
@dataclasses.dataclass
class MergeCase:
    kind: str
    seed: int
    K: int
    R: int
    nb: int
    blocks: list      # per rank (recs, fc)
    whole: tuple      # the unsharded universe's (recs, fc) for the same pods, or None
    universe: object
    pods: tuple

    @property
    def name(self):
        return f"merge {self.kind} seed={self.seed} K={self.K} R={self.R} nb={self.nb}"


def make_merge_case(O, kind, seed, K, R, nb=9):
    """R contiguous shards of one universe (some of them empty), their true lists, then: 'plain' as they are (no input
    cut: full shard lists are not flagged, as oracle.merge_topk reads them), 'ties' identical nodes so that keys differ
    only by index across ranks, 'cut1' / 'cutall' one / every non-empty input truncated and flagged, 'full' every full
    input flagged cut as the real pipeline does"""
    rng = np.random.default_rng([seed, K, R])
    opts = ((PRIO_RESOURCE, DOM_ALL, False), (PRIO_RESOURCE, DOM_FEASIBLE, True), (PRIO_PRICE, DOM_FEASIBLE, False))[seed % 3]
    if kind == "ties":
        u = _crafted(opts, rng, [(4000, 8388608, 110, 1.5)] * max(2 * R, 3 * K), nb, zero_mix=True)
    else:
        u = _random_universe(seed, max(40, min(1200, 3 * R)), nb, opts, False)
    n = u.ac.size
    bounds = np.sort(rng.integers(0, n + 1, size=R - 1)) if R > 1 else np.zeros(0, np.int64)
    if R >= 3:
        bounds[1] = bounds[0]  # an empty rank
    bounds = np.concatenate([[0], bounds, [n]]).astype(np.int64)
    pods = u.pods(slice(0, nb))
    blocks = []
    for r in range(R):
        recs, fc = u.topk(O, K, pods, int(bounds[r]), int(bounds[r + 1]))
        recs["pad"] = 0
        blocks.append((recs, fc))
    full = lambda recs, b: bool((recs["valid"].reshape(nb, K)[b] != 0).all())
    for b in range(nb):
        nonempty = [r for r in range(R) if blocks[r][0]["valid"].reshape(nb, K)[b, 0]]
        if kind in ("cut1", "cutall") and nonempty:
            for r in (nonempty if kind == "cutall" else [nonempty[int(rng.integers(len(nonempty)))]]):
                cnt = int(np.count_nonzero(blocks[r][0]["valid"].reshape(nb, K)[b]))
                cut = np.zeros(nb, np.int32)
                _truncate(blocks[r][0], cut, K, b, int(rng.integers(1, cnt + 1)))
                blocks[r][0]["pad"].reshape(nb, K)[b, 0] = 1
        elif kind == "full":
            for r in nonempty:
                if full(blocks[r][0], b):
                    blocks[r][0]["pad"].reshape(nb, K)[b, 0] = 1
    whole = u.topk(O, K, pods)
    return MergeCase(kind, seed, K, R, nb, blocks, whole, u, pods)


MERGE_KINDS = ("plain", "ties", "cut1", "cutall", "full")
_MERGE = []


def merge_cases(O):
    if not _MERGE:
        s = 0
        for K in KS:
            for R in MERGE_RANKS:
                for kind in MERGE_KINDS:
                    _MERGE.append(make_merge_case(O, kind, s, K, R))
                    s += 1
    return _MERGE


def pack_blocks(blocks):
    """the all-gather layout: per rank {Rec [nb][K]; int64 fc [nb]}"""
    return np.concatenate([np.concatenate([recs.view(np.uint8), _c64(fc).view(np.uint8)]) for recs, fc in blocks])


def pack_export(x, room=None):
    """an export as the device reads it: the 16-byte header {count, 0...} and the records"""
    buf = np.zeros(XHDR_BYTES + (len(x) if room is None else room) * XREC_DTYPE.itemsize, np.uint8)
    buf[:4] = np.array([len(x)], np.int32).view(np.uint8)
    buf[XHDR_BYTES:XHDR_BYTES + x.nbytes] = np.ascontiguousarray(x).view(np.uint8)
    return buf


def unpack_export(buf):
    n = int(buf[:4].view(np.int32)[0])
    x = buf[XHDR_BYTES:XHDR_BYTES + n * XREC_DTYPE.itemsize].view(XREC_DTYPE).copy()
    return x[np.argsort(x["idx"], kind="stable")]
