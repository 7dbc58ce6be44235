"""Shared by the ksched_rank tests: the oracle's ranked lists (oracle.local_topk over a node range, oracle.merge_topk
over shards) as the five columns of the C ABI -- idx, score (as int64 bit patterns), reason, count, feasible."""
import dataclasses

import numpy as np

CLUSTERS = {"c3": ("c3", 20011, 64), "c2": ("c2", 5000, 64), "c5hc": ("c5hc", 2000, 64), "c5": ("c5", 5000, 64)}


def make(name):
    from ksched import cluster
    if name in CLUSTERS:
        cfg, n, p = CLUSTERS[name]
        return cluster.make_cluster(cfg, n_nodes=n, n_pods=p)
    assert name == "small93"
    return cluster.random_small(93, n_nodes=211, n_pods=96)


def shard_recs(O, cl, k, lo, hi, pods=slice(None)):
    """oracle.local_topk of the cluster's pods over nodes [lo, hi): (recs[m * k], fc[m])."""
    lab = None if cl.labels is None else np.ascontiguousarray(cl.labels[lo:hi])
    pr = None if cl.price is None else np.ascontiguousarray(cl.price[lo:hi])
    sel = None if cl.selector is None else np.ascontiguousarray(cl.selector[pods])
    c = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    return O.local_topk((cl.priority, cl.domain, cl.use_labels), k, lo, c(cl.alloc_cpu[lo:hi]), c(cl.alloc_mem[lo:hi]),
                        c(cl.alloc_pods[lo:hi]), lab, pr, c(cl.req_cpu[pods]), c(cl.req_mem[pods]),
                        c(cl.req_pods[pods]), sel)


def reasons_of(O, cl, idx, pods=slice(None), lo=0, hi=None):
    """oracle.node_reasons(...)[1][idx] per pod, 0 where idx is -1.  idx is global; the state is nodes [lo, hi)."""
    hi = cl.n_nodes if hi is None else hi
    state = (cl.alloc_cpu[lo:hi], cl.alloc_mem[lo:hi], cl.alloc_pods[lo:hi])
    sub = dataclasses.replace(cl, labels=None if cl.labels is None else cl.labels[lo:hi])
    rc, rm, rp = cl.req_cpu[pods], cl.req_mem[pods], cl.req_pods[pods]
    sel = None if cl.selector is None else cl.selector[pods]
    out = np.zeros(idx.shape, np.uint8)
    for i in range(idx.shape[0]):
        per_node = O.node_reasons(sub, state, rc[i], rm[i], rp[i], 0 if sel is None else sel[i])[1]
        ok = idx[i] >= 0
        out[i, ok] = per_node[idx[i, ok] - lo]
    return out


def columns(O, cl, recs, fc, k, pods=slice(None), lo=0, hi=None):
    """(idx[m, k], score bits int64[m, k], reason[m, k], count[m], feasible[m]) of oracle recs."""
    r = recs.reshape(-1, k)
    valid = r["valid"] != 0
    idx = np.where(valid, r["idx"], -1).astype(np.int32)
    key = r["key"] if cl.priority == 0 else 0.0 - r["key"]  # the schedule's convention: the score, or the price
    score = np.where(valid, key, 0.0)
    return (idx, np.ascontiguousarray(score).view(np.int64), reasons_of(O, cl, idx, pods, lo, hi),
            valid.sum(1).astype(np.int32), fc.astype(np.int32))


def want(O, cl, k, pods=slice(None)):
    recs, fc = shard_recs(O, cl, k, 0, cl.n_nodes, pods)
    return columns(O, cl, recs, fc, k, pods)


def same(got, ref):
    """got: an Engine.rank / merge_ranked result; ref: columns().  Every column, scores by bit pattern."""
    names = ("idx", "score", "reason", "count", "feasible")
    g = (got[0], np.ascontiguousarray(got[1]).view(np.int64), got[2], got[3], got[4])
    for nm, a, b in zip(names, g, ref):
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{nm}: first difference at {bad[0].tolist()}: got {a[tuple(bad[0])]}, want {b[tuple(bad[0])]}"
