#!/usr/bin/env python3
"""Wall time of ksched_rank_full on c4's 100k nodes (the call with its copies and its sync: a host clock around it), the
median over --calls calls after --warmup, for m = 1 / k = 64 and m = 4096 / k = 16:
  (a) every constraint off, beside ksched_rank of the same pods: what the smaller tile and the histogram cost
  (b) all three on -- R = 4 extended columns, a 64 x 64 spread table, 64 affinity groups over 1024 zones -- and each of
      the three alone: what the row's extra loads, the LDS tables and the longer predicate cost, and which of them
and ksched_explain_full of one pod under (b) beside ksched_explain.  The tables are seeded random ones; the calls are dry
runs, so every call sees the same state.  One JSON line per case.   python tools/rank_full_time.py [--calls 40] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "k8s-scheduler_amd")]
from ksched import MODE_EXACT, Engine, cluster  # noqa: E402

R, S, D, GROUPS, ZONES = 4, 64, 64, 64, 1024


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(p50=statistics.median(ts), min=min(ts), max=max(ts))


def tables(n, m, seed=11):
    """(load_spread's, load_ext's, load_affinity's arguments), then the pods' constraint arrays by constraint."""
    g = np.random.default_rng(seed)
    bits = lambda size, per: np.bitwise_or.reduce(np.uint64(1) << g.integers(0, GROUPS, (per,) + size).astype(np.uint64)) \
        * (g.random(size) < 0.3).astype(np.uint64)
    spread = (np.where(g.random(n) < 0.02, -1, g.permutation(n) % D).astype(np.int32), g.integers(1, 6, S).astype(np.int32),
              g.integers(0, 20, (S, D)).astype(np.int32))
    ext = (g.integers(0, 9, (R, n)).astype(np.int64),)
    aff = (np.where(g.random(n) < 0.02, -1, g.permutation(n) % ZONES).astype(np.int32), bits((n,), 2), bits((n,), 1),
           bits((n,), 1))
    pods = dict(spread=dict(group=g.integers(-1, S, m).astype(np.int32), enforce=(g.random(m) < 0.8).astype(np.uint8)),
                ext=dict(req_ext=g.integers(0, 3, (R, m)).astype(np.int64)),
                affinity=dict(member=bits((m,), 1), anti_host=bits((m,), 1), anti_zone=bits((m,), 1),
                              aff_group=g.integers(-1, GROUPS, m).astype(np.int32), aff_zone=(g.random(m) < 0.5).astype(np.uint8)))
    return spread, ext, aff, pods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pods", type=int, default=4096)
    a = ap.parse_args()
    assert a.calls >= 20, "the median is taken over at least 20 calls"
    cl = cluster.make_cluster("c4", n_nodes=a.nodes, n_pods=a.pods)
    rc, rm, rp = cl.req_cpu, cl.req_mem, cl.req_pods
    spread, ext, aff, pods = tables(cl.n_nodes, cl.n_pods)
    variants = {"off": {}, "spread": pods["spread"], "ext": pods["ext"], "affinity": pods["affinity"],
                "all": {**pods["spread"], **pods["ext"], **pods["affinity"]}}
    i = int((rc > 0).argmax())  # the first pod with a request: a zero-request pod is all ties
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain, device=0) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        e.load_spread(*spread)
        e.load_ext(*ext)
        e.load_affinity(*aff, n_domains=ZONES)
        for case, sl, k in (("m=1,k=64", slice(i, i + 1), 64), (f"m={cl.n_pods},k=16", slice(None), 16)):
            cut = lambda kw: {nm: (v[:, sl] if v.ndim == 2 else v[sl]) for nm, v in kw.items()}
            out = dict(case=case, nodes=cl.n_nodes, calls=a.calls,
                       rank_ms=median_ms(lambda: e.rank(rc[sl], rm[sl], rp[sl], k=k), a.calls, a.warmup))
            for name, kw in variants.items():
                kw = cut(kw)
                out[f"rank_full_{name}_ms"] = median_ms(lambda: e.rank_full(rc[sl], rm[sl], rp[sl], None, k, **kw), a.calls, a.warmup)
                fe = e.rank_full(rc[sl], rm[sl], rp[sl], None, k, **kw)[4]
                out[f"eligible_mean_{name}"] = float(fe.mean())
            out["off_over_rank"] = out["rank_full_off_ms"]["p50"] / out["rank_ms"]["p50"]
            out["all_over_off"] = out["rank_full_all_ms"]["p50"] / out["rank_full_off_ms"]["p50"]
            print(json.dumps(out), flush=True)
        one = {nm: (v[:, i] if v.ndim == 2 else v[i]) for nm, v in variants["all"].items()}
        x = dict(case="explain, one pod", nodes=cl.n_nodes, calls=a.calls)
        for per_node in (False, True):
            tag = "per_node" if per_node else "counts"
            x[f"explain_{tag}_ms"] = median_ms(lambda: e.explain(int(rc[i]), int(rm[i]), int(rp[i]), per_node=per_node),
                                               a.calls, a.warmup)
            x[f"explain_full_{tag}_ms"] = median_ms(
                lambda: e.explain_full(int(rc[i]), int(rm[i]), int(rp[i]), 0, int(one["group"]), bool(one["enforce"]),
                                       one["req_ext"], int(one["member"]), int(one["anti_host"]), int(one["anti_zone"]),
                                       int(one["aff_group"]), bool(one["aff_zone"]), per_node=per_node), a.calls, a.warmup)
        print(json.dumps(x), flush=True)


if __name__ == "__main__":
    main()
