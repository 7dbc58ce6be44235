#!/usr/bin/env python3
"""Wall time of ksched_rank on c4's 100k nodes (the call with its copies and its sync: a host clock around it), the
median over --calls calls after --warmup, against the two existing calls that do comparable work:
  m = 1, k = 64     one pod shape      vs ksched_explain of the same pod (one pass over every row, then a sync)
  m = 4096, k = 16  bulk what-if       vs the stream pipeline's top-16 lists of the same pods: score + merge kernel
                                       time per pod (kernel_ms[0] + kernel_ms[1], topk=16, batch=64, every batch timed)
One JSON line per case.   python tools/rank_time.py [--calls 40] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "k8s-scheduler_amd")]
from ksched import MODE_BATCHED, Engine, cluster  # noqa: E402
from ksched._lib import PIPELINE_STREAM  # noqa: E402


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


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
    with Engine(mode=MODE_BATCHED, priority=cl.priority, domain=cl.domain, pipeline=PIPELINE_STREAM, topk=16, batch=64,
                timing=True, timing_every=1) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        e.save_state()
        # m = 1 (the first pod with a request: a zero-request pod is all ties)
        i = int((rc > 0).argmax())
        one = slice(i, i + 1)
        r1 = median_ms(lambda: e.rank(rc[one], rm[one], rp[one], k=64), a.calls, a.warmup)
        x1 = median_ms(lambda: e.explain(int(rc[i]), int(rm[i]), int(rp[i]), per_node=False), a.calls, a.warmup)
        x1n = median_ms(lambda: e.explain(int(rc[i]), int(rm[i]), int(rp[i]), per_node=True), a.calls, a.warmup)
        print(json.dumps(dict(case="m=1,k=64", nodes=cl.n_nodes, calls=a.calls, rank_ms=dict(zip(("p50", "min", "max"), r1)),
                              explain_counts_ms=dict(zip(("p50", "min", "max"), x1)),
                              explain_per_node_ms=dict(zip(("p50", "min", "max"), x1n)),
                              rank_over_explain=r1[0] / x1[0])), flush=True)
        # bulk
        rb = median_ms(lambda: e.rank(rc, rm, rp, k=16), a.calls, a.warmup)
        per = []
        for _ in range(3):  # the stream pipeline's own top-16 lists of the same pods (it also commits: state restored)
            e.restore_state()
            e.schedule(rc, rm, rp)
            st = e.stats()
            per.append((st["kernel_ms"][0] / max(st["kernel_launches"][0], 1) +
                        st["kernel_ms"][1] / max(st["kernel_launches"][1], 1)) / 64 * 1e3)
        print(json.dumps(dict(case=f"m={cl.n_pods},k=16", nodes=cl.n_nodes, calls=a.calls,
                              rank_ms=dict(zip(("p50", "min", "max"), rb)), rank_us_per_pod=rb[0] / cl.n_pods * 1e3,
                              stream_score_merge_us_per_pod=statistics.median(per), stream_pipeline=st["pipeline"],
                              stream_timed_batches=st["kernel_launches"][:2])), flush=True)


if __name__ == "__main__":
    main()
