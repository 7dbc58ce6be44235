#!/usr/bin/env python3
"""Wall time of ksched_preempt_constrained beside ksched_preempt on the table of tools/preempt_time.py (c4's 100k nodes
with the bound pods its used pod slots stand for), in the same process and the same run: the call with its copies and
its sync, a host clock around it, the median over --calls calls after --warmup.  Per m three numbers:
    preempt       ksched_preempt
    off           ksched_preempt_constrained with both constraints off (its own kernels on the same columns)
    ext2_spread   ksched_preempt_constrained with two extended columns and spread on (8 zones, 3 groups)
The two extra columns: amounts 0 .. 2 on about 40 % of the bound pods, node amounts 0 .. 2, requests 1 .. 4 on about half
the pods; each bound pod in each group at 0.35, the counts the table's own, skews 1 .. 3, every pod enforcing a group.
Each m runs in a child process of its own under --timeout seconds, and the first child that fails or runs out of time
ends the run.  Per case one JSON line.
    python tools/preempt_constrained_time.py [--calls 20] [--warmup 3] [--m 1 64 1024]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "k8s-scheduler_amd"), os.path.dirname(os.path.abspath(__file__))]

R, D, S = 2, 8, 3


def timed(fn, warmup, calls):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(p50=statistics.median(ts), min=min(ts), max=max(ts)), out


def run_case(a, m):
    import numpy as np
    from ksched import MODE_EXACT, Engine, cluster
    from preempt_time import table
    cl = cluster.make_cluster("c4", n_nodes=a.nodes, n_pods=max(m, 1))
    n = cl.n_nodes
    seg, bound = table(cl)
    nb = len(bound[0])
    r = np.random.default_rng(3)
    prio = (np.random.default_rng(2).integers(3, 8, m) * 100).astype(np.int32)
    node_ext = r.integers(0, 3, (R, n)).astype(np.int64)
    bound_ext = (r.integers(0, 3, (R, nb)) * (r.random((R, nb)) < 0.4)).astype(np.int64)
    req_ext = (r.integers(1, 5, (R, m)) * (r.random((R, m)) < 0.5)).astype(np.int64)
    dom = (np.arange(n) % D).astype(np.int32)
    mask = np.zeros(nb, np.uint64)
    counts = np.zeros((S, D), np.int32)
    for s in range(S):
        on = r.random(nb) < 0.35
        mask |= on.astype(np.uint64) << np.uint64(s)
        counts[s] = np.bincount(dom[bound[0][on]], minlength=D)
    skew = r.integers(1, 4, S).astype(np.int32)
    group = r.integers(0, S, m).astype(np.int32)
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        e.load_spread(dom, skew, counts)
        e.load_ext(node_ext)
        t0 = time.perf_counter()
        e.load_bound_constrained(*bound, bound_ext, mask)
        load_ms = (time.perf_counter() - t0) * 1e3
        rc, rm, rp = cl.req_cpu[:m] * 16, cl.req_mem[:m] * 16, cl.req_pods[:m]
        t_plain, plain = timed(lambda: e.preempt(rc, rm, rp, None, prio, vcap=16), a.warmup, a.calls)
        t_off, off = timed(lambda: e.preempt_constrained(rc, rm, rp, None, prio, vcap=16), a.warmup, a.calls)
        t_on, on = timed(lambda: e.preempt_constrained(rc, rm, rp, None, prio, group, None, req_ext, vcap=16), a.warmup, a.calls)
    assert all(np.array_equal(x, y) for x, y in zip(plain, off)), "constraints off must equal ksched_preempt"
    print(json.dumps(dict(case=f"m={m}", nodes=n, bound_pods=int(seg.sum()), calls=a.calls, preempt_ms=t_plain, off_ms=t_off,
                          ext2_spread_ms=t_on, load_bound_constrained_ms=load_ms,
                          no_fit=[int((o[0] < 0).sum()) for o in (plain, on)],
                          with_victims=[int((o[1] > 0).sum()) for o in (plain, on)])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--m", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--timeout", type=int, default=240, help="seconds a case may take")
    ap.add_argument("--case", type=int, default=None, help="(child) run this m in this process")
    a = ap.parse_args()
    if a.case is not None:
        run_case(a, a.case)
        return 0
    for m in a.m:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(m), "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--nodes", str(a.nodes)]
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"m={m}: no result within {a.timeout} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"m={m}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
