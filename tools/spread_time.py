#!/usr/bin/env python3
"""Device time per pod of ksched_schedule_spread against ksched_schedule in exact mode, the same pods on the c3 cluster
(50k nodes, resource priority, feasible domain -- the domain in which the constraint is enforced): the median over
--calls calls after --warmup, the node state restored and the spread table reloaded before each.  Both the call's wall
time (a host clock around it: copies, launch, sync) and its device time (the HIP events of ksched_stats.device_ms)
are reported, with the spread (min, max) of each:
  (a) schedule         ksched_schedule, exact mode -- the yardstick; also what a library without the spread call gives
                       (KSCHED_LIB=<an older build>, tools/build_base.sh: the same pods through the parent's kernel)
  (b) no groups        ksched_schedule_spread with every group -1: the same placements through k_exact<SPREAD>
  (c) 3 zones          one group, max_skew 1, every pod enforcing
  (d) D 1024, S 4      the table at its caps: pods spread over four groups, every pod enforcing
The spread rows carry their ratio to (a)'s device p50, the placements and the counts' range at the end.
One JSON line per case.   python tools/spread_time.py [--calls 21] [--warmup 3] [--pods 4096] [--only a]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "k8s-scheduler_amd")]
from ksched import MODE_EXACT, Engine, cluster  # noqa: E402
from ksched import _lib as L  # noqa: E402


def timed(e, fn, calls, warmup, before=None):
    wall, dev, out = [], [], None
    for k in range(warmup + calls):
        e.restore_state()
        e.sync()
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            wall.append(dt)
            dev.append(e.stats()["device_ms"])
    return wall, dev, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=4096)
    ap.add_argument("--only", default="abcd", help="the rows to run, e.g. a")
    a = ap.parse_args()
    cl = dataclasses.replace(cluster.make_cluster("c3", n_nodes=a.nodes, n_pods=a.pods), domain=cluster.DOMAIN_FEASIBLE)
    rc, rm, rp = cl.req_cpu, cl.req_mem, cl.req_pods
    n, p = cl.n_nodes, cl.n_pods
    rng = np.random.default_rng(1)
    tables = {  # row: (node_domain, max_skew, group)
        "b": ("no groups", np.arange(n) % 3, np.ones(1, np.int32), np.full(p, -1, np.int32)),
        "c": ("3 zones", np.arange(n) % 3, np.ones(1, np.int32), np.zeros(p, np.int32)),
        "d": ("D 1024, S 4", rng.permutation(n) % 1024, np.ones(4, np.int32), (np.arange(p) % 4).astype(np.int32)),
    }
    have = hasattr(L.lib(), "ksched_schedule_spread")
    base = None
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        e.save_state()
        for row in "abcd":
            if row not in a.only or (row != "a" and not have):
                continue
            if row == "a":
                name = "schedule"
                wall, dev, out = timed(e, lambda: e.schedule(rc, rm, rp), a.calls, a.warmup)
            else:
                name, dom, skew, group = tables[row]
                wall, dev, out = timed(e, lambda: e.schedule_spread(rc, rm, rp, None, group), a.calls, a.warmup,
                                       before=lambda: e.load_spread(dom, skew))
            us = lambda ms: ms / p * 1e3
            r = dict(row=row, case=name, lib=os.path.basename(L.LIB_PATH), nodes=n, pods=p, calls=a.calls,
                     placed=int((out[0] >= 0).sum()),
                     wall_us_per_pod=dict(p50=us(statistics.median(wall)), min=us(min(wall)), max=us(max(wall))),
                     device_us_per_pod=dict(p50=us(statistics.median(dev)), min=us(min(dev)), max=us(max(dev))))
            if row == "a":
                base = statistics.median(dev)
            else:
                cnt = e.read_spread()
                r.update(counts_min=int(cnt.min()), counts_max=int(cnt.max()), counts_sum=int(cnt.sum()))
                if base:
                    r["device_ratio_to_a"] = statistics.median(dev) / base
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
