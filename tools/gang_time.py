#!/usr/bin/env python3
"""Time per pod of ksched_schedule_gangs against ksched_schedule in exact mode, the same pods on the c3 cluster (50k
nodes, resource priority): the median over --calls calls after --warmup, the node state restored before each.
Both the call's wall time (a host clock around it: copies, launch, sync) and its device time (the HIP events of
ksched_stats.device_ms) are reported, with the spread (min, max) of each, on two sets of nodes:
  c3             the cluster as it is.  Its nodes are roomy and every gang is accepted (the rows print rejected = 0):
                 the gang cases measure the bookkeeping of accepted gangs only, no rollback runs
  c3 tight       every node's cpu and memory divided by --tight (16), feasible domain: about half of the 8-member
                 gangs are rejected and rolled back (rejected, rolled_back_pods in the row) -- the rollback's number
and per set:
  schedule       ksched_schedule, exact mode -- the yardstick; also what a library without the gang call gives
                 (KSCHED_LIB=<an older build>, tools/build_base.sh: the same pods through the parent's kernel)
  gangs of 1     ksched_schedule_gangs, every pod its own gang: the same placements, plus the gang bookkeeping
  gangs of 8     all members required
One JSON line per case.   python tools/gang_time.py [--calls 21] [--warmup 3] [--pods 4096] [--tight 16]"""
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


def timed(e, fn, calls, warmup):
    wall, dev, out = [], [], None
    for k in range(warmup + calls):
        e.restore_state()
        e.sync()
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
    ap.add_argument("--tight", type=int, default=16)
    a = ap.parse_args()
    c3 = cluster.make_cluster("c3", n_nodes=a.nodes, n_pods=a.pods)
    tight = dataclasses.replace(c3, name="c3 tight", alloc_cpu=c3.alloc_cpu // a.tight, alloc_mem=c3.alloc_mem // a.tight,
                                domain=cluster.DOMAIN_FEASIBLE)
    for cl in (c3, tight):
        rc, rm, rp = cl.req_cpu, cl.req_mem, cl.req_pods
        p = cl.n_pods
        cases = [("schedule", lambda e: e.schedule(rc, rm, rp))]
        if hasattr(L.lib(), "ksched_schedule_gangs"):
            for size in (1, 8):
                off = np.minimum(np.arange(0, p + size, size), p).astype(np.int64)
                cases.append((f"gangs of {size}", lambda e, off=off: e.schedule_gangs(rc, rm, rp, None, off)))
        with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain) as e:
            e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
            e.save_state()
            for name, fn in cases:
                wall, dev, out = timed(e, lambda: fn(e), a.calls, a.warmup)
                us = lambda ms: ms / p * 1e3
                row = dict(nodes_set=cl.name, case=name, lib=os.path.basename(L.LIB_PATH), nodes=cl.n_nodes, pods=p,
                           calls=a.calls, placed=int((out[0] >= 0).sum()),
                           wall_us_per_pod=dict(p50=us(statistics.median(wall)), min=us(min(wall)), max=us(max(wall))),
                           device_us_per_pod=dict(p50=us(statistics.median(dev)), min=us(min(dev)), max=us(max(dev))))
                if len(out) == 4:
                    row.update(gangs=int(out[3].shape[0]), rejected=int((out[3] == 0).sum()),
                               rolled_back_pods=int((out[0] == L.GANG_REJECTED).sum()))
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
