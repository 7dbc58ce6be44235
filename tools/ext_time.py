#!/usr/bin/env python3
"""Device time per pod of ksched_schedule_ext against ksched_schedule in exact mode, the same pods on the c3 cluster
(50k nodes, resource priority, feasible domain -- the domain in which the constraint is enforced), the same kernel
geometry for every row: the median over --calls calls after --warmup, the node state restored and the table reloaded
before each.  Both the call's wall time (a host clock around it: copies, launch, sync) and its device time (the HIP
events of ksched_stats.device_ms) are reported, with the spread (min, max) of each:
  (a) schedule         ksched_schedule, exact mode -- the yardstick, measured in this very process
  (b) all zero         ksched_schedule_ext, four columns loaded, every request zero: the same placements through
                       k_exact<EXT>, no LDS read per pod
  (c) one column       every pod asks for 1 of column 0 (8 per node)
  (d) four columns     every pod asks for 1 of every column
The rows are run in order --reps times (a b c d a b c d), so that drift between repetitions shows next to the
differences between rows; every ext row carries its ratio to (a)'s device p50 of the same repetition, and a last line
gives, per row, the range of the p50s and of the ratios over the repetitions.
One JSON line per row and repetition.   python tools/ext_time.py [--calls 21] [--warmup 3] [--pods 4096] [--reps 2]"""
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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", default="abcd", help="the rows to run, e.g. ab")
    a = ap.parse_args()
    cl = dataclasses.replace(cluster.make_cluster("c3", n_nodes=a.nodes, n_pods=a.pods), domain=cluster.DOMAIN_FEASIBLE)
    rc, rm, rp = cl.req_cpu, cl.req_mem, cl.req_pods
    n, p = cl.n_nodes, cl.n_pods
    node_ext = np.full((L.EXT_MAX, n), 8, np.int64)
    one = np.zeros((L.EXT_MAX, p), np.int64)
    one[0] = 1
    rows = {"b": ("all zero", np.zeros((L.EXT_MAX, p), np.int64)), "c": ("one column", one),
            "d": ("four columns", np.ones((L.EXT_MAX, p), np.int64))}
    p50s, ratios = {}, {}
    us = lambda ms: ms / p * 1e3
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        e.save_state()
        for rep in range(a.reps):
            base = None
            for row in "abcd":
                if row not in a.only:
                    continue
                if row == "a":
                    name = "schedule"
                    wall, dev, out = timed(e, lambda: e.schedule(rc, rm, rp), a.calls, a.warmup)
                else:
                    name, req = rows[row]
                    wall, dev, out = timed(e, lambda: e.schedule_ext(rc, rm, rp, None, req), a.calls, a.warmup,
                                           before=lambda: e.load_ext(node_ext))
                r = dict(rep=rep, row=row, case=name, nodes=n, pods=p, calls=a.calls, placed=int((out[0] >= 0).sum()),
                         wall_us_per_pod=dict(p50=us(statistics.median(wall)), min=us(min(wall)), max=us(max(wall))),
                         device_us_per_pod=dict(p50=us(statistics.median(dev)), min=us(min(dev)), max=us(max(dev))))
                p50s.setdefault(row, []).append(us(statistics.median(dev)))
                if row == "a":
                    base = statistics.median(dev)
                else:
                    tab = e.read_ext()
                    r.update(ext_taken=int((node_ext - tab).sum()), ext_min=int(tab.min()))
                    if base:
                        r["device_ratio_to_a"] = statistics.median(dev) / base
                        ratios.setdefault(row, []).append(r["device_ratio_to_a"])
                print(json.dumps(r), flush=True)
    print(json.dumps(dict(summary=True, device_p50_us_per_pod={k: [min(v), max(v)] for k, v in p50s.items()},
                          device_ratio_to_a={k: [min(v), max(v)] for k, v in ratios.items()})), flush=True)


if __name__ == "__main__":
    main()
