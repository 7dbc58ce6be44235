#!/usr/bin/env python3
"""Device time per pod of ksched_schedule_full against the calls it composes, the same pods on the c3 cluster (50k nodes,
resource priority, feasible domain -- the domain in which the constraints are enforced), the same kernel geometry for
every row: the median over --calls calls after --warmup, the node state restored and all three tables reloaded before
each.  Both the call's wall time (a host clock around it: copies, launch, sync) and its device time (the HIP events of
ksched_stats.device_ms) are reported, with the spread (min, max) of each.  The input is tools/constrained_time.py's --
gangs of 1, 2, 3, 5, 8, 13 pods in turn, every member required; three zones, one spread group with max_skew 1 that every
pod is in and enforces; four extended columns of 8 per node, every pod asking for 1 of column 0 -- with
tools/affinity_time.py's hostname row for the affinity words: one group, every pod a member with a host-scope
anti-affinity term against it (one replica per node; the affinity table on the same three zones).
  (a) schedule         ksched_schedule, exact mode -- the yardstick, measured in this very process
  (c) constrained      ksched_schedule_constrained, all three on     (C) ksched_schedule_full, the same with affinity off
  (f) affinity         ksched_schedule_affinity                      (F) ksched_schedule_full with only affinity on
  (A) all four         ksched_schedule_full with gangs, spread, extended resources and affinity on
  (R) all rejected     (A) with the last member of every gang asking for 9 of column 1, which no node has: every gang of
                       two or more is rolled back after its other members were placed and logged
The rows are run in order --reps times (a c C f F A R a c ...), so that drift between repetitions shows next to the
differences between rows.  Every row carries its ratio to (a)'s device p50 of the same repetition; C and F carry the
ratio to the call they stand in for, A the ratio to the slower of c and f, and R the device time it adds to A per
rolled-back member.  A last line gives, per row, the range of the p50s and of the ratios over the repetitions.
One JSON line per row and repetition.   python tools/full_time.py [--calls 21] [--warmup 3] [--pods 4096] [--reps 2]"""
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

ROWS = "acCfFAR"
OWN = {"C": "c", "F": "f"}


def timed(e, fn, calls, warmup, before):
    wall, dev, out = [], [], None
    for k in range(warmup + calls):
        e.restore_state()
        e.sync()
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
    ap.add_argument("--only", default=ROWS, help="the rows to run, e.g. acC")
    a = ap.parse_args()
    cl = dataclasses.replace(cluster.make_cluster("c3", n_nodes=a.nodes, n_pods=a.pods), domain=cluster.DOMAIN_FEASIBLE)
    rc, rm, rp = cl.req_cpu, cl.req_mem, cl.req_pods
    n, p = cl.n_nodes, cl.n_pods
    off = [0]
    while off[-1] < p:
        off.append(min(p, off[-1] + (1, 2, 3, 5, 8, 13)[(len(off) - 1) % 6]))
    off = np.asarray(off, np.int64)
    dom, skew = (np.arange(n) % 3).astype(np.int32), np.ones(1, np.int32)
    group = np.zeros(p, np.int32)
    node_ext = np.full((L.EXT_MAX, n), 8, np.int64)
    req = np.zeros((L.EXT_MAX, p), np.int64)
    req[0] = 1
    doomed = req.copy()
    doomed[1, off[1:] - 1] = 9  # the last member of every gang fits nowhere
    one = np.ones(p, np.uint64)
    words = dict(member=one, anti_host=one)
    p50s, ratios = {}, {}
    us = lambda ms: ms / p * 1e3
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        e.save_state()

        def reload():
            e.load_spread(dom, skew)
            e.load_ext(node_ext)
            e.load_affinity(dom)

        three = dict(gang_off=off, group=group, req_ext=req)
        full = lambda **kw: e.schedule_full(rc, rm, rp, None, **kw)
        calls = {"a": ("schedule", lambda: e.schedule(rc, rm, rp)),
                 "c": ("constrained, all three", lambda: e.schedule_constrained(rc, rm, rp, None, **three)),
                 "C": ("full, affinity off", lambda: full(**three)),
                 "f": ("affinity", lambda: e.schedule_affinity(rc, rm, rp, None, **words)),
                 "F": ("full, only affinity", lambda: full(**words)),
                 "A": ("full, all four", lambda: full(**three, **words)),
                 "R": ("full, every gang rejected", lambda: full(gang_off=off, group=group, req_ext=doomed, **words))}
        for rep in range(a.reps):
            med = {}
            for row in ROWS:
                if row not in a.only:
                    continue
                name, fn = calls[row]
                wall, dev, out = timed(e, fn, a.calls, a.warmup, reload)
                med[row] = statistics.median(dev)
                rolled = int((out[0] == L.GANG_REJECTED).sum())
                r = dict(rep=rep, row=row, case=name, nodes=n, pods=p, calls=a.calls, placed=int((out[0] >= 0).sum()),
                         rejected=rolled,
                         wall_us_per_pod=dict(p50=us(statistics.median(wall)), min=us(min(wall)), max=us(max(wall))),
                         device_us_per_pod=dict(p50=us(med[row]), min=us(min(dev)), max=us(max(dev))))
                p50s.setdefault(row, []).append(us(med[row]))
                if row != "a" and "a" in med:
                    r["device_ratio_to_a"] = med[row] / med["a"]
                    ratios.setdefault(row + "/a", []).append(r["device_ratio_to_a"])
                if OWN.get(row) in med:
                    r["device_ratio_to_own_call"] = med[row] / med[OWN[row]]
                    ratios.setdefault(row + "/" + OWN[row], []).append(r["device_ratio_to_own_call"])
                if row == "A" and all(k in med for k in "cf"):
                    r["device_ratio_to_slowest_part"] = med[row] / max(med[k] for k in "cf")
                    ratios.setdefault("A/max(c,f)", []).append(r["device_ratio_to_slowest_part"])
                if row == "R" and "A" in med and rolled:
                    r["device_us_added_per_rolled_member"] = (med[row] - med["A"]) * 1e3 / rolled
                    ratios.setdefault("(R-A)/rolled, us", []).append(r["device_us_added_per_rolled_member"])
                print(json.dumps(r), flush=True)
    print(json.dumps(dict(summary=True, device_p50_us_per_pod={k: [min(v), max(v)] for k, v in p50s.items()},
                          device_ratios={k: [min(v), max(v)] for k, v in ratios.items()})), flush=True)


if __name__ == "__main__":
    main()
