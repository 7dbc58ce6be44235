#!/usr/bin/env python3
"""Device time per pod of ksched_schedule_affinity against ksched_schedule in exact mode, the same pods on the c3 cluster
(50k nodes, resource priority, feasible domain -- the domain in which the constraint is enforced): the median over
--calls calls after --warmup, the node state restored and the affinity table reloaded before each.  Both the call's wall
time (a host clock around it: copies, launch, sync) and its device time (the HIP events of ksched_stats.device_ms)
are reported, with the spread (min, max) of each:
  (a) schedule         ksched_schedule, exact mode -- the yardstick; also what a library without the affinity call gives
                       (KSCHED_LIB=<an older build>, tools/build_base.sh: the same pods through the parent's kernel)
  (b) empty pods       ksched_schedule_affinity with no group and no term on any pod: the same placements through
                       k_exact<kRunAffinity>, no LDS read, no commit
  (c) hostname anti    one group, every pod a member with a host-scope anti-affinity term against it: one replica per
                       node, every placement ORs into its node's words and (D 3) into a zone word that already has the bit
  (d) zone, D 1024     four groups over 1024 zones: every pod refuses its own group in its zone, and the pods of groups
                       1-3 need the group before theirs in the zone: every placement moves the zone table
The affinity rows carry their ratio to (a)'s device p50, the placements and the bits set at the end.
One JSON line per case.   python tools/affinity_time.py [--calls 21] [--warmup 3] [--pods 4096] [--only a]"""
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
    g = np.arange(p) % 4
    bit = (np.uint64(1) << g.astype(np.uint64))
    one = np.ones(p, np.uint64)
    tables = {  # row: (name, node_domain, (member, anti_host, anti_zone, aff_group, aff_zone))
        "b": ("empty pods", np.arange(n) % 3, (None, None, None, None, None)),
        "c": ("hostname anti", np.arange(n) % 3, (one, one, None, None, None)),
        "d": ("zone, D 1024", rng.permutation(n) % 1024, (bit, None, bit, (g - 1).astype(np.int32), np.ones(p, np.uint8))),
    }
    have = hasattr(L.lib(), "ksched_schedule_affinity")
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
                name, dom, words = tables[row]
                wall, dev, out = timed(e, lambda: e.schedule_affinity(rc, rm, rp, None, *words), a.calls, a.warmup,
                                       before=lambda: e.load_affinity(dom))
            us = lambda ms: ms / p * 1e3
            r = dict(row=row, case=name, lib=os.path.basename(L.LIB_PATH), nodes=n, pods=p, calls=a.calls,
                     placed=int((out[0] >= 0).sum()),
                     wall_us_per_pod=dict(p50=us(statistics.median(wall)), min=us(min(wall)), max=us(max(wall))),
                     device_us_per_pod=dict(p50=us(statistics.median(dev)), min=us(min(dev)), max=us(max(dev))))
            if row == "a":
                base = statistics.median(dev)
            else:
                tab = e.read_affinity()
                r.update(nodes_with_member=int((tab[0] != 0).sum()), nodes_with_anti=int(((tab[1] | tab[2]) != 0).sum()))
                if base:
                    r["device_ratio_to_a"] = statistics.median(dev) / base
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
