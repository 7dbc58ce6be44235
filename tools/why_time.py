#!/usr/bin/env python3
"""Device time per pod of ksched_schedule_full_why against ksched_schedule_full on tools/full_time.py's input (the c3
cluster at 50k nodes, resource priority, feasible domain; gangs of 1, 2, 3, 5, 8, 13 pods in turn, every member required;
three zones, one spread group with max_skew 1 that every pod is in and enforces; four extended columns of 8 per node,
every pod asking for 1 of column 0; one affinity group, every pod a member with a host-scope anti-affinity term against
it), the same kernel geometry for every row: the median over --calls calls after --warmup, the node state restored and
all three tables reloaded before each.  Both the call's wall time and its device time (the HIP events of
ksched_stats.device_ms: the kernel alone -- the clears of the rows' buffer before it and the copies after it are in the
wall time only) are reported, with the spread (min, max) of each.
  (A)  ksched_schedule_full, all four on, every pod placed -- unchanged by the new call, so the yardstick of "a pod that
       finds a node pays nothing", measured in this very process
  (W0) ksched_schedule_full_why on the same input: no NO_FIT pod, why_rows = p
  (R)  full_time's rejected row: the last member of every gang asks for 9 of column 1, which no node has
  (W1) ksched_schedule_full_why on (R)'s input, why_rows = p, node_rows = 0
  (W2) the same with node_rows = 64
The rows are run in order --reps times (A W0 R W1 W2 A W0 ...), so that drift between repetitions shows next to the
differences between rows: the spread of (A)'s two p50s is the margin of every comparison here.  W0 carries its ratio to
A, W1 the device time it adds to R per NO_FIT pod, W2 what it adds to W1 per recorded node row.  A last line gives, per
row, the range of the p50s and of the derived figures over the repetitions.
One JSON line per row and repetition.
  python tools/why_time.py [--calls 21] [--warmup 3] [--nodes 50000] [--pods 4096] [--reps 2]
  python tools/why_time.py --nodes 400000 --pods 2048     (eight node slots per thread: the widest instantiation)"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "k8s-scheduler_amd"), os.path.join(ROOT, "tools")]
from full_time import timed  # noqa: E402
from ksched import MODE_EXACT, Engine, cluster  # noqa: E402
from ksched import _lib as L  # noqa: E402

ROWS = ("A", "W0", "R", "W1", "W2")
NODE_ROWS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--pods", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", default=",".join(ROWS), help="the rows to run, e.g. A,W0")
    a = ap.parse_args()
    only = a.only.split(",")
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
    p50s, derived = {}, {}
    us = lambda ms: ms / p * 1e3
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        e.save_state()

        def reload():
            e.load_spread(dom, skew)
            e.load_ext(node_ext)
            e.load_affinity(dom)

        ok = dict(gang_off=off, group=group, req_ext=req, **words)
        bad = dict(gang_off=off, group=group, req_ext=doomed, **words)
        calls = {"A": ("full, all four", lambda: e.schedule_full(rc, rm, rp, None, **ok)),
                 "W0": ("full_why, all four, nobody fails", lambda: e.schedule_full_why(rc, rm, rp, None, why_rows=p, **ok)),
                 "R": ("full, every gang rejected", lambda: e.schedule_full(rc, rm, rp, None, **bad)),
                 "W1": ("full_why, every gang rejected, counts only",
                        lambda: e.schedule_full_why(rc, rm, rp, None, why_rows=p, node_rows=0, **bad)),
                 "W2": (f"full_why, every gang rejected, {NODE_ROWS} node rows",
                        lambda: e.schedule_full_why(rc, rm, rp, None, why_rows=p, node_rows=NODE_ROWS, **bad))}
        for rep in range(a.reps):
            med = {}
            for row in ROWS:
                if row not in only:
                    continue
                name, fn = calls[row]
                wall, dev, out = timed(e, fn, a.calls, a.warmup, reload)
                med[row] = statistics.median(dev)
                nofit = int((out[0] == L.NO_FIT).sum())
                r = dict(rep=rep, row=row, case=name, nodes=n, pods=p, calls=a.calls, placed=int((out[0] >= 0).sum()),
                         rejected=int((out[0] == L.GANG_REJECTED).sum()), nofit=nofit,
                         wall_us_per_pod=dict(p50=us(statistics.median(wall)), min=us(min(wall)), max=us(max(wall))),
                         device_us_per_pod=dict(p50=us(med[row]), min=us(min(dev)), max=us(max(dev))))
                if len(out) > 4:  # the new call: what it recorded must be what the outputs say
                    wpod, counts, reasons, total = out[4]
                    assert total == nofit and wpod.tolist() == np.flatnonzero(out[0] == L.NO_FIT).tolist()
                    assert (counts[:, 0] == 0).all() and (counts.sum(axis=1) == n).all()
                    r["recorded"], r["node_rows"] = len(wpod), 0 if reasons is None else len(reasons)
                p50s.setdefault(row, []).append(us(med[row]))

                def derive(key, value):
                    r[key] = value
                    derived.setdefault(key, []).append(value)
                if row == "W0" and "A" in med:
                    derive("W0/A", med["W0"] / med["A"])
                if row == "W1" and "R" in med and nofit:
                    derive("(W1-R)/nofit, us", (med["W1"] - med["R"]) * 1e3 / nofit)
                if row == "W2" and "W1" in med and r.get("node_rows"):
                    derive("(W2-W1)/node_row, us", (med["W2"] - med["W1"]) * 1e3 / r["node_rows"])
                print(json.dumps(r), flush=True)
    print(json.dumps(dict(summary=True, device_p50_us_per_pod={k: [min(v), max(v)] for k, v in p50s.items()},
                          derived={k: [min(v), max(v)] for k, v in derived.items()})), flush=True)


if __name__ == "__main__":
    main()
