#!/usr/bin/env python3
"""Wall time of ksched_preempt on c4's 100k nodes with the bound pods its used pod slots stand for (0 .. 55 a node, ~27
on average): the call with its copies and its sync, a host clock around it, the median over --calls calls after
--warmup, for m = 1, 64 and 1024 pods (c4's pods sixteen times as large, priorities 300 .. 700).  Each m runs in a child process of its own under --timeout seconds, and the
first child that fails or runs out of time ends the run.  Per case one JSON line: ms per call, the bytes of the table
columns the scan reads (cpu, mem, prio: 20 B an entry, padding included), the pod tiles that each read them, and
table bytes x tiles per second -- to set against the HBM floor (table bytes x tiles / 8 TB/s).
    python tools/preempt_time.py [--calls 20] [--warmup 3] [--m 1 64 1024]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "k8s-scheduler_amd")]

TILE = 4            # kPreemptTile (csrc/ksched_preempt.h)
ENTRY_BYTES = 20    # cpu + mem + prio of one table entry
HBM_BYTES_PER_S = 8e12


def table(cl, seed=1):
    """The bound pods behind c4's used pod slots (capacity 110 a node), shuffled, with priorities 0 .. 500."""
    import numpy as np
    r = np.random.default_rng(seed)
    seg = 110 - cl.alloc_pods
    node = np.repeat(np.arange(cl.n_nodes), seg)
    node = node[r.permutation(node.size)].astype(np.int32)
    nb = node.size
    return seg, (node, r.integers(1, 41, nb) * 50, r.integers(64, 4097, nb) * 1024, r.integers(0, 6, nb).astype(np.int32) * 100)


def padded_entries(seg):
    import numpy as np
    pad = np.zeros((len(seg) + 63) // 64 * 64, np.int64)
    pad[:len(seg)] = seg
    return int(pad.reshape(-1, 64).max(axis=1).sum()) * 64


def run_case(a, m):
    import numpy as np
    from ksched import MODE_EXACT, Engine, cluster
    cl = cluster.make_cluster("c4", n_nodes=a.nodes, n_pods=max(m, 1))
    seg, bound = table(cl)
    prio = (np.random.default_rng(2).integers(3, 8, m) * 100).astype(np.int32)
    with Engine(mode=MODE_EXACT, priority=cl.priority, domain=cl.domain) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods)
        t0 = time.perf_counter()
        e.load_bound(*bound)
        load_ms = (time.perf_counter() - t0) * 1e3
        # c4's pods sixteen times as large: some fit as things are, some need victims, some fit nowhere (the scan's
        # work does not depend on which: it walks every slot for every pod)
        rc, rm, rp = cl.req_cpu[:m] * 16, cl.req_mem[:m] * 16, cl.req_pods[:m]
        fn = lambda: e.preempt(rc, rm, rp, None, prio, vcap=16)
        for _ in range(a.warmup):
            out = fn()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    p50 = statistics.median(ts)
    entries = padded_entries(seg)
    tiles = (m + TILE - 1) // TILE
    tb = entries * ENTRY_BYTES
    print(json.dumps(dict(case=f"m={m}", nodes=cl.n_nodes, bound_pods=int(seg.sum()), calls=a.calls,
                          preempt_ms=dict(p50=p50, min=min(ts), max=max(ts)), load_bound_ms=load_ms,
                          table_bytes=tb, padding_factor=entries / max(int(seg.sum()), 1), pod_tiles=tiles,
                          table_bytes_x_tiles_per_s=tb * tiles / (p50 * 1e-3), hbm_floor_ms=tb * tiles / HBM_BYTES_PER_S * 1e3,
                          no_fit=int((out[0] < 0).sum()), with_victims=int((out[1] > 0).sum()))), flush=True)


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
