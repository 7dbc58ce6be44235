"""The seeded score scan (score_role in ksched_pipe.hip, KC <= 4 kernels): each score workgroup takes its bound from the
rows the previous batch needed, then makes one pass over all rows against it.  Every case is bit-exact against the
CPU oracle (node index, score bits, feasible count, final node state): which rows seed must never show in a result.
The counters (Engine.seed_stats) say which form ran.

(An allocatable >= 2^52 takes the call off the FAST53 kernels, which are the only screened ones, so on the device the
unscreenable rows are those with a zero allocatable; tests/test_seed_bound_host.py covers both on the CPU statement.)
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

C4_KW = dict(topk=16, batch=64, pipe_wgs=27)  # 3 score workgroups: 1,290 nodes give c4's 430 rows each


@functools.lru_cache(maxsize=None)
def _case(name, nn, pp):
    """(cluster, oracle result), computed once per shape and shared (never modified)."""
    import oracle as O
    from ksched import cluster
    cl = cluster.make_cluster(name, n_nodes=nn, n_pods=pp)
    return cl, O.schedule(cl, nthreads=8)


def run(cl, calls=1, **kw):
    """`calls` schedule calls on one engine from the same node state: [(results + stats, seed counters)] per call."""
    from ksched import MODE_BATCHED, Engine
    out = []
    with Engine(mode=MODE_BATCHED, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, **kw) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
        e.save_state()
        for c in range(calls):
            if c:
                e.restore_state()
            oi, os_, of = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
            out.append(((oi, os_, of, e.read_nodes(), e.stats()), e.seed_stats()))
    return out


def check(cl, want, label, **kw):
    got, seeds = run(cl, **kw)[0]
    print(f"{label}: {seeds} | exact_rows {got[4]['exact_rows']} scan_rows {got[4]['scan_rows']} batches "
          f"{got[4]['batches']} truncations {got[4]['truncations']}")
    assert_same(got, want, label)
    assert got[4]["pipeline"] == "persistent", got[4]
    return got[4], seeds


def scans(stats, rows_per_wg):
    """(workgroup, batch) scans of a run whose workgroups all hold rows_per_wg rows"""
    assert stats["scan_rows"] % rows_per_wg == 0
    return stats["scan_rows"] // rows_per_wg


# ---- c4's geometry, the switches ----------------------------------------------------------------------------------------
def test_c4_geometry_seeds_from_masks(gpu_available, oracle_mod):
    cl, want = _case("c4", 1290, 2000)
    st, seeds = check(cl, want, "c4 1290x2000", **C4_KW)
    n = scans(st, 430)
    # All scans but each workgroup's first seed from the previous batch's needed rows, a few dozen of its 430 -- except
    # where that mask passed the cap (a quarter of the rows: a pod that ties on most nodes needs most rows), which by
    # the scan's own rule seeds from all rows.  No batch of this case runs unscreened.  (510 and 15 of 525.)
    assert seeds["seeded_scans"] + seeds["past_cap"] == n - 3 and seeds["after_unscreened"] == 0, (seeds, n)
    assert seeds["seeded_scans"] >= 0.85 * (n - 3), (seeds, n)
    assert seeds["seed_rows"] < 3 * 430 + (n - 3) * 108, (seeds, n)  # (a mask past a quarter of the rows is not used)
    assert seeds["zero_bound_scans"] == 0, seeds


def test_no_seed_switch(gpu_available, oracle_mod, monkeypatch):
    monkeypatch.setenv("KSCHED_NO_SEED", "1")
    cl, want = _case("c4", 1290, 2000)
    st, seeds = check(cl, want, "c4 1290x2000 KSCHED_NO_SEED=1", **C4_KW)
    assert seeds["seeded_scans"] == 0 and seeds["seed_rows"] == st["scan_rows"], (seeds, st)


def test_no_pairs_row_path_keeps_the_masks(gpu_available, oracle_mod, monkeypatch):
    """the exact phase by rows in every batch: the masks are built all the same and seed the next scan"""
    monkeypatch.setenv("KSCHED_NO_PAIRS", "1")
    cl, want = _case("c4", 1290, 2000)
    st, seeds = check(cl, want, "c4 1290x2000 KSCHED_NO_PAIRS=1", **C4_KW)
    assert seeds["seeded_scans"] > 0, seeds


@pytest.mark.parametrize("knob,val", [("KSCHED_POISON", "1"), ("KSCHED_JITTER", "5")])
def test_poison_and_jitter(gpu_available, oracle_mod, monkeypatch, knob, val):
    monkeypatch.setenv(knob, val)
    cl, want = _case("c4", 1290, 2000)
    st, seeds = check(cl, want, f"c4 1290x2000 {knob}={val}", **C4_KW)
    assert seeds["seeded_scans"] > 0, seeds


def test_two_calls_reset_the_masks(gpu_available, oracle_mod):
    cl, want = _case("c4", 1290, 2000)
    (g0, s0), (g1, s1) = run(cl, calls=2, **C4_KW)
    assert_same(g0, want, "call 0")
    assert_same(g1, want, "call 1")
    assert s0 == s1 and s0["seeded_scans"] > 0, (s0, s1)
    assert g0[4]["exact_rows"] == g1[4]["exact_rows"], (g0[4], g1[4])


def test_rank_group_on_one_device(gpu_available, oracle_mod):
    """R = 2 local ranks on the c4 shape: each rank's score workgroups seed on their own"""
    from test_gpu_xchg import check_oracle, run_local
    cl, want = _case("c4", 1290, 2000)
    check_oracle(cl, run_local(cl, 2, calls=1), want, 2)


# ---- poor seeds ---------------------------------------------------------------------------------------------------------
def alternating_cluster(n_nodes=1290, n_pods=1280):
    """Pods alternate batch by batch between CPU-heavy and memory-heavy requests; half of the nodes are CPU-rich and
    memory-poor, half the other way round: the rows a batch needs are the wrong ones for the next."""
    from ksched import cluster
    rng = np.random.default_rng(7)
    rich = (np.arange(n_nodes) // 3) % 2 == 0  # by row, so every workgroup holds both kinds
    cpu = np.where(rich, 64000, 8000) - rng.integers(0, 2000, n_nodes)
    mem = np.where(rich, 16 << 20, 128 << 20) - rng.integers(0, 1 << 20, n_nodes)
    heavy_cpu = (np.arange(n_pods) // 64) % 2 == 0
    rc = np.where(heavy_cpu, 2000, 100) + 50 * rng.integers(0, 8, n_pods)
    rm = (np.where(heavy_cpu, 64, 4096) + rng.integers(0, 64, n_pods)) << 10
    return cluster.Cluster(name="alternating", alloc_cpu=cpu.astype(np.int64), alloc_mem=mem.astype(np.int64),
                           alloc_pods=np.full(n_nodes, 110, np.int64), req_cpu=rc.astype(np.int64),
                           req_mem=rm.astype(np.int64), req_pods=np.ones(n_pods, np.int64),
                           priority=cluster.PRIORITY_RESOURCE, domain=cluster.DOMAIN_ALL, use_labels=False, mode="batched")


def test_alternating_pod_shapes(gpu_available, oracle_mod):
    cl = alternating_cluster()
    st, seeds = check(cl, oracle_mod.schedule(cl, nthreads=8), "alternating shapes", **C4_KW)
    assert seeds["seeded_scans"] > 0 and seeds["seed_rows"] < st["scan_rows"], (seeds, st)  # masks, not all rows


def tie_cluster(n_nodes=1290, n_pods=640, run=24):
    """tests/test_gpu_scan_tail.py's cluster of runs of identical nodes: dense masks, pods with two dozen tied pairs."""
    from ksched import cluster
    nruns = (n_nodes + run - 1) // run
    per_wg = nruns * 2 // 3
    w, i = np.arange(n_nodes) % 3, np.arange(n_nodes) // 3
    kind = (i % per_wg + (nruns // 3) * w) % nruns
    cpu = (4000 + 250 * kind).astype(np.int64)
    mem = ((8 << 20) + (kind % 6) * (2 << 20)).astype(np.int64)
    shapes = np.array([[100, 128 << 10, 1], [250, 512 << 10, 1], [500, 256 << 10, 2], [50, 1024 << 10, 3]], dtype=np.int64)
    s = shapes[np.arange(n_pods) % 4]
    return cluster.Cluster(name="ties", alloc_cpu=cpu, alloc_mem=mem, alloc_pods=np.full(n_nodes, 110, dtype=np.int64),
                           req_cpu=s[:, 0].copy(), req_mem=s[:, 1].copy(), req_pods=s[:, 2].copy(),
                           priority=cluster.PRIORITY_RESOURCE, domain=cluster.DOMAIN_ALL, use_labels=False, mode="batched")


def same_cluster(n_nodes=600, n_pods=640):
    """Every node identical: every pod's needed rows pass the pair cap -- the row path, after a seeded L too."""
    from ksched import cluster
    one = lambda v: np.full(n_nodes, v, dtype=np.int64)  # noqa: E731
    s = np.array([[100, 128 << 10, 1], [250, 512 << 10, 1]], dtype=np.int64)[np.arange(n_pods) % 2]
    return cluster.Cluster(name="same", alloc_cpu=one(16000), alloc_mem=one(32 << 20), alloc_pods=one(110),
                           req_cpu=s[:, 0].copy(), req_mem=s[:, 1].copy(), req_pods=s[:, 2].copy(),
                           priority=cluster.PRIORITY_RESOURCE, domain=cluster.DOMAIN_ALL, use_labels=False, mode="batched")


@pytest.mark.parametrize("run_len", [24, 28], ids=["runs_of_24", "runs_of_28"])
def test_tie_clusters(gpu_available, oracle_mod, run_len):
    cl = tie_cluster(run=run_len)
    st, seeds = check(cl, oracle_mod.schedule(cl, nthreads=8), f"ties, runs of {run_len}", **C4_KW)
    assert seeds["seeded_scans"] > 0, seeds  # the seeded form ran on this geometry


def test_identical_nodes_row_path(gpu_available, oracle_mod):
    cl = same_cluster()
    st, seeds = check(cl, oracle_mod.schedule(cl, nthreads=8), "all nodes identical", **C4_KW)
    # while most nodes are untouched every pod needs most rows: that mask is past the cap (or the screen is off for a
    # while) and the next scan seeds from all rows; the first batch's is one such
    assert seeds["past_cap"] + seeds["after_unscreened"] > 0, seeds


# ---- fewer than KC usable seeds -----------------------------------------------------------------------------------------
def test_thirty_nodes(gpu_available, oracle_mod):
    """so few nodes go to ONE score workgroup whatever pipe_wgs allows: 30 rows, waves of two or three"""
    cl, want = _case("c4", 30, 700)
    st, seeds = check(cl, want, "c4 30x700", **C4_KW)
    # the cap is 7 rows: 64 pods need more, so the screened scans seed from all 30 (a few batches run unscreened)
    assert seeds["past_cap"] > 0 and seeds["seed_rows"] % 30 == 0, seeds


def unscreenable_cluster(n_nodes=60, n_pods=640):
    """Only three nodes have a screen that can bound: the others have a zero allocatable (NaN reciprocal) or a CPU
    allocatable equal to every pod's request (fraction exactly 1: ambiguous).  However the engine deals the 60 nodes
    to score workgroups (so few go to one), none has KC = 4 lower bounds: L = 0 for every pod, everything is scored
    exactly."""
    from ksched import cluster
    rng = np.random.default_rng(11)
    row = np.arange(n_nodes) // 3
    cpu = np.full(n_nodes, 500, np.int64)            # == the request: fraction 1
    mem = np.full(n_nodes, 64 << 20, np.int64) - rng.integers(0, 1 << 20, n_nodes)
    pods = np.full(n_nodes, 110, np.int64)
    mem[row % 3 == 1] = 0                            # NaN screens
    pods[row % 5 == 2] = 0
    good = np.arange(n_nodes) < 3
    cpu[good] = 32000 - 100 * np.arange(int(good.sum()))
    mem[good] = 128 << 20
    pods[good] = 110
    return cluster.Cluster(name="unscreenable", alloc_cpu=cpu, alloc_mem=mem, alloc_pods=pods,
                           req_cpu=np.full(n_pods, 500, np.int64), req_mem=np.full(n_pods, 256 << 10, np.int64),
                           req_pods=np.ones(n_pods, np.int64), priority=cluster.PRIORITY_RESOURCE,
                           domain=cluster.DOMAIN_ALL, use_labels=False, mode="batched")


def test_unscreenable_best_rows_zero_bound(gpu_available, oracle_mod):
    cl = unscreenable_cluster()
    st, seeds = check(cl, oracle_mod.schedule(cl, nthreads=8), "unscreenable rows", **C4_KW)
    assert seeds["zero_bound_scans"] > 0, seeds


# ---- rows that die between batches, labels, a feasible domain -----------------------------------------------------------
def test_c5hc_feasible_domain_labels(gpu_available, oracle_mod):
    cl, want = _case("c5hc", 1290, 2000)
    st, seeds = check(cl, want, "c5hc 1290x2000", **C4_KW)
    # masks seed, and pods with fewer than KC feasible rows in a workgroup get L = 0
    assert seeds["seeded_scans"] > 0 and seeds["zero_bound_scans"] > 0, seeds


def test_c3_seeds_go_non_fitting(gpu_available, oracle_mod):
    """several pods per node: the rows a batch needed fill up and no longer fit the next batch's pods"""
    cl, want = _case("c3", 1290, 4000)
    st, seeds = check(cl, want, "c3 1290x4000", **C4_KW)
    assert seeds["seeded_scans"] > 0, seeds


# ---- partial geometry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn,pp", [(1283, 1000), (40, 1000)], ids=["partial_step_428_427", "short_waves_40_nodes"])
def test_partial_geometry_inactive_lanes(gpu_available, oracle_mod, nn, pp):
    """a partial last row step, waves without rows, and a last batch of 40 active lanes"""
    cl, want = _case("c4", nn, pp)
    st, seeds = check(cl, want, f"c4 {nn}x{pp}", **C4_KW)
    # 428 rows per workgroup: masks seed; 40 nodes on one workgroup: 64 pods need more than the cap of 10 rows
    assert seeds["seeded_scans" if nn == 1283 else "past_cap"] > 0, seeds
