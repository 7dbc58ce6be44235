"""The screened scan's tail (score_role in ksched_pipe.hip: pass 2's per-lane row masks, the pair lists whose
threads rank the pair they scored, the row path built from the masks) against the CPU oracle, bit-exact, at the
geometries where those paths change: c4's rows per wave, both chunk_topk instantiations, pods with a dozen tied
pairs, pods past the pair cap, partial row steps, short waves, inactive lanes, labels and a feasible domain, the
screen-off rule, and both environment fall-backs.
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_same, run_engine

pytestmark = pytest.mark.gpu

C4_KW = dict(topk=16, batch=64, pipe_wgs=27)  # 3 score workgroups: 1,290 nodes give c4's 430 rows each


@functools.lru_cache(maxsize=None)
def _case(name, nn, pp):
    """(cluster, oracle result), computed once per shape and shared (never modified)."""
    import oracle as O
    from ksched import cluster
    cl = cluster.make_cluster(name, n_nodes=nn, n_pods=pp)
    return cl, O.schedule(cl, nthreads=8)


def tie_cluster(n_nodes=1290, n_pods=640, run=24):
    """Resource priority, all-node domain: allocatables in runs of `run` identical nodes, pods of 4 request shapes.
    Node j is row j // 3 of score workgroup j % 3 (pipe_wgs=27); the runs are interleaved so that every run lies
    half in one workgroup and half in the next, its rows `nruns * 2 / 3` apart.  A pod's best run gives a workgroup
    a dozen tied pairs, ranked by node index alone, and nearby runs add more: a pod's list reaches ~24 pairs (under
    the cap of 48) and a workgroup's batch several hundred pairs, a different number in each of the three."""
    from ksched import cluster
    nruns = (n_nodes + run - 1) // run
    per_wg = nruns * 2 // 3  # runs a workgroup holds a half of
    w, i = np.arange(n_nodes) % 3, np.arange(n_nodes) // 3
    kind = (i % per_wg + (nruns // 3) * w) % nruns
    cpu = (4000 + 250 * kind).astype(np.int64)
    mem = ((8 << 20) + (kind % 6) * (2 << 20)).astype(np.int64)
    pods = np.full(n_nodes, 110, dtype=np.int64)
    shapes = np.array([[100, 128 << 10, 1], [250, 512 << 10, 1], [500, 256 << 10, 2], [50, 1024 << 10, 3]], dtype=np.int64)
    s = shapes[np.arange(n_pods) % 4]
    return cluster.Cluster(name="ties", alloc_cpu=cpu, alloc_mem=mem, alloc_pods=pods, req_cpu=s[:, 0].copy(),
                           req_mem=s[:, 1].copy(), req_pods=s[:, 2].copy(), priority=cluster.PRIORITY_RESOURCE,
                           domain=cluster.DOMAIN_ALL, use_labels=False, mode="batched")


def same_cluster(n_nodes=600, n_pods=640):
    """Every node identical: every pair of a batch ties, every pod's needed rows pass the pair cap."""
    from ksched import cluster
    one = lambda v: np.full(n_nodes, v, dtype=np.int64)  # noqa: E731
    s = np.array([[100, 128 << 10, 1], [250, 512 << 10, 1]], dtype=np.int64)[np.arange(n_pods) % 2]
    return cluster.Cluster(name="same", alloc_cpu=one(16000), alloc_mem=one(32 << 20), alloc_pods=one(110),
                           req_cpu=s[:, 0].copy(), req_mem=s[:, 1].copy(), req_pods=s[:, 2].copy(),
                           priority=cluster.PRIORITY_RESOURCE, domain=cluster.DOMAIN_ALL, use_labels=False, mode="batched")


def check(cl, want, label, **kw):
    from ksched import MODE_BATCHED
    got = run_engine(cl, MODE_BATCHED, **kw)
    assert_same(got, want, label)
    assert got[4]["pipeline"] == "persistent", got[4]
    return got[4]


def test_c4_geometry(gpu_available, oracle_mod):
    cl, want = _case("c4", 1290, 2000)
    check(cl, want, "c4 1290x2000", **C4_KW)


def test_chunk_topk_8(gpu_available, oracle_mod):
    cl, want = _case("c4", 1290, 2000)
    check(cl, want, "c4 1290x2000 KC=8", chunk_topk=8, **C4_KW)


@pytest.mark.parametrize("run", [24, 28], ids=["runs_of_24", "runs_of_28"])
def test_ties_ranked_by_node_index(gpu_available, oracle_mod, run):
    """Between them the two clusters take all three paths after pass 2 (measured with the phase trace, which counts
    workgroup 0's pairs, and estimated for the others on the CPU): runs of 24 give workgroup 0 ~640 pairs per batch --
    all in flight at once, a thread ranks the pair it scored -- and the other two workgroups 900-960, past the ranking
    waves' 704 lanes: their rank loop finds its pairs again.  Runs of 28 give workgroup 0 ~730 pairs and one
    workgroup more than 1,024: the row path.  The engine's statistics carry no pair counts, so the path is not
    asserted here; tests/test_scan_tail_host.py holds the two rank forms against each other at the boundary."""
    cl = tie_cluster(run=run)
    check(cl, oracle_mod.schedule(cl, nthreads=8), f"ties, runs of {run}", **C4_KW)


def test_overflow_takes_the_row_path(gpu_available, oracle_mod):
    cl = same_cluster()
    check(cl, oracle_mod.schedule(cl, nthreads=8), "all nodes identical", **C4_KW)


@pytest.mark.parametrize("nn,pp,kw", [(1291, 2000, C4_KW), (100, 2000, C4_KW), (1290, 1000, C4_KW)],
                         ids=["partial_step_431_430", "short_waves_100_nodes", "last_batch_40_lanes"])
def test_geometry_edges(gpu_available, oracle_mod, nn, pp, kw):
    cl, want = _case("c4", nn, pp)
    check(cl, want, f"c4 {nn}x{pp}", **kw)


def test_c5_labels_feasible_domain(gpu_available, oracle_mod):
    cl, want = _case("c5", 2000, 2000)
    check(cl, want, "c5 2000x2000", topk=16, batch=64)


def test_c5hc_screen_off_rule(gpu_available, oracle_mod):
    cl, want = _case("c5hc", 2000, 3000)
    check(cl, want, "c5hc 2000x3000", topk=16, batch=64)


@pytest.mark.parametrize("knob", ["KSCHED_NO_PAIRS", "KSCHED_NO_SCREEN"])
def test_env_fallbacks(gpu_available, oracle_mod, monkeypatch, knob):
    monkeypatch.setenv(knob, "1")
    cl, want = _case("c4", 1290, 2000)
    check(cl, want, f"c4 1290x2000 {knob}=1", **C4_KW)
