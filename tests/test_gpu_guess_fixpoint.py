"""The commit's two-tier guess step on the device (tests/test_guess_fixpoint_host.py states it): lists that send the
wave into the full K-entry scan, bit for bit against the CPU statements.

k_commit_spc alone (ksched_selftest_commit): the "same" family of tests/commit_ref.py -- one list shared by every pod,
so pods 2.. find their two lowest entries proposed by earlier pods -- and the "every0" family -- a node every pod
ranks first, inherited from the previous export, at the head of every list -- at K = 4, 8, 16 and nb = 1, 37, 64.

The persistent pipeline: identical pods on identical nodes (with and without zero-request pods mixed in) and
random_small's edge states, universes of at most 1,200 nodes and 4-8 batches of 64, against the oracle; the commit's
counters (KSCHED_COMMIT_STAMPS) show that the cases reach multi-round batches, failed guesses, pods resolved one by one
and guess iterations that took the full scan."""
import functools

import numpy as np
import pytest

import commit_ref as CR
from test_gpu_commit_alone import _first_diff, _want, dev  # noqa: F401  (dev: the module's fixture)
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nb", [1, 37, 64])
@pytest.mark.parametrize("K", CR.KS)
@pytest.mark.parametrize("family", ["same", "every0"])
def test_commit_spc_alone_shared_lists(dev, oracle_mod, family, K, nb):  # noqa: F811
    O = oracle_mod
    cases = [c for c in CR.commit_cases(O, 64) if c.family == family and c.K == K and c.nb == nb]
    assert len(cases) == len(CR.LADDER)
    bad = []
    for c in cases:
        want, done = _want(O, c)
        d = _first_diff(dev.commit(CR.COMMIT_SPECULATIVE, c), want, done)
        if d:
            bad.append(f"k_commit_spc {c.name}: {d}")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ:\n" + "\n".join(bad[:12])


def _identical(n_nodes, n_pods, zero_mix):
    from ksched import cluster
    i = np.arange(n_pods)
    z = (i % 3 == 0) if zero_mix else np.zeros(n_pods, bool)
    return cluster.Cluster(name=f"same{n_nodes}", alloc_cpu=np.full(n_nodes, 4000, np.int64),
                           alloc_mem=np.full(n_nodes, 8388608, np.int64), alloc_pods=np.full(n_nodes, 110, np.int64),
                           req_cpu=np.where(z, 0, 200).astype(np.int64), req_mem=np.where(z, 0, 65536).astype(np.int64),
                           req_pods=np.ones(n_pods, np.int64))


CASES = {
    "same_33x320": lambda: _identical(33, 320, False),
    "same_33x320_zero": lambda: _identical(33, 320, True),
    "same_1200x512": lambda: _identical(1200, 512, False),
    "same_1200x448_zero": lambda: _identical(1200, 448, True),
    "edge_300x384": lambda: __import__("ksched").cluster.random_small(41, n_nodes=300, n_pods=384),
    "edge_1200x512": lambda: __import__("ksched").cluster.random_small(42, n_nodes=1200, n_pods=512),
}


@functools.lru_cache(maxsize=None)
def run(name):
    """the case through the persistent pipeline under KSCHED_COMMIT_STAMPS, and the oracle's answer: computed once"""
    import oracle as O
    from ksched import MODE_BATCHED, Engine
    cl = CASES[name]()
    want = O.schedule(cl, nthreads=8)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("KSCHED_COMMIT_STAMPS", "1")
        with Engine(mode=MODE_BATCHED, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, topk=16,
                    batch=64) as e:
            e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
            oi, os_, of = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
            got = (oi, os_, of, e.read_nodes(), e.stats())
            cnt = e.commit_stamps()
    return got, want, cnt


@pytest.mark.parametrize("name", list(CASES))
def test_pipeline_is_the_oracle(gpu_available, oracle_mod, name):
    got, want, cnt = run(name)
    print(f"{name}: {cnt} | batches {got[4]['batches']} truncations {got[4]['truncations']} rescues {got[4]['rescues']}")
    assert_same(got, want, name)
    assert got[4]["pipeline"] == "persistent", got[4]
    assert 4 <= -(-len(want[0]) // 64) <= 8


def test_pipeline_cases_reach_the_paths(gpu_available, oracle_mod):
    cnts = {name: run(name)[2] for name in CASES}
    tot = {k: sum(c[k] for c in cnts.values()) for k in ("rounds", "batches", "failed_guesses", "one_by_one", "full_scans")}
    print(tot)
    assert any(c["rounds"] > c["batches"] > 0 for c in cnts.values()), cnts   # more than one round per batch
    assert tot["failed_guesses"] > 0 and tot["one_by_one"] > 0 and tot["full_scans"] > 0, cnts
