"""The speculative commit where its guesses fail: clusters small enough that pods of one 64-pod batch keep picking a
node an earlier pod of the same batch picked, so batches take several guess rounds, resolve pods one by one, rescan
the touched slots and rescue or truncate.  Every case is bit-exact against the CPU oracle (node index, score bits,
feasible count, final node state), as in test_gpu_parity.py.

Same-batch repeats on the oracle's replay (pods per 64-pod batch that pick a node an earlier pod of the batch picked):
c5hc 2000 nodes x 3000 pods: mean 27, >= 8 in all 47 batches; c3 200 x 2000: mean 9.7, max 53, 347 pods fit nowhere;
c2 100 x 1500 (best price): mean 17; c4 1000 x 4000: mean 3.3, every pod placed.
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_same, run_engine

pytestmark = pytest.mark.gpu

SHAPES = {"c5hc": (2000, 3000), "c3": (200, 2000), "c2": (100, 1500), "c4": (1000, 4000)}


@functools.lru_cache(maxsize=None)
def case(name):
    """the cluster and the oracle's answer, computed once and shared (neither is modified)"""
    import oracle as O
    from ksched import cluster
    nn, pp = SHAPES[name]
    cl = cluster.make_cluster(name, n_nodes=nn, n_pods=pp)
    return cl, O.schedule(cl, nthreads=8)


def check(name, label, persistent=True, **kw):
    from ksched import MODE_BATCHED
    cl, want = case(name)
    got = run_engine(cl, MODE_BATCHED, **kw)
    assert_same(got, want, f"{name}/{label}")
    if persistent:
        assert got[4]["pipeline"] == "persistent", got[4]
    else:
        assert got[4]["pipeline"] in ("stream", "stream-sequential"), got[4]
    return got[4]


def traced(monkeypatch, tmp_path, name, **kw):
    """the case once more with the per-batch trace dumped: column 16 = rounds | rescues << 16 | resolved << 24 |
    failed guesses << 32 | pods resolved one by one << 48"""
    dump = tmp_path / "trace.bin"
    monkeypatch.setenv("KSCHED_PERSIST_TRACE", "1")
    monkeypatch.setenv("KSCHED_TRACE_DUMP", str(dump))
    check(name, "traced", **kw)
    c16 = np.fromfile(dump, dtype=np.uint64).reshape(-1, 54)[:, 16]
    rounds, seq = c16 & np.uint64(0xffff), c16 >> np.uint64(48)
    print(f"{name}: {int((rounds > 0).sum())} batches, rounds max {int(rounds.max())}, "
          f"one-by-one pods {int(seq.sum())}")
    assert (rounds > 1).any(), f"{name}: no batch took more than one guess round"
    assert (seq > 0).any(), f"{name}: no pod was resolved one by one"


def test_c5hc_persistent(gpu_available, oracle_mod):
    """cut lists, the touched-node screen on, follow-one-node chains, rescues"""
    st = check("c5hc", "k16_b64", topk=16, batch=64)
    print(f"c5hc: batches {st['batches']} truncations {st['truncations']} rescues {st['rescues']}")


def test_c5hc_no_touch_screen(gpu_available, oracle_mod, monkeypatch):
    """every touched slot keyed exactly"""
    monkeypatch.setenv("KSCHED_NO_TOUCH_SCREEN", "1")
    check("c5hc", "no_touch_screen", topk=16, batch=64)


def test_c5hc_no_rescue(gpu_available, oracle_mod, monkeypatch):
    """an exhausted cut list truncates its batch"""
    monkeypatch.setenv("KSCHED_RESCUE_MAX", "0")
    st = check("c5hc", "no_rescue", topk=16, batch=64)
    assert st["rescues"] == 0, st


def test_c5hc_stream(gpu_available, oracle_mod):
    """the stream pipeline's commit kernel: plain loads, lag 2"""
    from ksched._lib import PIPELINE_STREAM
    check("c5hc", "stream", persistent=False, topk=16, batch=64, pipeline=PIPELINE_STREAM)


@pytest.mark.parametrize("kw", [dict(topk=16, batch=64), dict(topk=4, batch=32, chunk_topk=4)], ids=["k16_b64", "k4_b32_c4"])
def test_c3_persistent(gpu_available, oracle_mod, kw):
    """three score workgroups, uncut lists (no screen threshold), pods predicted not to fit"""
    cl, want = case("c3")
    assert int((want[0] < 0).sum()) > 0  # pods that fit nowhere
    check("c3", str(kw), **kw)


def test_c2_best_price(gpu_available, oracle_mod):
    """the unscreened price path"""
    check("c2", "k16_b64", topk=16, batch=64)


def test_c4_mixed_rounds(gpu_available, oracle_mod):
    """single- and multi-round batches side by side: the window policy"""
    cl, want = case("c4")
    assert (want[0] >= 0).all()
    check("c4", "k16_b64", topk=16, batch=64)


@pytest.mark.parametrize("name", ["c5hc", "c3"])
def test_conflict_paths_are_exercised(gpu_available, oracle_mod, monkeypatch, tmp_path, name):
    """the cases above do run the multi-round and one-by-one paths (a later change cannot silently stop that)"""
    traced(monkeypatch, tmp_path, name, topk=16, batch=64)
