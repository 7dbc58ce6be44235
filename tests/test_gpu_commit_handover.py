"""The persistent commit loads the mergers' inherited keys before its merges' wait once their own count (Ctl::inh_done)
shows them, and after the wait otherwise -- the older path is the fallback.  Every case is bit-exact against the CPU
oracle (node index, score bits, feasible count, final node state) with the part on and switched off
(KSCHED_NO_EARLY_INH), and under KSCHED_JITTER, which drives both orders of the new race (sites 110, 111).  The count
of batches the early load served comes from Engine.commit_stamps()."""
import functools

import pytest

from test_gpu_parity import assert_same, run_engine

pytestmark = pytest.mark.gpu

# the shapes of test_gpu_commit_conflict.py (voided and truncated batches, rescues, follow-one-node chains), a ring
# wrap with a partial last batch (9 full batches + 17 pods: every 4-deep ring reused twice) and empty exports (once
# c5's 64 nodes are full no pod is placed: n1 = n2 = 0, nothing to load early, idle records)
SHAPES = {"c5hc": ("c5hc", 2000, 3000), "c3": ("c3", 200, 2000), "c2": ("c2", 100, 1500), "c4": ("c4", 1000, 4000),
          "wrap": ("c4", 300, 593), "empty": ("c5", 64, 700)}
OFF = {"on": (), "no_inh": ("KSCHED_NO_EARLY_INH",)}


@functools.lru_cache(maxsize=None)
def case(name):
    """the cluster and the oracle's answer, computed once and shared (neither is modified)"""
    import oracle as O
    from ksched import cluster
    gen, nn, pp = SHAPES[name]
    cl = cluster.make_cluster(gen, n_nodes=nn, n_pods=pp)
    return cl, O.schedule(cl, nthreads=8)


def check(name, label):
    from ksched import MODE_BATCHED
    cl, want = case(name)
    got = run_engine(cl, MODE_BATCHED, topk=16, batch=64)
    assert_same(got, want, f"{name}/{label}")
    assert got[4]["pipeline"] == "persistent", got[4]
    return got[4]


def run_counted(name, label):
    """as check(), with the commit's counts of the run (the context must be created under KSCHED_COMMIT_STAMPS)"""
    from ksched import MODE_BATCHED, Engine
    cl, want = case(name)
    with Engine(mode=MODE_BATCHED, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, topk=16, batch=64) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
        oi, os_, of = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        got = (oi, os_, of, e.read_nodes(), e.stats())
        cnt = e.commit_stamps()
    assert_same(got, want, f"{name}/{label}")
    assert got[4]["pipeline"] == "persistent", got[4]
    print(f"{name}/{label}: {cnt}")
    return cnt


def test_ring_wrap_partial_last_batch(gpu_available, oracle_mod):
    cl, want = case("wrap")
    assert cl.req_cpu.shape[0] % 64 == 17
    check("wrap", "on")


def test_empty_exports(gpu_available, oracle_mod):
    cl, want = case("empty")
    assert int((want[0] < 0).sum()) > 128  # whole batches that place nothing
    check("empty", "on")


@pytest.mark.parametrize("off", list(OFF))
@pytest.mark.parametrize("name", ["c5hc", "c3", "c2"])
def test_conflict_shapes_parts_on_and_off(gpu_available, oracle_mod, monkeypatch, name, off):
    for v in OFF[off]:
        monkeypatch.setenv(v, "1")
    check(name, off)


@pytest.mark.parametrize("seed", [3, 11, 29])
def test_both_orders_under_jitter(gpu_available, oracle_mod, monkeypatch, seed):
    monkeypatch.setenv("KSCHED_JITTER", str(seed))
    check("c3", f"jitter{seed}")


def test_early_reads_serve_batches(gpu_available, oracle_mod, monkeypatch):
    """without jitter the early load serves some batches; under jitter not all that tried, so the fallback ran too"""
    monkeypatch.setenv("KSCHED_COMMIT_STAMPS", "1")
    cnt = run_counted("c4", "stamps")
    assert cnt["batches"] > 0 and cnt["early_inh"] > 0, cnt
    monkeypatch.setenv("KSCHED_JITTER", "7")
    cnt = run_counted("c4", "stamps_jitter")
    assert cnt["early_inh"] < cnt["early_inh_tried"] <= cnt["batches"] + 2, cnt  # (+ voided batches: they tried too)


def test_rank_group_on_one_device(gpu_available, oracle_mod):
    """R = 2 local ranks: each rank's commit loads its inherited keys early, behind the rank merge"""
    from test_gpu_xchg import check_oracle, run_local
    cl, want = case("c4")
    check_oracle(cl, run_local(cl, 2, calls=1), want, 2)
