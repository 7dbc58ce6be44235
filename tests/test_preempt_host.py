"""ksched_preempt without a device: the library exports the calls, the plain-Python restatement (preempt_ref) passes a
hand-worked example, shard answers merge into the one-shard answer, and the kube-JSON reader sees spec.priority.
(FakeCluster.preempt_pod needs an engine: tests/test_gpu_preempt.py.)"""
import numpy as np

import preempt_ref as PR

B = 1 << 31


def test_library_exports_preempt_symbols():
    from ksched import _lib as L
    lb = L.lib()
    assert hasattr(lb, "ksched_load_bound") and hasattr(lb, "ksched_preempt")
    assert L.BOUND_MAX_PER_NODE == 1024 and L.PREEMPT_NO_VICTIM_PRIO == -(1 << 31) == PR.NO_VICTIM_PRIO
    assert lb.ksched_abi_version() == 6  # added within ABI 6: callers probe for the symbols


def test_state_errors_need_no_device():
    """A NULL context is refused before anything touches a device."""
    from ksched import _lib as L
    assert L.lib().ksched_load_bound(None, 0, None, None, None, None) == L.E_INVALID
    assert L.lib().ksched_preempt(None, 0, None, None, None, None, None, 1, None, None, None, None, None, None) == L.E_INVALID


def hand_example():
    """3 nodes, 6 bound pods; memory and pod slots never bind (every node has 1 MiB and 10 slots free).

        node  alloc cpu   its pods as (table index, cpu, prio)
        0     400         (1, 600, 200)  (3, 500, 100)
        1     0           (2, 500, 200)  (4, 500, 50)
        2     400         (5, 600, 200)  (0, 500, 100)

    Pod A asks 1000 cpu at priority 1000: every bound pod is a potential victim.
      node 0: free = 400 + 600 + 500 = 1500.  Walk 1 (prio 200): 1500 - 600 = 900 < 1000, a victim.  Walk 3 (prio
              100): 1500 - 500 = 1000 fits, REPRIEVED.  Key (200, 200 + 2^31, 1), victims [1].
      node 1: free = 1000.  Walk 2: 500 < 1000, victim.  Walk 4: 1000 - 500 < 1000, victim.  Key (200, 250 + 2^32, 2),
              victims [2, 4]: ties node 0 on the max priority, loses on the sum.
      node 2: node 0 again with other table indices: key (200, 200 + 2^31, 1), victims [5]: ties node 0 on every
              field, loses on the node index.
      Answer: node 0, 1 victim, max 200, sum 200 + 2^31, 3 candidates, victims [1].
    Pod B asks the same at priority 150: only the pods below 150 may go.  Node 0: 400 + 500 = 900, node 1: 500,
      node 2: 900 -- no candidate: NO_FIT.
    Pod C asks 400 cpu at priority 1000.  Nodes 0 and 2 fit as they are: every pod is reprieved, key (no victim, 0, 0);
      node 1 reprieves pod 2 (1000 - 500 >= 400) and loses pod 4 (500 - 500 < 400): key (50, ...).  Answer: node 0,
      no victim, 3 candidates."""
    alloc = (np.array([400, 0, 400]), np.full(3, 1 << 20), np.full(3, 10))
    bound = (np.array([2, 0, 1, 0, 1, 2], np.int32), np.array([500, 600, 500, 500, 500, 600]), np.zeros(6, np.int64),
             np.array([100, 200, 200, 100, 50, 200], np.int32))
    pods = (np.array([1000, 1000, 400]), np.zeros(3, np.int64), np.ones(3, np.int64), np.array([1000, 150, 1000], np.int32))
    return alloc, bound, pods


def test_reference_hand_example():
    alloc, bound, pods = hand_example()
    seg = {j: [(t, int(bound[1][t]), 0, int(bound[3][t])) for t in range(6) if bound[0][t] == j] for j in range(3)}
    row = lambda j: (int(alloc[0][j]), 1 << 20, 10)
    a = (1000, 0, 1)
    assert PR.node_key(a, 1000, row(0), seg[0]) == ((200, 200 + B, 1), [1])
    assert PR.node_key(a, 1000, row(1), seg[1]) == ((200, 250 + 2 * B, 2), [2, 4])
    assert PR.node_key(a, 1000, row(2), seg[2]) == ((200, 200 + B, 1), [5])
    assert all(PR.node_key(a, 150, row(j), seg[j]) is None for j in range(3))
    assert PR.node_key((400, 0, 1), 1000, row(1), seg[1]) == ((50, 50 + B, 1), [4])
    node, nv, mx, sm, cand, vic = PR.preempt(alloc, bound, pods, 2)
    assert node.tolist() == [0, PR.NO_FIT, 0] and nv.tolist() == [1, 0, 0]
    assert mx.tolist() == [200, PR.NO_VICTIM_PRIO, PR.NO_VICTIM_PRIO] and sm.tolist() == [200 + B, 0, 0]
    assert cand.tolist() == [3, 0, 3] and vic.tolist() == [[1, -1], [-1, -1], [-1, -1]]
    # without node 0 the tie on the max priority goes to node 2 by the sum; vcap cuts the list, not the count
    node, nv, _, sm, cand, vic = PR.preempt(alloc, bound, pods, 1, lo=1)
    assert node.tolist() == [2, PR.NO_FIT, 2] and cand.tolist() == [2, 0, 2] and vic.tolist() == [[5], [-1], [-1]]
    node, nv, _, _, _, vic = PR.preempt(alloc, bound, pods, 1, lo=1, hi=2)
    assert node.tolist() == [1, PR.NO_FIT, 1] and nv.tolist() == [2, 0, 1] and vic.tolist() == [[2], [-1], [4]]


def test_merge_preempt_over_three_shards():
    from ksched.dist import merge_preempt, shard_range
    alloc, bound, pods = PR.gen(2, 211, 96)
    want = PR.preempt(alloc, bound, pods, 16)
    nofit, novictim, multi = PR.classes(want)
    assert nofit and novictim and multi
    shards = [PR.preempt(alloc, bound, pods, 16, *shard_range(211, r, 3)) for r in range(3)]
    got = merge_preempt(shards)
    PR.same(got[:6], want)
    lo = np.array([shard_range(211, r, 3)[0] for r in range(3)] + [211])
    assert np.array_equal(got[6], np.where(want[0] < 0, -1, np.searchsorted(lo, want[0], side="right") - 1))
    assert len({int(x) for x in got[6]} - {-1}) == 3  # every shard wins some pod
    # one shard merges into itself
    PR.same(merge_preempt([want])[:6], want)


def test_pod_from_kube_reads_priority():
    from ksched.host import Pod, pod_from_kube
    obj = {"metadata": {"name": "p"}, "spec": {"priority": 1000, "containers": []}}
    assert pod_from_kube(obj).priority == 1000
    obj["spec"]["priority"] = -5
    assert pod_from_kube(obj).priority == -5
    del obj["spec"]["priority"]
    assert pod_from_kube(obj).priority == 0 == Pod("q", []).priority
