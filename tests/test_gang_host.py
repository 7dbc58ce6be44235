"""ksched_schedule_gangs without a GPU: the CPU restatement (gang_ref) on the worked example of include/ksched.h's
rules, the entry point's argument check, and ksched.host.group_gangs."""
import ctypes as C

import numpy as np
import pytest

import gang_ref as GR


def test_worked_example_reference(oracle_mod):
    cl, off = GR.worked_example()
    idx, score, feas, placed, state, info = GR.schedule_gangs(oracle_mod, cl, off)
    A, B = 0, 1
    assert idx.tolist() == [A, B, GR.GANG_REJECTED, -1, A]
    assert placed.tolist() == [2, 0, 1]
    assert state[0].tolist() == [0, 400]
    assert feas.tolist() == [2, 1, 2, 0, 2]
    assert score.tolist() == [float(np.float32(0.1)), 0.5, 0.0, 0.0, float(np.float32(0.1))]
    assert info == dict(rejected=1, rollbacks=1, partial=0, accepted_after_reject=1)
    # without the rollback p2 keeps A's 300 and p4 lands on B
    plain = oracle_mod.schedule(cl)
    assert plain[0].tolist() == [A, B, A, -1, B]
    # with a minimum of one member the second gang is accepted with p2 alone, and p4 lands on B again
    idx1, _, _, placed1, state1, info1 = GR.schedule_gangs(oracle_mod, cl, off, np.array([2, 1, 1], np.int32))
    assert idx1.tolist() == [A, B, A, -1, B] and placed1.tolist() == [2, 1, 1] and state1[0].tolist() == [100, 0]
    assert info1 == dict(rejected=0, rollbacks=0, partial=1, accepted_after_reject=0)


def test_size_one_gangs_are_the_plain_schedule(oracle_mod):
    from ksched import cluster
    cl = cluster.random_small(7, 64, 256, domain=cluster.DOMAIN_FEASIBLE)
    want = oracle_mod.schedule(cl)
    got = GR.schedule_gangs(oracle_mod, cl, np.arange(cl.n_pods + 1))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert np.array_equal(got[2], want[2]) and all(np.array_equal(a, b) for a, b in zip(got[4], want[3]))
    assert np.array_equal(got[3], (want[0] >= 0).astype(np.int32))


def test_null_context_is_invalid():
    from ksched import _lib as L
    assert L.GANG_REJECTED == GR.GANG_REJECTED == -3 and L.GANG_MAX == 1024
    off = np.array([0], np.int64)
    r = L.lib().ksched_schedule_gangs(None, 0, None, None, None, None, 0, L.ptr(off, C.c_int64), None, None, None, None,
                                      None)
    assert r == L.E_INVALID


def _pod(name, group=None, need=None):
    from ksched.host import GROUP_MIN_ANNOTATION, GROUP_NAME_ANNOTATION, Container, Pod
    ann = {}
    if group is not None:
        ann[GROUP_NAME_ANNOTATION] = group
    if need is not None:
        ann[GROUP_MIN_ANNOTATION] = str(need)
    return Pod(name=name, containers=[Container()], annotations=ann)


def test_group_gangs_interleaved_members():
    from ksched.host import group_gangs
    pods = [_pod("a0", "a"), _pod("b0", "b"), _pod("x"), _pod("a1", "a"), _pod("b1", "b"), _pod("y"), _pod("a2", "a")]
    out, off, need = group_gangs(pods)
    # a gang sits where its first member was; members keep their order; plain pods are gangs of one
    assert [p.name for p in out] == ["a0", "a1", "a2", "b0", "b1", "x", "y"]
    assert off.tolist() == [0, 3, 5, 6, 7] and off.dtype == np.int64
    assert need.tolist() == [3, 2, 1, 1] and need.dtype == np.int32


def test_group_gangs_no_annotations_and_empty():
    from ksched.host import group_gangs
    pods = [_pod(f"p{i}") for i in range(4)]
    out, off, need = group_gangs(pods)
    assert out == pods and off.tolist() == [0, 1, 2, 3, 4] and need.tolist() == [1, 1, 1, 1]
    out, off, need = group_gangs([])
    assert out == [] and off.tolist() == [0] and need.tolist() == []


def test_group_gangs_min_member():
    from ksched.host import group_gangs
    pods = [_pod("a0", "a"), _pod("b0", "b", 1), _pod("a1", "a", 2), _pod("a2", "a"), _pod("b1", "b", 1)]
    _, off, need = group_gangs(pods)
    assert off.tolist() == [0, 3, 5] and need.tolist() == [2, 1]


@pytest.mark.parametrize("need", [4, 0, -1, "many"])
def test_group_gangs_bad_min_member(need):
    from ksched.host import group_gangs
    with pytest.raises(ValueError):
        group_gangs([_pod("a0", "a", need), _pod("a1", "a"), _pod("a2", "a")])


def test_group_gangs_members_disagree():
    from ksched.host import group_gangs
    with pytest.raises(ValueError):
        group_gangs([_pod("a0", "a", 1), _pod("a1", "a", 2)])
