"""The speculative commit's guess step (ksched_commit.h, step 1), stated in numpy and compared with the statement it
must equal -- no GPU.

Guess step: lane = pod; a pod's proposal is its lowest active list entry whose table position no earlier pod of the
window proposes.  The kernel iterates to a fixpoint over own[] (lowest proposing pod per table position) and probes in
two tiers: the lane's two lowest active entries first, and all K entries, for the whole wave, only in an iteration
in which some active lane found both taken and has further active entries.  Asserted here: every iteration of the
two-tier form proposes what the full scan proposes, and the fixpoint is the sequential greedy guess order.

This file states the loop in numpy and runs none of the HIP code: the kernel's LDS gathers (inline assembly) are
exercised by the GPU tests only (tests/test_gpu_guess_fixpoint.py and the parity suites)."""
import numpy as np
import pytest

H = 2048          # table positions (the last one stands for "no entry": always taken)
INVALID = H - 1


# ---- the guess step ---------------------------------------------------------------------------------------------------
def greedy(hp, am, c, cend):
    """sequential guess order: pod by pod, the first active entry no earlier pod of the window took"""
    taken, out = set(), np.full(64, -1)
    for i in range(c, cend):
        for q in range(hp.shape[0]):
            if (am[i] >> q) & 1 and int(hp[q, i]) not in taken:
                out[i] = q
                taken.add(int(hp[q, i]))
                break
    return out


def full_scan(hp, am, own, lane):
    for q in range(hp.shape[0]):
        if (am[lane] >> q) & 1 and own[hp[q, lane]] >= lane:
            return q
    return -1


def fixpoint(hp, am, c, cend, two_tier):
    """the kernel's loop.  Returns (proposals, iterations, iterations that took the full scan)"""
    K = hp.shape[0]
    act = np.array([c <= j < cend and am[j] != 0 for j in range(64)])
    own = np.full(H, 64)
    pq = np.full(64, -1)
    iters = nfull = 0
    while True:
        iters += 1
        nq = np.full(64, -1)
        need = False
        for j in range(64):
            a = int(am[j])
            qs = [q for q in range(K) if (a >> q) & 1]
            if two_tier:
                for q in qs[:2]:
                    if own[hp[q, j]] >= j:
                        nq[j] = q
                        break
                need = need or (nq[j] < 0 and len(qs) > 2)
            else:
                nq[j] = full_scan(hp, am, own, j)
        if two_tier and need:  # uniform: every lane scans all K entries
            nfull += 1
            for j in range(64):
                nq[j] = full_scan(hp, am, own, j)
        if two_tier:  # either tier: the lowest active entry whose own[] >= lane
            assert all(nq[j] == full_scan(hp, am, own, j) for j in range(64))
        changed = bool(np.any(act & (nq != pq)))
        for j in range(64):
            if act[j] and pq[j] >= 0:
                own[hp[pq[j], j]] = 64
        pq = nq
        if not changed and iters > 1:
            break
        for j in range(64):
            if act[j] and pq[j] >= 0:
                own[hp[pq[j], j]] = min(own[hp[pq[j], j]], j)
        assert iters <= (cend - c) + 2
    return np.where(act, pq, -1), iters, nfull


def lists(kind, K, rng):
    """hp [K][64] table positions (distinct within a pod's list), am [64] active masks (am = 0: the pod is not active)"""
    hp = np.full((K, 64), INVALID)
    am = np.zeros(64, np.int64)
    if kind == "random":  # a small pool (K + 4 positions), so that pods share entries; some confirmed-taken, some short
        for j in range(64):
            n = int(rng.integers(0, K + 1))
            hp[:n, j] = rng.choice(K + 4, size=n, replace=False)
            am[j] = sum(1 << q for q in range(n) if rng.random() < 0.8)
        am[rng.integers(0, 64, size=6)] = 0
    elif kind == "same":  # one list for all 64 pods: pods 2.. take the full scan, pods >= K exhaust it
        hp[:, :] = np.arange(100, 100 + K)[:, None]
        am[:] = (1 << K) - 1
    elif kind == "two_taken":  # every list starts with the two entries pods 0 and 1 take
        for j in range(64):
            rest = rng.choice(np.arange(10, 10 + 2 * K), size=K - 2, replace=False)
            hp[:, j] = np.concatenate([[3, 4] if j % 2 == 0 else [4, 3], rest])
        am[:] = (1 << K) - 1
        am[5] &= ~1  # a pod whose first entry is confirmed-taken already
    return hp, am


@pytest.mark.parametrize("K", [4, 8, 16])
@pytest.mark.parametrize("kind", ["random", "same", "two_taken"])
def test_two_tier_fixpoint_is_the_greedy_order(kind, K):
    rng = np.random.default_rng([K, len(kind)])
    full_scans = max_iters = 0
    for rep in range(3 if kind == "random" else 1):
        hp, am = lists(kind, K, rng)
        for c, W in ((0, 64), (0, 1), (5, 1), (9, 4), (60, 4), (0, 4), (17, 64)):
            cend = min(c + W, 64)
            want = greedy(hp, am, c, cend)
            got, iters, nfull = fixpoint(hp, am, c, cend, True)
            ref, riters, _ = fixpoint(hp, am, c, cend, False)
            assert np.array_equal(got, want), (kind, K, c, cend)
            assert np.array_equal(ref, want) and iters == riters, (kind, K, c, cend)
            full_scans += nfull
            max_iters = max(max_iters, iters)
            if kind == "same" and W == 64 and c == 0:
                assert nfull > 0 and (got[K:] == -1).all() and (got[:K] == np.arange(K)).all()
    # on the reference alone: the cases reach the fallback and fixpoints of more than two iterations
    assert max_iters > 2, (kind, K)
    assert full_scans > 0, (kind, K)


def test_single_pod_window_never_scans():
    hp, am = lists("same", 16, np.random.default_rng(1))
    got, iters, nfull = fixpoint(hp, am, 7, 8, True)
    assert got[7] == 0 and iters == 2 and nfull == 0
