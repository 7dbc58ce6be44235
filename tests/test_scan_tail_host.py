"""The screened scan's tail without a GPU: the bound from class maxima as tests/diag/screen_sim_classes.py
simulates it (class_bound, the table DESIGN 5 quotes) -- the KC-th largest class maximum never exceeds the KC-th
largest key, and pairs_report counts the rows at or above it; and the pair lists' rank, thread for thread: the pair a thread scored
and holds against the pair it finds again, at the boundary between the two (704 pairs), equal to a stable sort.
(The pair groups that ranked in registers were backed out, DESIGN 5, and their lane-for-lane model with them.)
"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("screen_sim_classes", os.path.join(HERE, "diag", "screen_sim_classes.py"))
SIM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SIM)

NINF = -np.inf


# ---- the class bound -------------------------------------------------------------------------------------------
def _kth(K, kc):
    """KC-th largest key per (pod, workgroup) of K [pod, row, workgroup]; -inf with fewer rows."""
    if K.shape[1] < kc:
        return np.full((K.shape[0], K.shape[2]), NINF)
    return -np.sort(-K, axis=1)[:, kc - 1, :]


def _key_sets():
    rng = np.random.default_rng(7)
    pods, wgs = 5, 3
    out = {}
    for rows in (1, 3, 12, 47, 48, 49, 100, 431):
        out[f"random_{rows}"] = rng.random((pods, rows, wgs)) * 10
    out["all_tied"] = np.full((pods, 100, wgs), 3.25)
    few = np.full((pods, 100, wgs), NINF)
    few[:, [5, 40], :] = [[1.0], [2.0]]
    out["fewer_than_kc_finite"] = few
    holes = rng.random((pods, 100, wgs)) * 10
    holes[rng.random(holes.shape) < 0.7] = NINF
    out["minus_inf_rows"] = holes
    one = rng.random((pods, 480, wgs))
    one[:, 0:480:48, :] += 100.0  # rows 0, 48, 96, ...: wave 0, slot 0 -- one class holds the 10 best keys
    out["one_class_holds_the_best"] = one
    return out


@pytest.mark.parametrize("name", list(_key_sets()))
@pytest.mark.parametrize("kc", [4, 8])
@pytest.mark.parametrize("wmod", [12, 6, 3, 1])
def test_class_bound_is_a_lower_bound(name, kc, wmod):
    K = _key_sets()[name]
    L = SIM.class_bound(K, kc, 12, 4, wmod)
    kth = _kth(K, kc)
    assert (L <= kth).all(), f"{name}: a class bound above the KC-th largest key"
    if wmod == 12 and K.shape[1] <= 48:  # one row per class: the bound IS the KC-th largest key
        assert np.array_equal(L, kth)
    # rows at or above the bound: never fewer than min(KC, finite rows); and what the tool reports
    fin = np.isfinite(K)
    need = (K >= L[:, None, :]) & fin
    assert (need.sum(1) >= np.minimum(kc, fin.sum(1))).all()
    rep = SIM.pairs_report(K, L, 0.0)
    per_wg = need.sum(1).sum(0)
    assert f"mean {per_wg.mean():.0f} max {per_wg.max()}," in rep, rep
    assert f"pods over 48 pairs: {(need.sum(1) > 48).sum()}," in rep, rep


def test_one_class_bound_is_weak():
    """The adversarial case: the best keys in one class leave the bound at the other classes' level."""
    K = _key_sets()["one_class_holds_the_best"]
    assert (SIM.class_bound(K, 4, 12, 4, 12) < 100.0).all() and (_kth(K, 4) >= 100.0).all()


# ---- the pair lists' rank: the held pair against the search, thread for thread -------------------------------------
SW, RW = 12, 11  # score waves; the ranking waves (wave SW - 1 prefetches the next batch)


def _find_pod(pincl, ec):
    """The exact phase's 6-step search: how many pods' inclusive counts are <= ec."""
    p = 0
    for st in (32, 16, 8, 4, 2, 1):
        p += st if pincl[p + st - 1] <= ec else 0
    return p


def pair_lists_rank(cnt, rows, keys, kc):
    """score_role's pair lists for one batch and workgroup: cnt[p] pairs of pod p, rows[p][s] / keys[p][s] the s-th
    (reservation order).  Thread e scores pair e (pod-major) and keeps {pod, range, row, key}; after the barrier the
    ranking waves rank every pair among its pod's (key descending, row ascending), from the held values when all
    pairs are in flight at once (pT <= RW * 64; KC <= 4 kernels), else finding their pairs again.  Returns (slots, held)."""
    pincl = np.cumsum(cnt).tolist()
    pexcl = [a - c for a, c in zip(pincl, cnt)]
    pT = pincl[63]
    key_lds, held_regs, nel = {}, {}, [0] * 64
    for wave in range(SW):  # exact phase: e0 = wave * 64, stride SW * 64
        for e0 in range(wave * 64, pT, SW * 64):
            for lane in range(64):
                e = e0 + lane
                if e >= pT:
                    continue
                p = _find_pod(pincl, e)
                ex = pexcl[p]
                r, k = rows[p][e - ex], keys[p][e - ex]
                key_lds[e] = k
                nel[p] += k != NINF
                held_regs[(wave, lane)] = (p, ex, pincl[p], r, k)  # the thread's registers: its LAST pair
    held = kc <= 4 and pT <= RW * 64  # (the KC = 8 kernels always search: kMasks)
    slots = [[(NINF, None)] * kc for _ in range(64)]
    stored = set()
    for wave in range(RW):
        for e0 in range(wave * 64, pT, RW * 64):
            for lane in range(64):
                e = e0 + lane
                if e >= pT:
                    continue
                if held:
                    p, ex, end, r, k = held_regs[(wave, lane)]
                else:
                    p = _find_pod(pincl, e)
                    ex, end = pexcl[p], pincl[p]
                    k, r = key_lds[e], rows[p][e - ex]
                if k == NINF:
                    continue
                rank = sum(key_lds[e2] > k or (key_lds[e2] == k and rows[p][e2 - ex] < r) for e2 in range(ex, end))
                if rank < kc:
                    assert (p, rank) not in stored
                    stored.add((p, rank))
                    slots[p][rank] = (k, r)
    for p in range(64):  # wave 0 fills the slots past the pod's eligible keys
        for q in range(nel[p], kc):
            assert (p, q) not in stored
    return slots, held


def _batch(rng, total, variant):
    """64 pods' pair lists with `total` pairs in all, each pod at most 48."""
    cnt = np.zeros(64, dtype=int)
    for _ in range(total):
        free = np.nonzero(cnt < 48)[0]
        cnt[rng.choice(free)] += 1
    rows, keys = [], []
    for c in cnt:
        rows.append(rng.permutation(430)[:c].tolist())  # reservation order, not node order
        if variant == "ties":
            keys.append(rng.integers(0, 3, c).astype(float).tolist())
        elif variant == "all_tied":
            keys.append([1.5] * c)
        elif variant == "minus_inf":
            keys.append([NINF if rng.random() < 0.5 else float(rng.integers(0, 4)) for _ in range(c)])
        else:
            keys.append(rng.random(c).tolist())
    return cnt.tolist(), rows, keys


@pytest.mark.parametrize("total", [0, 1, 63, 64, 303, 703, 704, 705, 768, 769, 1024])
@pytest.mark.parametrize("kc", [4, 8])
def test_pair_rank_held_and_searched_agree_with_a_stable_sort(total, kc):
    rng = np.random.default_rng(1000 * kc + total)
    for variant in ("distinct", "ties", "all_tied", "minus_inf"):
        cnt, rows, keys = _batch(rng, total, variant)
        slots, held = pair_lists_rank(cnt, rows, keys, kc)
        assert held == (kc <= 4 and total <= 704)  # the boundary: 11 ranking waves of 64 lanes
        for p in range(64):
            live = sorted(((k, r) for k, r in zip(keys[p], rows[p]) if k != NINF), key=lambda x: (-x[0], x[1]))
            assert slots[p] == (live + [(NINF, None)] * kc)[:kc], (total, kc, variant, p)
