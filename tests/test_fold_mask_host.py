"""The screened commit's masked folds against their plain forms, as tests/fold_mask_ref.py states them, on the CPU: on
random rounds -- skipped columns (NaN in every lane), -inf keys, equal keys on different nodes, rounds that key nothing,
rounds with one keyed wave, predicate deltas on columns that are not keyed, columns without a guess -- the t* fold over
the marked waves and the confirm fold over the marked columns give what the folds over every wave and every column give:
tk / ti / ts, and rbk / rbi / rbs / rb2 in every lane and fcc in the lanes that are read again (lanes >= f: the pods
not yet confirmed).  The rows of unmarked waves hold garbage that would win, as own[] leaves them on the device, so a
wrong wave bit shows; and a column mask that drops a column with a predicate delta is caught."""
import numpy as np
import pytest

import fold_mask_ref as F

WAVES = 12
KEYS = np.array([0.25, 0.5, 0.5, 1.0, 2.0, 3.5, F.NEG_INF])
KINDS = ("mixed", "all_skipped", "single_wave", "d_unkeyed", "full", "short")


def make_round(rng, kind):
    """one round's inputs: window [c, cend), first failure f, guesses, key matrix S[lane][column], deltas D[column][lane]"""
    if kind == "short":
        c = int(rng.integers(40, 63)); cend = int(rng.integers(c + 1, 65))
    else:
        c = int(rng.integers(0, 8)); cend = 64 if rng.random() < 0.5 else int(rng.integers(c + 13, 65))
    f = int(rng.integers(c, cend + 1))
    p_key = {"mixed": 0.15, "all_skipped": 0.0, "single_wave": 0.0, "d_unkeyed": 0.05, "full": 0.9, "short": 0.3}[kind]
    p_d = {"mixed": 0.02, "all_skipped": 0.0, "single_wave": 0.01, "d_unkeyed": 0.3, "full": 0.05, "short": 0.1}[kind]
    nodes = rng.permutation(4096).astype(np.int32)
    gn = np.full(64, -2, np.int32)
    gs = np.full(64, -1, np.int32)
    keyed = np.zeros(64, bool)
    S = np.full((64, 64), np.nan)
    D = np.zeros((64, 64), np.int8)
    slot = 130
    for k in range(c, cend):
        r = rng.random()
        if r < 0.1:
            gn[k] = -1 if r < 0.05 else -2  # list exhausted / predicted no fit: no column
            continue
        gn[k] = nodes[k]
        gs[k] = slot; slot += 1
        keyed[k] = rng.random() < p_key
        if rng.random() < p_d:
            D[k] = rng.choice(np.array([-1, 0, 0, 1], np.int8), 64)
    if kind == "single_wave":  # every keyed column in one wave
        w = int(rng.integers(0, WAVES))
        for k in range(c, cend):
            keyed[k] = gn[k] >= 0 and F.column_wave(k, c, WAVES) == w and rng.random() < 0.7
    for k in range(c, cend):
        if keyed[k]:
            S[:, k] = rng.choice(KEYS, 64)
    lanes_set = rng.random(64) < 0.7
    rbk = np.where(lanes_set, rng.choice(KEYS[:-1], 64), F.NEG_INF)
    rbi = np.where(lanes_set, nodes[100:164], F.NO_IDX).astype(np.int32)
    rbs = np.where(lanes_set, rng.integers(0, 128, 64), -1).astype(np.int32)
    fcc = rng.integers(0, 50, 64).astype(np.int32)
    rb2 = np.where(rng.random(64) < 0.2, np.inf, rng.choice(KEYS[:-2], 64)).astype(np.float32)
    return dict(c=c, cend=cend, f=f, gn=gn, gs=gs, keyed=keyed, S=S, D=D, rbk=rbk, rbi=rbi, rbs=rbs, fcc=fcc, rb2=rb2)


def garbage_rows(pk, pi, ps, wmask):
    """the partial rows as the masked step 2 leaves them: the unmarked waves' rows are never written"""
    pk, pi, ps = pk.copy(), pi.copy(), ps.copy()
    for w in range(pk.shape[0]):
        if not (wmask >> w) & 1:
            pk[w] = 1e300; pi[w] = 0; ps[w] = 77
    return pk, pi, ps


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
def test_masked_folds_equal_plain(kind):
    rng = np.random.default_rng(KINDS.index(kind) + 7)
    seen = dict(none=0, some=0, skipped=0, visited=0, d_only=0)
    for _ in range(200):
        r = make_round(rng, kind)
        pk, pi, ps, wmask = F.step2(r["S"], r["gn"], r["gs"], r["keyed"], r["c"], r["cend"], WAVES)
        plain = F.tstar_fold(r["rbk"], r["rbi"], r["rbs"], pk, pi, ps)
        masked = F.tstar_fold(r["rbk"], r["rbi"], r["rbs"], *garbage_rows(pk, pi, ps, wmask), wmask)
        assert same(plain, masked)
        seen["none" if wmask == 0 else "some"] += 1
        cmask = F.column_mask(r["gn"], r["keyed"], r["D"], r["c"], r["cend"])
        for rb2 in (None, r["rb2"]):
            a = F.confirm_fold(r["rbk"], r["rbi"], r["rbs"], r["fcc"], rb2, r["S"], r["D"], r["gn"], r["gs"], r["c"], r["f"])
            b = F.confirm_fold(r["rbk"], r["rbi"], r["rbs"], r["fcc"], rb2, r["S"], r["D"], r["gn"], r["gs"], r["c"], r["f"], cmask)
            assert same(a[:3], b[:3])
            assert np.array_equal(a[3][r["f"]:], b[3][r["f"]:])  # fcc of the pods still to come
            if rb2 is not None:
                assert np.array_equal(a[4], b[4])
        seen["visited"] += b[5]
        seen["skipped"] += a[5] - b[5]
        seen["d_only"] += sum(1 for k in range(r["c"], r["f"]) if (cmask >> k) & 1 and not r["keyed"][k])
    if kind == "all_skipped":
        assert seen["some"] == 0 and seen["visited"] == 0 and seen["skipped"] > 0
    elif kind == "single_wave":
        assert seen["some"] > 0
    else:
        assert seen["some"] > 0 and seen["visited"] > 0 and seen["skipped"] > 0, seen
    if kind == "d_unkeyed":
        assert seen["d_only"] > 0  # columns the fold visits for their predicate delta alone


def test_single_wave_rounds_mark_one_wave():
    rng = np.random.default_rng(3)
    n = 0
    for _ in range(100):
        r = make_round(rng, "single_wave")
        wmask = F.step2(r["S"], r["gn"], r["gs"], r["keyed"], r["c"], r["cend"], WAVES)[3]
        assert wmask & (wmask - 1) == 0
        n += wmask != 0
    assert n > 0


def test_later_round_keys_nothing():
    """a batch's first round keys a column, its next round none: the partial rows still hold the first round's bests
    (stale, and better than anything confirmed), the second round's mask is empty and its fold reads none of them"""
    rng = np.random.default_rng(11)
    r1 = make_round(rng, "full")
    pk, pi, ps, wmask = F.step2(r1["S"], r1["gn"], r1["gs"], r1["keyed"], r1["c"], r1["cend"], WAVES)
    assert wmask != 0
    pk = np.where(pk == F.NEG_INF, 9.0, pk + 9.0)  # (every row a winner)
    r2 = make_round(rng, "all_skipped")
    _, _, _, wmask2 = F.step2(r2["S"], r2["gn"], r2["gs"], r2["keyed"], r2["c"], r2["cend"], WAVES)
    assert wmask2 == 0
    t = F.tstar_fold(r2["rbk"], r2["rbi"], r2["rbs"], pk, pi, ps, wmask2)
    assert same(t, (r2["rbk"], r2["rbi"], r2["rbs"]))
    assert not same(F.tstar_fold(r2["rbk"], r2["rbi"], r2["rbs"], pk, pi, ps, wmask), t)  # the stale mask would not do


def test_wrong_masks_are_caught():
    """the comparison sees a dropped column with a predicate delta, a dropped keyed column, a dropped keyed wave and
    a wave bit set for rows that were never written"""
    rng = np.random.default_rng(5)
    caught = dict(d=0, key=0, wave=0, extra=0)
    for _ in range(200):
        r = make_round(rng, "d_unkeyed" if rng.random() < 0.5 else "mixed")
        c, f = r["c"], r["f"]
        args = (r["rbk"], r["rbi"], r["rbs"], r["fcc"], r["rb2"], r["S"], r["D"], r["gn"], r["gs"], c, f)
        a = F.confirm_fold(*args)
        cmask = F.column_mask(r["gn"], r["keyed"], r["D"], c, r["cend"])
        for k in range(c, f):
            if not (cmask >> k) & 1:
                continue
            b = F.confirm_fold(*args, cmask & ~(1 << k))
            differs = not (same(a[:3], b[:3]) and np.array_equal(a[3][f:], b[3][f:]) and np.array_equal(a[4], b[4]))
            if (r["D"][k, f:] != 0).any():
                assert differs  # a delta of a pod still to come: always seen, in fcc
                caught["d"] += 1
            elif r["keyed"][k] and differs:
                caught["key"] += 1
        pk, pi, ps, wmask = F.step2(r["S"], r["gn"], r["gs"], r["keyed"], c, r["cend"], WAVES)
        plain = F.tstar_fold(r["rbk"], r["rbi"], r["rbs"], pk, pi, ps)
        g = garbage_rows(pk, pi, ps, wmask)
        for w in range(WAVES):
            t = F.tstar_fold(r["rbk"], r["rbi"], r["rbs"], *g, wmask ^ (1 << w))
            if (wmask >> w) & 1:
                caught["wave"] += not same(plain, t)
            else:
                assert not same(plain, t)  # garbage read
                caught["extra"] += 1
    assert all(v > 0 for v in caught.values()), caught


def test_better_is_the_commits():
    k = np.array([1.0, 1.0, 2.0, F.NEG_INF, np.nan, 1.0])
    i = np.array([3, 5, 9, 1, 1, 4], np.int32)
    assert F.better(k, i, np.float64(1.0), np.int32(4)).tolist() == [True, False, True, False, False, False]
    assert not F.better(np.float64(1.0), 1, np.float64(np.nan), 2)  # nothing beats NaN either: it is never a holder
    x = np.array([1.0 + 2.0 ** -30, 0.5, np.nan])
    assert (F.f32_ru(x)[:2].astype(np.float64) >= x[:2]).all() and np.isnan(F.f32_ru(x)[2])
    assert F.f32_ru(x)[0] == np.nextafter(np.float32(1.0), np.float32(2.0))
