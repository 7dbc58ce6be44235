"""ksched_rank without a GPU: the host merge of the shards' ranked lists (ksched_rank_merge) against the oracle's
merge_topk, and the two compare-exchange steps ksched_rank.hip adds to wave_sort_desc<1> -- rank_merge_step, the
merge of two sorted 64-lists, and rank_insert_step, one candidate into a sorted list -- modelled lane for lane, as
tests/test_merge_network.py models the sort."""
import ctypes as C
import random

import numpy as np
import pytest

import rank_ref as RR


# ---- ksched_rank_merge == oracle.merge_topk ---------------------------------------------------------------------
def _call_merge(L, priority, nranks, m, k, cols):
    idx, score, reason, count, feas = cols
    oi = np.empty((m, k), np.int32); os_ = np.empty((m, k), np.float64); orr = np.empty((m, k), np.uint8)
    oc = np.empty(m, np.int32); of = np.empty(m, np.int32)
    rc = L.lib().ksched_rank_merge(priority, nranks, m, k, L.ptr(idx, C.c_int32), L.ptr(score, C.c_double),
                                   L.ptr(reason, C.c_uint8), L.ptr(count, C.c_int32), L.ptr(feas, C.c_int32),
                                   L.ptr(oi, C.c_int32), L.ptr(os_, C.c_double), L.ptr(orr, C.c_uint8),
                                   L.ptr(oc, C.c_int32), L.ptr(of, C.c_int32))
    return rc, (oi, os_, orr, oc, of)


@pytest.mark.parametrize("name", ["c3", "c2", "c5hc", "small93"])
def test_rank_merge_equals_oracle_merge(name, oracle_mod):
    from ksched import _lib as L
    from ksched.dist import merge_ranked, shard_range
    O = oracle_mod
    cl = RR.make(name)
    m = cl.n_pods
    for k in (1, 16, 64):
        for R in (1, 2, 3, 8):
            ranges = [shard_range(cl.n_nodes, r, R) for r in range(R)]
            parts = [RR.shard_recs(O, cl, k, lo, hi) for lo, hi in ranges]
            shards = [RR.columns(O, cl, recs, fc, k, lo=lo, hi=hi) for (recs, fc), (lo, hi) in zip(parts, ranges)]
            mrecs, mfc = O.merge_topk(k, R, m, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
            ref = RR.columns(O, cl, mrecs, mfc, k)
            # the shards as Engine.rank returns them: scores as doubles
            sh = [(s[0], s[1].view(np.float64), s[2], s[3], s[4]) for s in shards]
            RR.same(merge_ranked(cl.priority, sh), ref)
            if R == 3 and k == 16:  # the C call itself, NULL reason / feasible inputs and NULL outputs admitted
                cols = tuple(np.ascontiguousarray(np.stack([s[j] for s in sh])) for j in range(5))
                rc, got = _call_merge(L, cl.priority, R, m, k, (cols[0], cols[1], None, cols[3], None))
                assert rc == L.OK
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[3], ref[3])
                assert not got[2].any() and not got[4].any()


def test_rank_merge_arguments():
    from ksched import _lib as L
    m, k = 2, 4
    cols = (np.full((1, m, k), -1, np.int32), np.zeros((1, m, k)), np.zeros((1, m, k), np.uint8),
            np.zeros((1, m), np.int32), np.zeros((1, m), np.int32))
    assert _call_merge(L, 0, 1, m, k, cols)[0] == L.OK
    assert _call_merge(L, 0, 1, m, 0, cols)[0] == L.E_INVALID
    assert _call_merge(L, 0, 0, m, k, cols)[0] == L.E_INVALID
    big = tuple(np.zeros((1, m, 65), t) for t in (np.int32, np.float64, np.uint8)) + cols[3:]
    assert _call_merge(L, 0, 1, m, 65, big)[0] == L.E_INVALID
    assert _call_merge(L, 2, 1, m, k, cols)[0] == L.E_INVALID
    assert L.RANK_MAX == 64
    rc, got = _call_merge(L, 1, 1, m, k, cols)  # empty lists stay empty
    assert rc == L.OK and (got[0] == -1).all() and not got[3].any()


# ---- rank_merge_step, lane for lane ---------------------------------------------------------------------------------
EMPTY = (0, 0x7FFFFFFF)


def better(a, b):
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


def stage(v, m, hb):
    """sort_stage<M, HB>: lane l meets lane l ^ M; the lane with bit HB clear keeps the better pair."""
    p = [v[l ^ m] for l in range(64)]
    return [p[l] if (better(p[l], v[l]) != bool(l & hb)) else v[l] for l in range(64)]


def rank_merge_step(kept, cand):
    r = [cand[l ^ 63] for l in range(64)]  # xpartner<63>: the candidates reversed
    v = [r[l] if better(r[l], kept[l]) else kept[l] for l in range(64)]
    for d in (32, 16, 8, 4, 2, 1):  # the half-cleaners of a bitonic sequence
        v = stage(v, d, d)
    return v


KEY = lambda p: (-p[0], p[1])


def test_merge_step_zero_one_exhaustive():
    """All 65 x 65 zero-one inputs of two sorted 64-lists (a ones then zeros, b ones then zeros), the tie-break by
    index: within a code class the lists are sorted by index, and the two lists' indices interleave in three ways
    (kept's all lower, cand's all lower, alternating).  The output must be the best 64 of the 128, sorted."""
    splits = {"kept_low": (list(range(64)), list(range(64, 128))), "cand_low": (list(range(64, 128)), list(range(64))),
              "alternate": (list(range(0, 128, 2)), list(range(1, 128, 2)))}
    rng = random.Random(3)
    for a in range(65):
        for b in range(65):
            for nm, (ik, ic) in splits.items():
                def lst(ones, ids):
                    # ones first (code 2), then zeros (code 1): each class in index order
                    hi = sorted(rng.sample(ids, ones))
                    lo = sorted(set(ids) - set(hi))
                    return [(2, i) for i in hi] + [(1, i) for i in lo]
                kept, cand = lst(a, ik), lst(b, ic)
                got = rank_merge_step(kept, cand)
                assert got == sorted(kept + cand, key=KEY)[:64], (a, b, nm)


def test_merge_step_partial_lists_and_ties():
    """Lists with empty tails ((0, kNoIdx), equal among themselves), all-equal keys and few distinct keys."""
    rng = random.Random(5)
    for _ in range(2000):
        ids = rng.sample(range(10 ** 6), 128)
        kind = rng.choice(["random", "ties", "few"])
        codes = {"random": lambda: rng.randrange(1, 1 << 63), "ties": lambda: 7,
                 "few": lambda: rng.choice((3, 5, 9))}[kind]
        na, nb = rng.randrange(0, 65), rng.randrange(0, 65)
        kept = sorted([(codes(), i) for i in ids[:na]], key=KEY) + [EMPTY] * (64 - na)
        cand = sorted([(codes(), i) for i in ids[64:64 + nb]], key=KEY) + [EMPTY] * (64 - nb)
        got = rank_merge_step(kept, cand)
        assert got == sorted(kept + cand, key=KEY)[:64]


# ---- rank_insert_step, lane for lane ----------------------------------------------------------------------------
def rank_insert_step(kept, x):
    prev = [((1 << 64) - 1, 0)] + kept[:63]  # wave_shr:1; lane 0's missing neighbour is unbeatable
    out = []
    for l in range(64):
        b, pb = better(x, kept[l]), better(x, prev[l])
        out.append((prev[l] if pb else x) if b else kept[l])
    return out


def test_insert_step_zero_one_exhaustive():
    """Every sorted zero-one 64-list (a ones, b zeros, the rest empty) and a candidate of either code whose index is
    below, between or above the list's: the result is the best 64 of the 65, sorted."""
    for a in range(65):
        for b in range(65 - a):
            kept = [(2, 10 + 2 * i) for i in range(a)] + [(1, 10 + 2 * i) for i in range(b)] + [EMPTY] * (64 - a - b)
            for code in (1, 2):
                for xi in (0, 11, 10 + 2 * max(a, b) - 1, 1000):
                    got = rank_insert_step(kept, (code, xi))
                    assert got == sorted(kept + [(code, xi)], key=KEY)[:64], (a, b, code, xi)


def test_insert_steps_equal_a_merge():
    """The scan's use: up to 8 candidates chosen against the OLD bar, inserted in lane order -- one the rising bar has
    overtaken drops out -- give what the sort-and-merge path gives."""
    rng = random.Random(9)
    for _ in range(1500):
        ids = rng.sample(range(10 ** 6), 128)
        codes = rng.choice([lambda: rng.randrange(1, 1 << 63), lambda: rng.choice((3, 5, 9))])
        na = rng.randrange(0, 65)
        kept = sorted([(codes(), i) for i in ids[:na]], key=KEY) + [EMPTY] * (64 - na)
        cands = [(codes(), i) for i in ids[64:64 + rng.randrange(1, 9)]]
        cands = [c for c in cands if better(c, kept[63])]
        got = kept
        for c in cands:
            got = rank_insert_step(got, c)
        assert got == sorted(kept + cands, key=KEY)[:64]
        assert got == rank_merge_step(kept, sorted(cands, key=KEY) + [EMPTY] * (64 - len(cands)))


def test_rank_geometry_is_bounded():
    """The header's workspace claim, from the constants in ksched_rank.h restated here: spans * pods of a chunk never
    exceeds 2048 * 8 span lists of 1 KiB, every span has at least one row and no span is shorter than 256 rows."""
    def geometry(n, m, tile=8, span_min=1024, grid=2048, threads=256):
        tiles = max(1, -(-m // tile))
        s = max(1, min(grid // tiles, -(-n // span_min)))
        rows = max(threads, -(-(-(-n // s)) // threads) * threads)
        return max(1, -(-n // rows)), rows
    for n in (1, 63, 64, 65, 129, 1024, 1025, 20011, 100003, 2 ** 31 - 17):
        for m in (1, 7, 8, 9, 65, 300, 1024):
            spans, rows = geometry(n, m)
            assert spans * m <= 2048 * 8 and (spans - 1) * rows < n <= spans * rows
    assert geometry(100003, 3)[0] == 98 and geometry(100003, 1024)[0] == 16
