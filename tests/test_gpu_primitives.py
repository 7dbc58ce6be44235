"""The device's own score, screen, record and wave primitives (csrc/ksched_device.h, ksched_merge.h, screen_y of
ksched_commit.h), run in isolation by the library's self-test unit (csrc/ksched_selftest.hip, ksched_selftest_* in
include/ksched.h) on arrays of adversarial operands, against the committed CPU statements (tests/screen_ref.py), the
oracle's score and a plain sort.  The checks are those of tests/primitives_ref.py, which tests/test_primitives_host.py
runs on the CPU statements alone.  One or two launches per test.

This proves the source semantics of the primitives under the library's compile flags; it does not prove the
instruction stream inside the kernels that inline them (the parity tests cover their results)."""
import ctypes as C

import numpy as np
import pytest

import primitives_ref as P

pytestmark = pytest.mark.gpu

N_ORACLE = 1 << 16   # elements where the scalar oracle is the reference
N_WIDE = 1 << 18
WAVE_CASES = 4096    # per kind
LIST_SEQS = 1 << 14


@pytest.fixture(scope="module")
def dev(gpu_available):
    from ksched import Engine
    with Engine() as e:
        yield Device(e._ctx)


class Device:
    """the self-test entry points on numpy arrays"""

    def __init__(self, ctx):
        from ksched import _lib as L
        self.L, self.lib, self.ctx = L, L.lib(), ctx

    def _ok(self, rc, what):
        self.L.check(rc, self.ctx, what)

    def score(self, req, alloc):
        n = req.shape[1]
        out = dict(score=np.empty((3, n)), upper=np.empty((2, n)), recip=np.empty((3, n)), flags=np.empty(n, np.int32))
        p = self.L.ptr
        self._ok(self.lib.ksched_selftest_score(self.ctx, n, p(req, C.c_int64), p(alloc, C.c_int64),
                                                p(out["score"], C.c_double), p(out["upper"], C.c_double),
                                                p(out["recip"], C.c_double), p(out["flags"], C.c_int32)), "selftest_score")
        return out

    def price_key(self, price):
        key = np.empty(price.size)
        self._ok(self.lib.ksched_selftest_price_key(self.ctx, price.size, self.L.ptr(price, C.c_float),
                                                    self.L.ptr(key, C.c_double)), "selftest_price_key")
        return key

    def screen(self, req, alloc):
        n = req.shape[1]
        out = dict(f=np.empty((13, n), np.float32), u=np.empty((8, n), np.uint32))
        p = self.L.ptr
        self._ok(self.lib.ksched_selftest_screen(self.ctx, n, p(req, C.c_int64), p(alloc, C.c_int64),
                                                 p(out["f"], C.c_float), p(out["u"], C.c_uint32)), "selftest_screen")
        return out

    def rec_w(self, w, w2):
        out = np.empty((4, w.size), np.uint32)
        p = self.L.ptr
        self._ok(self.lib.ksched_selftest_rec_w(self.ctx, w.size, p(w, C.c_float), p(w2, C.c_float),
                                                p(out, C.c_uint32)), "selftest_rec_w")
        return out

    def threshold(self, L, rec):
        out = np.empty((4, L.size), np.int32)
        p = self.L.ptr
        self._ok(self.lib.ksched_selftest_threshold(self.ctx, L.size, p(L, C.c_float), p(rec, C.c_uint32),
                                                    p(out, C.c_int32)), "selftest_threshold")
        return out

    def wave(self, cs):
        nl = cs["ncases"] * 64
        out = dict(u=np.empty((12, nl), np.uint64), v=np.empty((13, nl), np.int32))
        p = self.L.ptr
        self._ok(self.lib.ksched_selftest_wave(self.ctx, cs["ncases"], p(cs["sort_code"], C.c_uint64),
                                               p(cs["sort_idx"], C.c_int32), p(cs["key"], C.c_double),
                                               p(cs["idx"], C.c_int32), p(cs["aux"], C.c_int32), p(cs["cut"], C.c_int32),
                                               p(cs["nv"], C.c_int32), p(out["u"], C.c_uint64), p(out["v"], C.c_int32)),
                 "selftest_wave")
        return out

    def lists(self, ls):
        out = dict(key=np.empty((30, ls["n"])), idx=np.empty((30, ls["n"]), np.int32))
        p = self.L.ptr
        self._ok(self.lib.ksched_selftest_list(self.ctx, ls["n"], P.LIST_STEPS, p(ls["key"], C.c_double),
                                               p(ls["idx"], C.c_int32), p(out["key"], C.c_double),
                                               p(out["idx"], C.c_int32)), "selftest_list")
        return out

    def slots(self, sc):
        out = np.empty((60, sc["n"]), np.uint32)
        self._ok(self.lib.ksched_selftest_slots(self.ctx, sc["n"], P.SLOT_STEPS, self.L.ptr(sc["x"], C.c_uint32),
                                                self.L.ptr(out, C.c_uint32)), "selftest_slots")
        return out


def _contig(*arrays):
    for a in arrays:
        assert a.flags["C_CONTIGUOUS"]


# ---- score ----------------------------------------------------------------------------------------------------------
def test_score_forms_carry_the_oracles_bits(dev, oracle_mod):
    """resource_score and resource_score_fast<false> on every element, <true> under its precondition; eligibility"""
    req, alloc = P.score_operands(101, N_ORACLE)
    _contig(req, alloc)
    ex = P.oracle_scores(oracle_mod, req, alloc)
    info = P.check_score(req, alloc, dev.score(req, alloc), ex)
    print(f"score: FAST53 precondition holds on {info['fast53_share']:.1%} of {N_ORACLE} elements")


def test_score_kats_on_the_device(dev):
    """every entry of tests/golden/score_kats.json gives its score_hex, in all three forms where FAST53 may run"""
    req, alloc, want = P.kat_operands()
    out = dev.score(req, alloc)
    pre = P.fast53_ok(req, alloc)
    assert (P.bits64(out["score"][0]) == P.bits64(want)).all()
    assert (P.bits64(out["score"][1]) == P.bits64(want)).all()
    assert (P.bits64(out["score"][2])[pre] == P.bits64(want)[pre]).all() and pre.any()


def test_price_key_bits(dev):
    price = P.price_operands(104, N_WIDE)
    P.check_price_key(price, dev.price_key(price))


def test_recip_within_one_ulp(dev):
    """recip(af) against the correctly rounded 1 / af for integer-valued |a| in 1 .. 2^62 and for 3.0; prints the
    worst distance"""
    req, alloc = P.recip_operands(105, N_WIDE)
    out = dev.score(req, alloc)
    assert alloc[0, 0] == 3
    P.check_recip(alloc, out["recip"])


def test_upper_bound_with_the_device_values(dev, oracle_mod):
    req, alloc = P.upper_operands(102, N_ORACLE)
    ex = P.oracle_scores(oracle_mod, req, alloc)
    info = P.check_upper(req, alloc, dev.score(req, alloc), ex)
    print(f"upper: near1 on {info['near1_share']:.1%} of the pairs; worst upper - score outside it {info['worst_slack']:.3e}")


# ---- screen ---------------------------------------------------------------------------------------------------------
def test_screen_device_equals_statement(dev):
    req, alloc = P.screen_operands(107, N_WIDE)
    info = P.check_screen_identity(req, alloc, dev.screen(req, alloc))
    assert info["ambiguous_share"] > 0.2 and info["nan_share"] > 0.1 and info["non_fitting_share"] > 0.1


def test_screen_device_is_sound(dev, oracle_mod):
    """the device's screen values through the inequalities of tests/test_screen_bound.py, against the oracle's score;
    prints the worst error of each form"""
    req, alloc = P.screen_operands(103, N_ORACLE)
    ex = P.oracle_scores(oracle_mod, req, alloc)
    P.check_screen_sound(req, alloc, dev.screen(req, alloc), ex)


def test_records_round_down(dev):
    """every f16 pattern of the two record forms with its f32 neighbours: screen_rec_w rounds down and both halves of
    the packed round-toward-zero conversion pass 1 uses are that record"""
    w, w2 = P.rec_operands()
    P.check_rec_w(w, w2, dev.rec_w(w, w2))


def test_thresholds_equal_statement_and_are_a_superset(dev):
    L, rec = P.threshold_operands()
    P.check_threshold(L, rec, dev.threshold(L, rec))


# ---- wave -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KEY_KINDS)
def test_wave_primitives(dev, kind):
    """wave_sort_desc<1..32>, wave_rank, both arg-bests, the max / sum / min / or reductions, key_code and list_thr_bits
    on 4096 cases of one kind against a plain sort"""
    cs = P.wave_cases(200 + P.KEY_KINDS.index(kind), WAVE_CASES, kind)
    P.check_wave(cs, dev.wave(cs))


def test_list_insert_ordered(dev):
    ls = P.list_cases(300, LIST_SEQS)
    P.check_list(ls, dev.lists(ls))


def test_score_role_slot_helpers(dev):
    """bound_slots in both of its forms, sort_desc_u32 and topk_merge_u32 (ksched_pipe.h), KC = 4 and 8"""
    sc = P.slot_cases(400, LIST_SEQS)
    P.check_slots(sc, dev.slots(sc))
