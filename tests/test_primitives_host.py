"""The checks of tests/test_gpu_primitives.py run on the CPU statements' own arrays (tests/primitives_ref.py), with
the oracle's score standing in for the device's: same operand generators, same seeds, same sizes.  This shows that
the reference alone meets every condition the GPU test asserts -- the 10 % near1 cap and near1's locality, the
at-least-half FAST53 coverage, every screen inequality, the record and threshold properties, and the wave checks on
the network model of tests/test_merge_network.py.  A failure here means a check is wrong, not the device."""
import numpy as np
import pytest

import primitives_ref as P

N_ORACLE = 1 << 16   # elements where the scalar oracle is the reference
N_WIDE = 1 << 18
WAVE_CASES = 4096    # per kind
LIST_SEQS = 1 << 14


@pytest.fixture(scope="module")
def score_set(oracle_mod):
    req, alloc = P.score_operands(101, N_ORACLE)
    return req, alloc, P.oracle_scores(oracle_mod, req, alloc)


@pytest.fixture(scope="module")
def upper_set(oracle_mod):
    req, alloc = P.upper_operands(102, N_ORACLE)
    return req, alloc, P.oracle_scores(oracle_mod, req, alloc)


@pytest.fixture(scope="module")
def screen_set(oracle_mod):
    req, alloc = P.screen_operands(103, N_ORACLE)
    return req, alloc, P.oracle_scores(oracle_mod, req, alloc)


def test_score_checks_hold_on_the_oracle(score_set):
    req, alloc, ex = score_set
    info = P.check_score(req, alloc, P.score_statement(req, alloc, ex), ex)
    assert info["fast53_share"] >= 0.5


def test_score_kats_are_the_oracles(oracle_mod):
    req, alloc, want = P.kat_operands()
    ex = P.oracle_scores(oracle_mod, req, alloc)
    assert (P.bits64(ex) == P.bits64(want)).all()
    assert P.fast53_ok(req, alloc).any()


def test_price_key_check_holds_on_numpy():
    price = P.price_operands(104, N_WIDE)
    P.check_price_key(price, -price.astype(np.float64) + 0.0)


def test_recip_check_holds_on_the_rounded_reciprocal():
    _, alloc = P.recip_operands(105, N_WIDE)
    assert np.abs(alloc).min() == 1 and np.abs(alloc).max() == 1 << 62
    with np.errstate(divide="ignore"):
        assert P.check_recip(alloc, 1.0 / alloc.astype(np.float64)) == 0


def test_upper_checks_hold_on_the_statement(upper_set):
    req, alloc, ex = upper_set
    info = P.check_upper(req, alloc, P.score_statement(req, alloc, ex), ex)
    assert 0.02 < info["near1_share"] <= 0.10


def test_near1_is_local_on_the_plain_cases(oracle_mod):
    """with test_score_bound._cases themselves (about half of the pairs flagged) near1 is set only within 2e-12 of a
    full resource, no exception"""
    req, alloc = P.score_operands(106, N_ORACLE)
    req[:, 0], alloc[:, 0] = (1, 1, 1), (3, 3, 3)
    ex = P.oracle_scores(oracle_mod, req, alloc)
    info = P.check_upper(req, alloc, P.score_statement(req, alloc, ex), ex, share_cap=1.0)
    assert 0.4 < info["near1_share"] < 0.65


def test_screen_identity_check_holds_on_the_statement():
    req, alloc = P.screen_operands(107, N_WIDE)
    info = P.check_screen_identity(req, alloc, P.screen_statement(req, alloc))
    assert info["ambiguous_share"] > 0.2 and info["nan_share"] > 0.1 and info["non_fitting_share"] > 0.1


def test_screen_soundness_checks_hold_on_the_statement(screen_set):
    req, alloc, ex = screen_set
    worst = P.check_screen_sound(req, alloc, P.screen_statement(req, alloc), ex)
    assert max(v for k, v in worst.items() if "non-fitting" not in k) < P.BOUND


def test_fma32_is_the_exact_fused_multiply_add():
    """screen_ref.fma32 rounds through long double; on the screen's operands that is the single rounding of the exact
    sum (the referee of check_screen_identity, in rational arithmetic)"""
    req, alloc = P.screen_operands(108, 4096)
    v, mx, amb, rf = P.R.screen_fast(*req, *alloc)
    idx = np.nonzero(~amb & rf)[0][:600]
    assert idx.size == 600
    for i in idx:
        c, m, p = (P.R.screen_req(req[k, i:i + 1])[0] * P.R.screen_recip(alloc[k, i:i + 1])[0] for k in range(3))
        assert P.screen_fast_poly_exact(c, m, p) == v[i], (i, c, m, p)


def test_record_checks_hold_on_the_statement():
    w, w2 = P.rec_operands()
    assert w.size > 3 * 0x4900
    P.check_rec_w(w, w2, P.rec_w_statement(w, w2))


def test_threshold_checks_hold_on_the_statement():
    L, rec = P.threshold_operands()
    P.check_threshold(L, rec, P.threshold_statement(L, rec))


@pytest.mark.parametrize("kind", P.KEY_KINDS)
def test_wave_checks_hold_on_the_network_model(kind):
    cs = P.wave_cases(200 + P.KEY_KINDS.index(kind), WAVE_CASES, kind)
    P.check_wave(cs, P.wave_statement(cs))


def test_list_check_holds_on_the_statement():
    ls = P.list_cases(300, LIST_SEQS)
    P.check_list(ls, P.list_statement(ls))


def test_slot_checks_hold_on_the_statement():
    sc = P.slot_cases(400, LIST_SEQS)
    P.check_slots(sc, P.slots_statement(sc))
