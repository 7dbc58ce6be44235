"""The commit's touched-node column screen as tests/touch_screen_ref.py states it, on the CPU: the staged reciprocals
are screen_y's, the value is screen_pair's, the value is NaN or within screen_pair's documented bounds of the oracle's
score (so the lists' threshold RN_f32(last key - 5e-5) stays sound: a skipped pair keys below the list's last entry),
and an unscreenable state is always needed.  Operands: primitives_ref.screen_operands' families."""
import numpy as np
import pytest

import primitives_ref as P
import screen_ref as R
import touch_screen_ref as T

N = 1 << 16


@pytest.fixture(scope="module")
def pairs(oracle_mod):
    req, alloc = P.screen_operands(141, N)
    ty = T.touch_stage(alloc, T.recip64(alloc))
    return req, alloc, ty, T.touch_value(req, alloc, ty), P.oracle_scores(oracle_mod, req, alloc)


def test_staged_reciprocal_is_screen_y(pairs):
    """RN_f32 of the refined f64 reciprocal inside screen_recip's domain, NaN outside it: (float)(1.0 / a), bit for bit"""
    req, alloc, ty, v, ex = pairs
    want = np.stack([R.screen_recip(alloc[k]) for k in range(3)])
    assert P.same_f32(ty, want).all()
    dom = (alloc > 0) & (alloc < T.P52)
    assert (np.isnan(ty) == ~dom).all() and dom.any() and (~dom).any()
    assert (P.bits32(ty[dom]) == P.bits32((1.0 / alloc[dom].astype(np.float64)).astype(np.float32))).all()


def test_value_is_screen_pairs(pairs):
    """the operation-by-operation statement equals screen_ref.screen_pair bit for bit, NaN in the same places"""
    req, alloc, ty, v, ex = pairs
    want, _ = R.screen_pair(*req, *alloc)
    assert P.same_f32(v, want).all()
    assert np.isnan(v).mean() > 0.1 and (~np.isnan(v)).mean() > 0.5


def test_value_is_nan_or_within_the_bounds(pairs):
    """screen_pair's documented bounds (ksched_device.h): every resource fitting with room to spare, the polynomial
    within 1.3e-5 of the score; some request over its allocatable, the non-fitting form within 2e-6.  With a resource
    exactly full the reference drops the balanced part, and the polynomial is the documented upper bound of the score:
    the one direction the screen relies on."""
    req, alloc, ty, v, ex = pairs
    fin = ~np.isnan(v)
    assert not np.isinf(v).any()
    fit = (alloc >= req).all(axis=0)
    full = (alloc == req).any(axis=0)
    err = v.astype(np.float64) - ex
    poly, nf, up = fin & fit & ~full, fin & ~fit, fin & fit & full
    worst = float(np.abs(err[poly]).max()), float(np.abs(err[nf]).max()), float(-err[up].min())
    print(f"touch screen: worst error {worst[0]:.3g} (fitting, bound {T.BOUND}), {worst[1]:.3g} (non-fitting, "
          f"{T.BOUND_NF}), score above the value by at most {worst[2]:.3g} with a full resource")
    assert poly.sum() > N // 8 and nf.sum() > N // 16 and up.sum() > 100
    assert worst[0] < T.BOUND and worst[1] < T.BOUND_NF and worst[2] < T.BOUND


@pytest.mark.parametrize("gap", [0.0, 1e-12, 1e-7, 1e-6, 1e-5, 3e-5, 4.9e-5, 6e-5, 1e-4, 1e-2, 1.0])
def test_threshold_stays_sound(pairs, gap):
    """a cut list whose last entry keys `gap` below (or at) the pair's exact key: the pair could enter the list, so
    it must be needed -- thr = RN_f32(last key - 5e-5) never skips it"""
    req, alloc, ty, v, ex = pairs
    el = ex > 0
    need = T.touch_need(v, T.list_thr(ex - gap), True)
    P._none_bad(~el | need, f"skipped at or above the last key (gap {gap})", req, alloc, v, ex)


def test_skips_happen_and_inactive_pods_never_need(pairs):
    """the other direction is not a proof obligation, but the screen is only worth its cost if it skips: a last key
    1e-4 above the pair's key skips every screenable pair (but one with a resource exactly full, whose value is only
    an upper bound)"""
    req, alloc, ty, v, ex = pairs
    need = T.touch_need(v, T.list_thr(ex + 1e-4), True)
    full = ((alloc == req) & (alloc >= req).all(axis=0)).any(axis=0)
    assert (need == np.isnan(v))[~full].all() and (~need).mean() > 0.5
    assert not T.touch_need(v, T.list_thr(ex - 1.0), False).any()
    assert T.touch_need(v, F_NEG_INF, True).all()  # an uncut list's threshold, and KSCHED_NO_TOUCH_SCREEN


F_NEG_INF = np.float32(-np.inf)


def test_unscreenable_state_is_always_needed(pairs):
    """a <= 0 or a >= 2^52 in any resource: whatever the threshold, +inf included"""
    req, alloc, ty, v, ex = pairs
    bad = ((alloc <= 0) | (alloc >= T.P52)).any(axis=0)
    assert bad.sum() > N // 16
    assert np.isnan(v[bad]).all()
    for thr in (np.float32(np.inf), np.float32(10.0), np.float32(0.0), F_NEG_INF):
        assert T.touch_need(v[bad], thr, True).all()
    # and an unscreenable request (negative or >= 2^52) likewise
    badr = ((req < 0) | (req >= T.P52)).any(axis=0)
    assert badr.sum() > 100 and T.touch_need(v[badr], np.float32(np.inf), True).all()
