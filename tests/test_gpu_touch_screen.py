"""The commit's touched-node column on the device (csrc/ksched_commit.h touch_stage, touch_need, touch_column, run in
isolation by ksched_selftest_touch_screen) against its numpy statement tests/touch_screen_ref.py, bit for bit, on
65,536 (pod, column) pairs of primitives_ref.screen_operands' families: the staged reciprocals (they are screen_y of
the device's own refined reciprocal, which ksched_selftest_score and ksched_selftest_screen return), the screen value,
the decision against thresholds at, one ulp around and near the value, and the column's key -- the oracle's score
where some pod of the wave needs it, the skip NaN otherwise.  Three launches."""
import ctypes as C

import numpy as np
import pytest

import primitives_ref as P
import touch_screen_ref as T

pytestmark = pytest.mark.gpu

N = 1 << 16
SKIP_BITS = 0x7FF8000000000BAD


def thresholds(v, ex, req, alloc):
    """per pair a threshold and an active flag; waves (64 consecutive pairs) of every kind: nobody active, everybody
    screened out, mixed"""
    rng = np.random.default_rng(151)
    n = v.size
    inf = np.float32(np.inf)
    thr = T.list_thr(ex + (rng.random(n) - 0.5) * 2e-4)           # a last key within 1e-4 of the pair's own
    k = n // 8
    thr[:k] = v[:k]                                               # exactly at the value: needed
    thr[k:2 * k] = np.nextafter(v[k:2 * k], inf)                  # one ulp above: skipped
    thr[2 * k:3 * k] = np.nextafter(v[2 * k:3 * k], -inf)
    thr[3 * k:3 * k + 512] = -inf                                 # an uncut list
    thr[3 * k + 512:3 * k + 1024] = inf
    thr[3 * k + 1024:3 * k + 1536] = np.nan
    active = (rng.random(n) < 0.85).astype(np.uint32)
    wave = np.arange(n) // 64
    late = np.arange(n) >= n // 2                                 # (the second half: the edges above stay as they are)
    active[late & (wave % 4 == 3)] = 0                            # a wave nobody may use the column in
    out = late & (wave % 4 == 2)                                  # a wave every screenable pair is screened out in
    thr[out] = inf
    active[out & np.isnan(v)] = 0
    return np.ascontiguousarray(thr, np.float32), np.ascontiguousarray(active)


@pytest.fixture(scope="module")
def run(gpu_available, oracle_mod):
    from ksched import Engine, _lib as L
    req, alloc = P.screen_operands(142, N)
    ex = P.oracle_scores(oracle_mod, req, alloc)
    lib, p = L.lib(), L.ptr
    with Engine() as e:
        sc = dict(score=np.empty((3, N)), upper=np.empty((2, N)), recip=np.empty((3, N)), flags=np.empty(N, np.int32))
        L.check(lib.ksched_selftest_score(e._ctx, N, p(req, C.c_int64), p(alloc, C.c_int64), p(sc["score"], C.c_double),
                                          p(sc["upper"], C.c_double), p(sc["recip"], C.c_double),
                                          p(sc["flags"], C.c_int32)), e._ctx, "selftest_score")
        sf, su = np.empty((13, N), np.float32), np.empty((8, N), np.uint32)
        L.check(lib.ksched_selftest_screen(e._ctx, N, p(req, C.c_int64), p(alloc, C.c_int64), p(sf, C.c_float),
                                           p(su, C.c_uint32)), e._ctx, "selftest_screen")
        y = np.where(alloc == 0, 0.0, sc["recip"])  # recip_or_zero, from the device's own recip
        ty = T.touch_stage(alloc, y)
        v = T.touch_value(req, alloc, ty)
        thr, active = thresholds(v, ex, req, alloc)
        f, u, key = np.empty((4, N), np.float32), np.empty((2, N), np.uint32), np.empty(N)
        L.check(lib.ksched_selftest_touch_screen(e._ctx, N, p(req, C.c_int64), p(alloc, C.c_int64), p(thr, C.c_float),
                                                 p(active, C.c_uint32), p(f, C.c_float), p(u, C.c_uint32),
                                                 p(key, C.c_double)), e._ctx, "selftest_touch_screen")
    return dict(req=req, alloc=alloc, ex=ex, ty=ty, v=v, thr=thr, active=active, f=f, u=u, key=key, screen_y=sf[6:9])


def test_staged_reciprocals(run):
    """touch_stage's floats are the statement's, and the device's own screen_y, bit for bit; NaN outside (0, 2^52)"""
    d = run
    for k, name in enumerate("cmp"):
        P._none_bad(P.same_f32(d["f"][k], d["ty"][k]), f"staged reciprocal {name}", d["alloc"], d["f"][k], d["ty"][k])
        P._none_bad(P.same_f32(d["f"][k], d["screen_y"][k]), f"staged reciprocal {name} against screen_y", d["alloc"])
    dom = (d["alloc"] > 0) & (d["alloc"] < T.P52)
    assert (np.isnan(d["f"][:3]) == ~dom).all() and (~dom).any()


def test_value_and_decision(run):
    d = run
    P._none_bad(P.same_f32(d["f"][3], d["v"]), "screen value", d["req"], d["alloc"], d["f"][3], d["v"])
    need = T.touch_need(d["v"], d["thr"], d["active"] != 0)
    P._none_bad((d["u"][0] != 0) == need, "needed", d["req"], d["alloc"], d["v"], d["thr"], d["active"])
    assert 0.1 < need.mean() < 0.8
    k = N // 8  # the edges: at the value needed, one ulp above it skipped
    act, fin = d["active"] != 0, ~np.isnan(d["v"])
    assert need[:k][act[:k]].all() and not need[k:2 * k][fin[k:2 * k]].any()
    assert need[(np.isnan(d["v"]) | np.isnan(d["thr"])) & act].all()  # an unscreenable state is always needed


def test_column_key(run, oracle_mod):
    """touch_column per wave: some pod needs it -> every lane's exact key, the oracle's score bits (-inf where the
    score is not positive); nobody -> the skip NaN"""
    d = run
    need = T.touch_need(d["v"], d["thr"], d["active"] != 0)
    any_ = np.repeat(need.reshape(-1, 64).any(axis=1), 64)
    P._none_bad((d["u"][1] != 0) == any_, "some pod of the wave needs the column", d["req"], d["alloc"])
    assert 0.5 < any_.mean() < 0.9
    with np.errstate(invalid="ignore"):
        exact = np.where(d["ex"] > 0, d["ex"], -np.inf)
    want = np.where(any_, P.bits64(exact), np.int64(SKIP_BITS))
    P._none_bad(P.bits64(d["key"]) == want, "column key", d["req"], d["alloc"], d["key"], exact)
