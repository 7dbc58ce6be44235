"""The seeded scan's device primitives (ksched_device.h screen_need, ksched_pipe.h bound_insert), run in isolation by
ksched_selftest_seed, element by element against their numpy statements in tests/seed_ref.py: screen values around L
at every distance from one f32 ulp to 1, NaN and infinite values, L = 0 ("everything passes"), every flag combination;
bound lists with ties, zeros and fewer than KC bounds.  One launch."""
import ctypes as C

import numpy as np
import pytest

import seed_ref as S
from screen_ref import EPS, F

pytestmark = pytest.mark.gpu


def operands(n=1 << 16):
    rng = np.random.default_rng(13)
    v = (rng.random(n) * 11).astype(np.float32)
    L = (v + F(1.0) + (rng.random(n).astype(np.float32) - F(0.5)) * F(2e-4)).astype(np.float32)  # within +- 1e-4 of v + 1
    k = n // 8
    # exactly at the boundary and one ulp to each side of it
    edge = (v[:k] + (F(1.0) + EPS)).astype(np.float32)
    L[:k] = edge
    L[k:2 * k] = np.nextafter(edge, F(np.inf))
    L[2 * k:3 * k] = np.nextafter(edge, F(-np.inf))
    L[3 * k:4 * k] = 0
    v[4 * k:4 * k + 64] = np.nan
    v[4 * k + 64:4 * k + 128] = np.inf
    v[4 * k + 128:4 * k + 192] = -np.inf
    L[5 * k:6 * k] = (rng.random(k) * 12).astype(np.float32)  # unrelated
    flags = rng.integers(0, 4, n).astype(np.uint32)
    x = (rng.random((6, n)) * 10 + 1).astype(np.float32).view(np.uint32)
    x[:, :k] = x[0, :k]                      # ties
    x[rng.random((6, n)) < 0.4] = 0          # "no bound": some elements end with fewer than four
    x[:, k:k + 64] = 0
    return v, L, flags, np.ascontiguousarray(x)


def test_screen_need_and_bound_insert(gpu_available):
    from ksched import Engine, _lib as Lb
    v, L, flags, x = operands()
    n = v.size
    out = np.empty((5, n), np.uint32)
    with Engine() as e:
        Lb.check(Lb.lib().ksched_selftest_seed(e._ctx, n, Lb.ptr(v, C.c_float), Lb.ptr(L, C.c_float),
                                                Lb.ptr(flags, C.c_uint32), Lb.ptr(x, C.c_uint32), Lb.ptr(out, C.c_uint32)),
                 e._ctx, "selftest_seed")
    want = S.screen_need(v, (flags & 1) != 0, (flags & 2) != 0, L)
    bad = np.nonzero((out[0] != 0) != want)[0]
    assert bad.size == 0, (bad[:5], v[bad[:5]], L[bad[:5]], flags[bad[:5]])
    assert want.any() and not want.all()
    lst = S.bound_insert_top(x)
    assert np.array_equal(out[1:], lst)
    assert np.array_equal(lst, -np.sort(-np.concatenate([x, np.zeros((4, n), np.uint32)]).astype(np.int64), axis=0)[:4])
