"""The numpy statement of the commit's touched-node column screen (k8s-scheduler_amd/csrc/ksched_commit.h touch_stage,
touch_need), bit for bit: tests/test_touch_screen_host.py proves it sound against the oracle's score,
tests/test_gpu_touch_screen.py compares the device's own results (ksched_selftest_touch_screen) with it.

A column is a node state n[3] every pod of a batch is keyed against.  The lane that stages the column computes its
three f32 reciprocals once (touch_stage); every pod then takes its f32 screen value from them and needs the column's
exact key unless the value lies below its list's threshold thr = RN_f32(last key - 5e-5) (list_thr).  numpy's f32
arithmetic is IEEE round-to-nearest like the device's, which is built with -ffp-contract=off."""
import numpy as np

F = np.float32
P52 = 1 << 52
BOUND = 1.3e-5      # screen_pair's documented error, every resource fitting (the polynomial)
BOUND_NF = 2e-6     # ... some request over its allocatable (the non-fitting form)
THR_MARGIN = 5e-5   # list_thr_bits: thr = RN_f32(last key - 5e-5)


def recip64(a):
    """the refined f64 reciprocal the commit stages beside a state (recip_or_zero): 0 for a zero state.  The device's
    value comes from ksched_selftest_score; on the host the correctly rounded 1 / a stands for it."""
    a = np.asarray(a, np.int64)
    with np.errstate(divide="ignore"):
        return np.where(a == 0, 0.0, 1.0 / a.astype(np.float64))


def touch_stage(n, y):
    """screen_y per resource: RN_f32 of the f64 reciprocal y for 0 < n < 2^52, NaN otherwise ([3][k] each)"""
    n = np.asarray(n, np.int64)
    with np.errstate(all="ignore"):
        out = np.asarray(y, np.float64).astype(np.float32)
    out[(n <= 0) | (n >= P52)] = np.nan
    return out


def screen_req(r):
    """a request in f32; NaN when negative or >= 2^52"""
    r = np.asarray(r, np.int64)
    out = r.astype(np.float32)
    out[(r < 0) | (r >= P52)] = np.nan
    return out


def touch_value(req, n, ty):
    """the f32 screen value of pods req[3][k] against columns n[3][k] with staged reciprocals ty[3][k], one f32
    operation per line as the device rounds them"""
    req, n = np.asarray(req, np.int64), np.asarray(n, np.int64)
    q = screen_req(req)
    ok = n >= req
    five3, five9, one, zero = F(5.0) / F(3.0), F(5.0) / F(9.0), F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        c = q[0] * ty[0]
        m = q[1] * ty[1]
        p = q[2] * ty[2]
        S = c + m
        S = S + p
        cc = c * c
        mm = m * m
        pp = p * p
        Q = cc + mm
        Q = Q + pp
        t = five3 * S
        poly = F(10.0) - t
        t = five3 * Q
        poly = poly - t
        t = S * S
        t = five9 * t
        poly = poly + t
        nf = np.where(ok[0], one - c, zero) + np.where(ok[1], one - m, zero)
        nf = nf + np.where(ok[2], one - p, zero)
        nf = five3 * nf
        nf = nf + zero * S  # an unscreenable operand (S is NaN) makes the value NaN in this form too
        return np.where(ok[0] & ok[1] & ok[2], poly, nf).astype(np.float32)


def touch_need(v, thr, active):
    """the pod needs the column's exact key: it may use the column and the screen does not prove the key below thr
    (a NaN value never does)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(active, bool) & ~(np.asarray(v, np.float32) < np.asarray(thr, np.float32))


def list_thr(last_key):
    """the threshold of a cut list whose last entry keys at last_key (ksched_merge.h list_thr_bits)"""
    return (np.asarray(last_key, np.float64) - THR_MARGIN).astype(np.float32)
