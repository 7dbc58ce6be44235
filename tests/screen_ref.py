"""CPU statements of the device's score, screen and record primitives (k8s-scheduler_amd/csrc/ksched_device.h), in
numpy: what tests/test_screen_bound.py and tests/test_score_bound.py prove sound, and what
tests/test_gpu_primitives.py compares with the device's own results (ksched_selftest_*), element by element.

numpy's float32 / float64 arithmetic is IEEE round-to-nearest like the device's, and the library builds with
-ffp-contract=off, so each function below is meant to be the device computation bit for bit; the GPU test is what
checks that sentence.  Where a statement is only value-equal by design it says so."""
import numpy as np

EPS = np.float32(4e-5)      # kScreenEps
BOUND = 1.3e-5              # the polynomial's error bound ksched_device.h derives
BOUND_NF = 2e-6             # the non-fitting form's
F = np.float32
NF_BASE = F(3.375)          # kNfBase
NO_IDX = 0x7FFFFFFF         # kNoIdx


def screen_req(r):
    r = np.asarray(r, dtype=np.int64)
    out = r.astype(np.float32)
    out[(r < 0) | (r >= (1 << 52))] = np.nan
    return out


def screen_recip(a):
    a = np.asarray(a, dtype=np.int64)
    with np.errstate(divide="ignore"):
        out = (1.0 / a.astype(np.float64)).astype(np.float32)
    out[(a <= 0) | (a >= (1 << 52))] = np.nan
    return out


def screen_pair_from(qc, qm, qp, yc, ym, yp, okc, okm, okp):
    """screen_pair from its own arguments: f32 requests, f32 reciprocals, ok_k = a_k >= r_k."""
    with np.errstate(all="ignore"):
        c, m, p = qc * yc, qm * ym, qp * yp
        rf = okc & okm & okp
        fmax = np.fmax(np.fmax(c, m), p)
        S = (c + m) + p
        Q = (c * c + m * m) + p * p
        poly = ((F(10.0) - (F(5.0) / F(3.0)) * S) - (F(5.0) / F(3.0)) * Q) + (F(5.0) / F(9.0)) * (S * S)
        one = F(1.0)
        nf = (F(5.0) / F(3.0)) * ((np.where(okc, one - c, F(0)) + np.where(okm, one - m, F(0))) + np.where(okp, one - p, F(0)))
        nf = nf + F(0.0) * S
        v = np.where(rf, poly, nf).astype(np.float32)
        lo_ok = np.where(rf, fmax < F(0.999), True) & (v > EPS)
    return v, lo_ok


def screen_pair(rc, rm, rp, ac, am, ap):
    """(value, lo_ok) as screen_pair computes them; ok_k = a_k >= r_k exactly."""
    rc, rm, rp, ac, am, ap = (np.asarray(x, np.int64) for x in (rc, rm, rp, ac, am, ap))
    return screen_pair_from(screen_req(rc), screen_req(rm), screen_req(rp), screen_recip(ac), screen_recip(am),
                            screen_recip(ap), ac >= rc, am >= rm, ap >= rp)


def exact_score(rc, rm, rp, ac, am, ap):
    """anchor/priorities.go:5-23,45-50 + scores.go:3-25 in the reference's f64 operation order."""
    rcf, rmf, rpf = (np.asarray(x, np.int64).astype(np.float64) for x in (rc, rm, rp))
    acf, amf, apf = (np.asarray(x, np.int64).astype(np.float64) for x in (ac, am, ap))
    with np.errstate(all="ignore"):
        c = np.where(acf == 0, 1.0, rcf / acf)
        m = np.where(amf == 0, 1.0, rmf / amf)
        p = np.where(apf == 0, 1.0, rpf / apf)
        mean = ((c + m) + p) / 3.0
        var = (((c - mean) * (c - mean) + (m - mean) * (m - mean)) + (p - mean) * (p - mean)) / 3.0
        b = np.where((c >= 1) | (m >= 1) | (p >= 1), 0.0, (1.0 - var) * 10.0)
        lc = np.where((acf == 0) | (rcf > acf), 0.0, ((acf - rcf) * 10.0) / acf)
        lm = np.where((amf == 0) | (rmf > amf), 0.0, ((amf - rmf) * 10.0) / amf)
        lp = np.where((apf == 0) | (rpf > apf), 0.0, ((apf - rpf) * 10.0) / apf)
        l = ((lc + lm) + lp) / 3.0
        return ((0.0 + b) + l) / 2.0


# ---- the 16-bit records and their integer thresholds -------------------------------------------------------------
def screen_rec_w(w):
    """ksched_device.h screen_rec_w: the f16 pattern of w >= 0 rounded down."""
    w = np.asarray(w, np.float32)
    h = w.astype(np.float16)  # round to nearest even, like v_cvt_f16_f32
    hb = h.view(np.uint16).astype(np.int64)
    return hb - (h.astype(np.float32) > w)


def screen_rec(v):
    """ksched_device.h screen_rec: the f16 pattern of w = max(RN(10 - v), 0) rounded down (NaN -> 0)."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        w = np.fmax(F(10.0) - v, F(0.0))
    return screen_rec_w(w)


def screen_rec_nf(v):
    """0x8000 | the f16 pattern of w = max(RN(kNfBase - v), 0) rounded down."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        w = np.fmax(NF_BASE - v, F(0.0))
    return 0x8000 | screen_rec_w(w)


def rec_value(hb):
    return np.asarray(hb, np.int64).astype(np.uint16).view(np.float16).astype(np.float64)


def screen_rec_threshold(L):
    """ksched_device.h screen_rec_threshold."""
    L = np.asarray(L, np.float32)
    T = 11.0 + np.float64(EPS) + 2.0 ** -20 - L.astype(np.float64)
    h = T.astype(np.float32).astype(np.float16)
    return np.where(T >= 0, h.view(np.uint16).astype(np.int64) + 1, -1)


def screen_rec_threshold_nf(L):
    L = np.asarray(L, np.float32)
    T = np.float64(NF_BASE) + 1.0 + np.float64(EPS) + 2.0 ** -20 - L.astype(np.float64)
    h = T.astype(np.float32).astype(np.float16)
    return np.where(T >= 0, h.view(np.uint16).astype(np.int64) + 1, -1)


def needed(hb, tq, tqn):
    """ksched_device.h screen_rec_needed"""
    hb = np.asarray(hb, np.int64)
    return np.where(hb & 0x8000, (hb & 0x7FFF) <= tqn, hb <= tq)


def pass1_record(v, amb, rf, el):
    """The record pass 1 stores (ksched_pipe.hip): by the screen's form, 0 when ambiguous, 0xffff without a key."""
    rec = np.where(rf, screen_rec(v), screen_rec_nf(v))
    return np.where(amb, 0, np.where(el, rec, 0xFFFF)).astype(np.int64)


# ---- pass 1's VALU form (ksched_device.h screen_fast) ------------------------------------------------------------
def fma32(a, b, c):
    """f32 fused multiply-add: a * b + c rounded once (the product is exact in long double, the sum to 64 bits)"""
    L = np.longdouble
    return (np.asarray(a, np.float32).astype(L) * np.asarray(b, np.float32).astype(L) + np.asarray(c, np.float32).astype(L)).astype(np.float32)


def screen_fast(rc, rm, rp, ac, am, ap):
    """(v, mx, amb, rf) as screen_fast computes them from pass 1's f32 fractions."""
    rc, rm, rp, ac, am, ap = (np.asarray(x, np.int64) for x in (rc, rm, rp, ac, am, ap))
    with np.errstate(all="ignore"):
        c, m, p = screen_req(rc) * screen_recip(ac), screen_req(rm) * screen_recip(am), screen_req(rp) * screen_recip(ap)
        S = (c + m) + p
        mx = np.fmax(np.fmax(c, m), p)
        d = np.fmin(np.fmin(np.abs(c - F(1)), np.abs(m - F(1))), np.abs(p - F(1)))
        amb = ~(fma32(F(0), S, d) > F(2.0 ** -20))
        rf = mx < F(1)
        Q = fma32(c, c, fma32(m, m, p * p))
        poly = fma32(F(5.0 / 9.0), S * S, fma32(F(-5.0 / 3.0), S + Q, F(10)))
        sat = lambda x: np.clip(x, F(0), F(1))  # noqa: E731
        nf = F(5.0 / 3.0) * ((sat(F(1) - c) + sat(F(1) - m)) + sat(F(1) - p))
        v = np.where(rf, poly, nf).astype(np.float32)
    return v, mx, amb, rf


# ---- the commit's re-scoring filter (ksched_device.h resource_score_upper) ---------------------------------------
def _wsub(a, b):
    return (a.astype(np.uint64) - b.astype(np.uint64)).view(np.int64)  # Go int64 wrap-around


def _upper(rc, rm, rp, ac, am, ap, yc, ym, yp, y3):
    with np.errstate(all="ignore"):
        rcf, rmf, rpf = (x.astype(np.float64) for x in (rc, rm, rp))
        c = np.where(ac == 0, 1.0, rcf * yc)
        m = np.where(am == 0, 1.0, rmf * ym)
        p = np.where(ap == 0, 1.0, rpf * yp)
        near1 = ((ac != 0) & (np.abs(c - 1.0) < 1e-12)) | ((am != 0) & (np.abs(m - 1.0) < 1e-12)) | \
                ((ap != 0) & (np.abs(p - 1.0) < 1e-12))
        mean = ((c + m) + p) * y3
        var = (((c - mean) * (c - mean) + (m - mean) * (m - mean)) + (p - mean) * (p - mean)) * y3
        b = np.where((c >= 1.0) | (m >= 1.0) | (p >= 1.0), 0.0, (1.0 - var) * 10.0)
        dc, dm, dp = (_wsub(a, r).astype(np.float64) for a, r in ((ac, rc), (am, rm), (ap, rp)))
        lc = np.where((ac == 0) | (rc > ac), 0.0, dc * 10.0 * yc)
        lm = np.where((am == 0) | (rm > am), 0.0, dm * 10.0 * ym)
        lp = np.where((ap == 0) | (rp > ap), 0.0, dp * 10.0 * yp)
        l = ((lc + lm) + lp) * y3
        s = (b + l) * 0.5
        return s + 1e-9 * (np.abs(b) + np.abs(l) + 1.0), near1, (c >= 1) | (m >= 1) | (p >= 1)
