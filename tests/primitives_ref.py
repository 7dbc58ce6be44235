"""Operands, CPU statements and checks of the device-primitive self-tests (ksched_selftest_* in include/ksched.h).

Every check is a function of plain arrays: tests/test_gpu_primitives.py feeds it what the device returned,
tests/test_primitives_host.py what the CPU statements below return for the same operands (tests/screen_ref.py for
the score and screen families with the oracle's score in place of the device's, the network model of
tests/test_merge_network.py for the wave sort).  A check that fails on the statements is wrong itself; one that
fails only on the device's arrays is a finding.  The arrays have the layouts ksched.h documents."""
import json
import os
from fractions import Fraction

import numpy as np

import screen_ref as R
from screen_ref import BOUND, BOUND_NF, EPS, NF_BASE, NO_IDX, F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P52 = 1 << 52


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_f32(a, b):
    """bit-identical, any NaN matching any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits32(a) == bits32(b)) | (np.isnan(a) & np.isnan(b))


def same_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (bits64(a) == bits64(b)) | (np.isnan(a) & np.isnan(b))


def _none_bad(ok, what, *cols):
    """no mismatch is tolerated: name the first few offenders with their operands"""
    bad = np.nonzero(~np.asarray(ok))[0]
    assert bad.size == 0, f"{what}: {bad.size} elements differ, e.g. " + "; ".join(
        f"[{i}] " + " ".join(repr(np.asarray(c)[..., i].tolist()) for c in cols) for i in bad[:4])


# ---- operands ------------------------------------------------------------------------------------------------------
def _edges():
    """(requests, allocatables) where kernels go wrong: zero, negative and unit allocatables, a negative request, the
    2^52 / 2^53 conversion limits, +-2^62 (wsub wraps), requests at and around the allocatable, all-zero requests."""
    e = [((1, 1, 1), (3, 3, 3)),                      # element 0: its recip is the y3 every score uses
         ((1, 1, 1), (0, 10, 10)), ((1, 1, 1), (0, 0, 0)), ((0, 0, 0), (0, 0, 0)), ((0, 5, 1), (10, 0, 0)),
         ((1, 1, 1), (-1, 10, 10)), ((5, 5, 5), (-100, -7, 10)), ((0, 0, 0), (-1, -1, -1)), ((1, 2, 3), (10, -1, 10)),
         ((-5, 1, 1), (10, 10, 10)), ((1, -5, 1), (10, 10, 10)), ((-5, -5, -5), (10, 10, 10)),
         ((P52 - 1, 1, 1), (P52 - 1, 10, 10)), ((1, 1, 1), (P52 - 1, P52 - 1, P52 - 1)), ((1, 1, 1), (P52, 10, 10)),
         ((P52, 1, 1), (P52 + 5, 10, 10)), ((P52 - 1, 1, 1), (P52, 10, 10)), ((P52 - 2, P52 - 1, 1), (P52 - 1, P52 - 1, 1)),
         (((1 << 53) + 1, 1, 1), ((1 << 53) + 1, 10, 10)), ((1, 1, 1), ((1 << 53) + 1, 10, 10)),
         (((1 << 53) + 1, 1, 1), ((1 << 53) + 3, 10, 10)), ((1 << 62, 1, 1), (-(1 << 62), 10, 10)),
         ((-(1 << 62), 1, 1), (1 << 62, 10, 10)), ((1 << 62, 1 << 62, 1), (1 << 62, (1 << 62) + 1, 10)),
         ((1, 1, 1), (1 << 62, -(1 << 62), 10)), ((0, 0, 0), (10, 20, 30)), ((0, 0, 0), (1, 1, 1)),
         ((1, 1, 1), (1, 1, 1)), ((1, 0, 0), (1, 5, 5)), ((2, 0, 0), (1, 5, 5)), ((0, 0, 1), (7, 7, 1)),
         ((1, 1, 1), (2, 2, 2)), ((500, 1 << 20, 1), (64000, 1 << 36, 110))]
    for a in (10, 1_000_003, 1 << 40, P52 - 3):
        for d in (-2, -1, 0, 1, 2):
            e.append(((a + d, 1, 1), (a, 10, 10)))
            e.append(((1, a + d, a + d), (10, a, a)))
    return np.array([x[0] for x in e], np.int64).T.copy(), np.array([x[1] for x in e], np.int64).T.copy()


def _with_edges(req, alloc):
    er, ea = _edges()
    k = er.shape[1]
    req, alloc = req.copy(), alloc.copy()
    req[:, :k], alloc[:, :k] = er, ea
    return np.ascontiguousarray(req), np.ascontiguousarray(alloc)


def fast53_ok(req, alloc):
    """resource_score_fast<true>'s host-checked precondition: every magnitude below 2^52"""
    return ((np.abs(req.astype(np.float64)) < P52) & (np.abs(alloc.astype(np.float64)) < P52)).all(axis=0)


def score_operands(seed, n):
    from test_score_bound import _cases
    rc, rm, rp, ac, am, ap = _cases(np.random.default_rng(seed), n)
    return _with_edges(np.stack([rc, rm, rp]), np.stack([ac, am, ap]))


def upper_operands(seed, n):
    """test_score_bound._cases with 'exactly full' drawn with probability 3 % per resource: _cases makes 22 % of the
    resources exactly full, which flags about 52 % of its pairs near1 and would leave the bound half untested."""
    rng = np.random.default_rng(seed)

    def one_res(scale):
        a = rng.integers(-scale // 4, scale, n)
        kind = rng.integers(0, 6, n)
        r = rng.integers(0, scale, n)
        r = np.where(kind == 1, a - rng.integers(1, 3, n), r)  # one or two below full
        r = np.where(kind == 2, a + 1, r)
        a = np.where(kind == 3, 0, a)                          # zero allocatable
        r = np.where(kind == 4, 0, r)
        r = np.where(rng.random(n) < 0.03, a, r)               # exactly full
        return r.astype(np.int64), a.astype(np.int64)
    rc, ac = one_res(64_000)
    rm, am = one_res(1 << 36)
    rp, ap = one_res(120)
    big = rng.random(n) < 0.05
    ac = np.where(big, rng.integers(-(1 << 62), 1 << 62, n), ac)
    rc = np.where(big, rng.integers(0, 1 << 62, n), rc)
    req, alloc = np.stack([rc, rm, rp]), np.stack([ac, am, ap])
    req[:, 0], alloc[:, 0] = (1, 1, 1), (3, 3, 3)              # element 0 carries y3
    return np.ascontiguousarray(req), np.ascontiguousarray(alloc)


def recip_operands(seed, n):
    """integer-valued divisors of every magnitude 1 .. 2^62, both signs, with the powers of two and their neighbours;
    element 0 is 3"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(1 << 61, 1 << 62, (3, n), dtype=np.int64) >> rng.integers(0, 62, (3, n))).astype(np.int64)
    a = np.maximum(a, 1)
    p2 = np.array([(1 << k) + d for k in range(63) for d in (-1, 0, 1) if 1 <= (1 << k) + d <= 1 << 62], np.int64)
    a[1, :p2.size] = p2
    a[2, :200] = np.arange(1, 201)
    a = np.where(rng.random((3, n)) < 0.3, -a, a)
    a[:, 0] = 3
    return np.zeros((3, n), np.int64), np.ascontiguousarray(a)


def price_operands(seed, n):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-5, 5, n - 4096), rng.uniform(0, 1e-38, 2048), -rng.uniform(0, 1e-38, 2048)]).astype(np.float32)
    fi = np.finfo(np.float32)
    tiny = np.array([1, 2, 0x7FFFFF, 0x800000], np.uint32).view(np.float32)  # denormals and the smallest normal
    sp = np.concatenate([F([0.0, -0.0, fi.max, -fi.max, 1.0, -1.0, 0.05, 1.6]), tiny, -tiny])
    p[:sp.size] = sp
    return p


def screen_operands(seed, n):
    """test_screen_bound._pairs, a quarter each: as they are, with requests over the allocatable
    (test_non_fitting_form), within two of it (test_screen_fast_matches_the_bounds) and with an unscreenable operand
    (negative or >= 2^52 request, non-positive or >= 2^52 allocatable); then the explicit edges."""
    from test_screen_bound import _pairs
    rng = np.random.default_rng(seed)
    r, a = _pairs(rng, n)
    kind = np.arange(n) % 4
    over = (rng.random((3, n)) < 0.4) & (kind == 1)
    k1 = np.nonzero(kind == 1)[0]
    over[rng.integers(0, 3, k1.size), k1] = True
    big = np.minimum(a + 1 + (rng.random((3, n)) * a * 4).astype(np.int64), P52 - 1)
    r = np.where(over & (a < P52 - 1), big, r)
    k2 = np.nonzero(kind == 2)[0]
    res = rng.integers(0, 3, k2.size)
    r[res, k2] = np.maximum(a[res, k2] + rng.integers(-2, 3, k2.size), 0)
    k3 = np.nonzero(kind == 3)[0]
    res = rng.integers(0, 3, k3.size)
    which = rng.integers(0, 6, k3.size)
    bad_r = np.choose(which % 3, [-rng.integers(1, 1 << 40, k3.size), np.full(k3.size, P52), rng.integers(P52, 1 << 62, k3.size)])
    bad_a = np.choose(which % 3, [-rng.integers(0, 1 << 40, k3.size), np.full(k3.size, P52), rng.integers(P52, 1 << 62, k3.size)])
    r[res, k3] = np.where(which < 3, bad_r, r[res, k3])
    a[res, k3] = np.where(which >= 3, bad_a, a[res, k3])
    return _with_edges(r.astype(np.int64), a.astype(np.int64))


def rec_operands():
    """every f16 pattern of [0, 10] (0 .. 0x4900: the resource-fitting records; 0 .. 0x42C0 of them are the
    non-fitting ones') as an f32 w with its two f32 neighbours; w2 pairs each w with another one"""
    h = np.arange(0, 0x4900 + 1, dtype=np.uint16).view(np.float16).astype(np.float32)
    w = np.concatenate([h, np.nextafter(h, F(-1)), np.nextafter(h, F(11))])
    w = w[w >= 0]
    w = np.concatenate([w, F([10.0, 3.375, 1e-30, 6.1e-5, 6.0e-8, 5.9e-8, 2.9e-8, 3.1e-8])])
    return np.ascontiguousarray(w), np.ascontiguousarray(np.roll(w, 12345))


def threshold_operands():
    """the L and record sets of test_pass2_two_form_threshold_is_a_superset (L = 0 among them), each L once with a
    resource-fitting and once with a non-fitting record, then the no-key and always-needed patterns"""
    rng = np.random.default_rng(23)
    L = np.concatenate([rng.uniform(0, 11.001, 60000), 4.25 - rng.uniform(0, 0.1, 20000), F([0.0, 1.0, 4.375, 11.0])]).astype(np.float32)
    n = L.size
    poly = rng.integers(0, 0x4901, n)
    nfr = 0x8000 | rng.integers(0, 0x42C1, n)
    sp = np.array([0, 0x8000, 0x4900, 0xFFFF, 0xC2C0], np.int64)
    Ls = np.repeat(F([0.0, 1.0, 4.375, 11.0, 11.5, 14.0]), sp.size)
    rec = np.concatenate([poly, nfr, np.tile(sp, 6)]).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([L, L, Ls])), np.ascontiguousarray(rec)


# ---- CPU statements in the device's output layouts -----------------------------------------------------------------
def oracle_scores(oracle_mod, req, alloc):
    return np.array([oracle_mod.score(*t) for t in zip(*(x.tolist() for x in (*req, *alloc)))], np.float64)


def score_statement(req, alloc, ex):
    """the score entry point's arrays from the CPU side: the oracle's score in all three forms, numpy's correctly
    rounded reciprocals, screen_ref._upper on them"""
    af = alloc.astype(np.float64)
    with np.errstate(all="ignore"):
        y = np.where(alloc == 0, 0.0, 1.0 / af)
        rcp = 1.0 / af
    hi, near1, _ = R._upper(*req, *alloc, y[0], y[1], y[2], 1.0 / 3.0)
    fit = (alloc >= req).all(axis=0)
    flags = near1 * 3 + (ex > 0) * 4 + ((ex > 0) & fit) * 8 + fit * 16
    return dict(score=np.stack([ex, ex, ex]), upper=np.stack([hi, hi]), recip=rcp, flags=flags.astype(np.int32))


def screen_statement(req, alloc):
    q = [R.screen_req(x) for x in req]
    y = [R.screen_recip(x) for x in alloc]
    ok = [alloc[k] >= req[k] for k in range(3)]
    v, lo = R.screen_pair_from(*q, *y, *ok)
    fv, mx, amb, rf = R.screen_fast(*req, *alloc)
    f = np.stack([*q, *y, *y, v, v, fv, mx]).astype(np.float32)
    ra, rfe = R.pass1_record(fv, amb, rf, True), R.pass1_record(fv, amb, rf, rf)
    u = np.stack([lo, lo, amb, rf, ra, ra, rfe, rfe]).astype(np.uint32)
    return dict(f=f, u=u)


def rec_w_statement(w, w2):
    a, b = R.screen_rec_w(w), R.screen_rec_w(w2)
    return np.stack([a, b, a, b]).astype(np.uint32)


def threshold_statement(L, rec):
    tq, tqn = R.screen_rec_threshold(L), R.screen_rec_threshold_nf(L)
    return np.stack([tq, tqn, R.needed(rec, tq, tqn), R.needed(rec, -1, -1)]).astype(np.int32)


# ---- checks: score family -------------------------------------------------------------------------------------------
def check_score(req, alloc, out, ex):
    """resource_score and resource_score_fast<false> carry the oracle's bits everywhere, <true> wherever its
    precondition holds (at least half of the elements); eligibility is score > 0 (and fits, feasible domain)."""
    pre = fast53_ok(req, alloc)
    assert pre.mean() >= 0.5, f"FAST53 coverage {pre.mean():.3f}"
    assert not np.isnan(ex).any()
    _none_bad(bits64(out["score"][0]) == bits64(ex), "resource_score vs oracle", req, alloc)
    _none_bad(bits64(out["score"][1]) == bits64(ex), "resource_score_fast<false> vs oracle", req, alloc)
    _none_bad((bits64(out["score"][2]) == bits64(ex)) | ~pre, "resource_score_fast<true> vs oracle", req, alloc)
    fl = out["flags"]
    fit = (alloc >= req).all(axis=0)
    _none_bad(((fl >> 4) & 1) == fit, "fits", req, alloc)
    _none_bad(((fl >> 2) & 1) == (ex > 0), "eligible (all-node domain)", req, alloc)
    _none_bad(((fl >> 3) & 1) == ((ex > 0) & fit), "eligible (feasible domain)", req, alloc)
    return dict(fast53_share=float(pre.mean()))


def kat_operands():
    kats = json.load(open(os.path.join(GOLDEN, "score_kats.json")))
    req = np.array([k["req"] for k in kats], np.int64).T.copy()
    alloc = np.array([k["alloc"] for k in kats], np.int64).T.copy()
    want = np.array([float.fromhex(k["score_hex"]) for k in kats], np.float64)
    return req, alloc, want


def check_price_key(price, key):
    want = -price.astype(np.float64) + 0.0
    _none_bad(bits64(key) == bits64(want), "price_key", price)
    assert not (np.signbit(key) & (key == 0)).any(), "price_key returned -0.0"
    z = price == 0
    assert z.sum() >= 2 and (bits64(key[z]) == 0).all()


def check_recip(alloc, rcp):
    """recip(af) within 1 ulp of the correctly rounded 1 / af; returns the worst distance in ulps"""
    nz = alloc != 0
    want = 1.0 / alloc[nz].astype(np.float64)
    d = np.abs(bits64(rcp[nz]) - bits64(want))
    worst = int(d.max())
    print(f"recip: worst distance from the correctly rounded reciprocal {worst} ulp over {d.size} divisors "
          f"({(d > 0).mean():.2%} not exact)")
    assert worst <= 1, f"recip is {worst} ulp off"
    return worst


def check_upper(req, alloc, out, ex, share_cap=0.10):
    """With the reciprocals of out['recip'] (element 0's allocatable is 3: y3): the bound is screen_ref._upper bit for
    bit; near1 | (upper >= score); outside near1 the branch 'some fraction >= 1' is the exact one; near1 only where a
    fraction is within 2e-12 of 1; at most share_cap of the pairs flagged."""
    assert tuple(alloc[:, 0]) == (3, 3, 3)
    pre = fast53_ok(req, alloc)
    y = np.where(alloc == 0, 0.0, out["recip"])  # recip_or_zero
    y3 = out["recip"][0, 0]
    hi, near1_m, br = R._upper(*req, *alloc, y[0], y[1], y[2], y3)
    fl = out["flags"]
    near1, near1_t = (fl & 1) == 1, ((fl >> 1) & 1) == 1
    _none_bad(near1 == near1_m, "near1 vs the statement", req, alloc)
    _none_bad((near1_t == near1_m) | ~pre, "near1 <FAST53> vs the statement", req, alloc)
    _none_bad(same_f64(out["upper"][0], hi), "resource_score_upper<false> vs the statement", req, alloc)
    _none_bad(same_f64(out["upper"][1], hi) | ~pre, "resource_score_upper<true> vs the statement", req, alloc)
    rf, af = req.astype(np.float64), alloc.astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.where(alloc == 0, 1.0, rf / np.where(alloc == 0, 1.0, af))
        close = ((alloc != 0) & (np.abs(rf / np.where(alloc == 0, 1.0, af) - 1.0) < 2e-12)).any(axis=0)
    ebr = (e >= 1).any(axis=0)
    _none_bad(near1 | (br == ebr), "balanced branch outside near1", req, alloc)
    _none_bad(near1 | (out["upper"][0] >= ex), "upper<false> >= score", req, alloc, out["upper"][0], ex)
    _none_bad(near1_t | (out["upper"][1] >= ex) | ~pre, "upper<true> >= score", req, alloc, out["upper"][1], ex)
    _none_bad(~near1 | close, "near1 away from a full resource", req, alloc)
    share = float(near1.mean())
    assert share <= share_cap, f"near1 flags {share:.3f} of the pairs"
    slack = (out["upper"][0] - ex)[~near1]
    return dict(near1_share=share, worst_slack=float(slack.max()))


# ---- checks: screen family ------------------------------------------------------------------------------------------
def _f32_exact(x):
    """round a Fraction to the nearest f32 (ties to even); the values here are far from the exponent limits"""
    if x == 0:
        return 0.0
    s, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = x / Fraction(2) ** (e - 23)
    m = q.numerator // q.denominator
    rem = q - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (m & 1)):
        m += 1
    return s * float(Fraction(m) * Fraction(2) ** (e - 23))


def screen_fast_poly_exact(c, m, p):
    """screen_fast's polynomial for three f32 fractions with each fused multiply-add rounded once, in exact rational
    arithmetic: the referee between the device and screen_ref.fma32 (which rounds through long double)."""
    fr = lambda x: Fraction(float(x))  # noqa: E731
    fma = lambda a, b, cc: _f32_exact(fr(a) * fr(b) + fr(cc))  # noqa: E731
    S = F(F(c + m) + p)
    Q = fma(c, c, fma(m, m, F(p * p)))
    return F(fma(F(5.0 / 9.0), F(S * S), fma(F(-5.0 / 3.0), F(S + F(Q)), F(10))))


def _referee(req, alloc, got_v, want_v, idx):
    """for polynomial values that differ: which side the exact arithmetic is on"""
    out = []
    for i in idx[:6]:
        c, m, p = (R.screen_req(req[k, i:i + 1])[0] * R.screen_recip(alloc[k, i:i + 1])[0] for k in range(3))
        ex = screen_fast_poly_exact(c, m, p)
        out.append(f"[{i}] device {got_v[i]!r} statement {want_v[i]!r} exact {ex!r}")
    return "; ".join(out)


def check_screen_identity(req, alloc, out):
    """The device's arrays are tests/screen_ref.py's, bit for bit (NaN matching NaN): screen_req, screen_recip, the
    screen_pair value built from screen_recip with its lo_ok, amb; where not ambiguous also rf, mx, v and the record
    (ambiguous: the record is 0, v and rf are don't-care).  The record's two paths agree everywhere; screen_y is
    screen_recip within one f32 ulp, NaN in the same places."""
    st = screen_statement(req, alloc)
    f, u, sf, su = out["f"], out["u"], st["f"], st["u"]
    for k, name in enumerate(["screen_req c", "screen_req m", "screen_req p", "screen_recip c", "screen_recip m",
                              "screen_recip p"]):
        _none_bad(same_f32(f[k], sf[k]), name, req, alloc, f[k], sf[k])
    _none_bad(same_f32(f[9], sf[9]), "screen_pair value", req, alloc, f[9], sf[9])
    _none_bad(u[0] == su[0], "screen_pair lo_ok", req, alloc)
    _none_bad(u[2] == su[2], "screen_fast amb", req, alloc)
    na = su[2] == 0
    _none_bad((u[3] == su[3]) | ~na, "screen_fast rf", req, alloc)
    _none_bad(same_f32(f[12], sf[12]) | ~na, "screen_fast mx", req, alloc, f[12], sf[12])
    vbad = np.nonzero(~(same_f32(f[11], sf[11]) | ~na))[0]
    assert vbad.size == 0, f"screen_fast v: {vbad.size} elements differ: " + _referee(req, alloc, f[11], sf[11], vbad)
    for k in (4, 5, 6, 7):
        _none_bad(u[k] == su[k], f"pass-1 record (row {k})", req, alloc, u[k], su[k], f[11])
    _none_bad((u[4] == u[5]) & (u[6] == u[7]), "record paths (screen_rec* vs cvt_pkrtz)", req, alloc, u[4], u[5])
    assert (u[4][~na] == 0).all() and (u[6][~na] == 0).all()
    # screen_y = (float)recip(a): value-equal by design only
    for k in range(3):
        yy, ys = f[6 + k], f[3 + k]
        _none_bad(np.isnan(yy) == np.isnan(ys), "screen_y NaN domain", alloc)
        fin = ~np.isnan(ys)
        _none_bad(np.abs(bits32(yy[fin]).astype(np.int64) - bits32(ys[fin])) <= 1, "screen_y within 1 f32 ulp", alloc[:, fin])
    return dict(ambiguous_share=float((~na).mean()), nan_share=float(np.isnan(sf[9]).mean()),
                non_fitting_share=float((na & (su[3] == 0)).mean()))


def check_screen_sound(req, alloc, out, ex):
    """The inequalities of tests/test_screen_bound.py on these arrays against the f64 score ex: BOUND / BOUND_NF / EPS
    for both screen_pair variants and for screen_fast, the records as upper bounds, nf < kNfBase, and
    lo_ok => score > 0 and v - eps < score.  Returns the worst error of each form."""
    f, u = out["f"], out["u"]
    fit = (alloc >= req).all(axis=0)
    nfit = (req > alloc).any(axis=0)
    one = (req == alloc).any(axis=0)
    worst = {}
    eps = float(EPS)
    for name, v, lo in (("screen_pair(screen_recip)", f[9], u[0] == 1), ("screen_pair(screen_y)", f[10], u[1] == 1)):
        fin = np.isfinite(v)
        assert not np.isinf(v).any()
        v64 = v.astype(np.float64)
        err = np.abs(v64 - ex)
        a = fin & fit & ~one
        worst[name + " polynomial"] = float(err[a].max())
        _none_bad(~a | (err < BOUND), name + ": polynomial error", req, alloc, v, ex)
        _none_bad(~fin | (v64 + eps >= ex), name + ": v + eps >= score", req, alloc, v, ex)
        b = fin & nfit
        worst[name + " non-fitting"] = float(err[b].max())
        _none_bad(~b | (err < BOUND_NF), name + ": non-fitting error", req, alloc, v, ex)
        _none_bad(~b | (v < NF_BASE), name + ": non-fitting value below kNfBase", req, alloc, v)
        assert not (lo & ~fin).any()
        _none_bad(~lo | ((ex > 0) & ((v - EPS).astype(np.float64) < ex)), name + ": lo_ok", req, alloc, v, ex)
        assert a.mean() > 0.1 and b.mean() > 0.1 and lo.mean() > 0.1
    # screen_fast, where it is not ambiguous (an ambiguous pair is scored exactly)
    v, mx, amb, rf = f[11], f[12], u[2] == 1, u[3] == 1
    ok = ~amb
    assert np.isfinite(v[ok]).all()
    v64 = v.astype(np.float64)
    err = np.abs(v64 - ex)
    _none_bad(~ok | (rf == fit), "screen_fast rf is the exact fit", req, alloc)
    pf = ok & rf & (mx < F(0.999))
    worst["screen_fast polynomial"] = float(err[pf].max())
    _none_bad(~pf | (err < BOUND), "screen_fast: polynomial error", req, alloc, v, ex)
    _none_bad(~(ok & rf) | (v64 + eps >= ex), "screen_fast: v + eps >= score", req, alloc, v, ex)
    nfm = ok & ~rf
    worst["screen_fast non-fitting"] = float(err[nfm].max())
    _none_bad(~nfm | (err < BOUND_NF), "screen_fast: non-fitting error", req, alloc, v, ex)
    _none_bad(~nfm | (v < NF_BASE), "screen_fast: nf < kNfBase", req, alloc, v)
    lo = ok & ~(rf & (mx >= F(0.999))) & (v > EPS)
    _none_bad(~lo | ((ex > 0) & ((v - EPS).astype(np.float64) < ex)), "screen_fast: pass-1 lower bound", req, alloc, v, ex)
    assert pf.mean() > 0.1 and nfm.mean() > 0.1
    # the records: what pass 2 implies of one (base - value(h) + 2^-21) bounds the screen value, so with eps the score
    for row, dom in ((4, "all-node"), (6, "feasible")):
        h = u[row].astype(np.int64)
        key = ok & (h != 0xFFFF)
        isnf = (h & 0x8000) != 0
        assert not (key & (isnf == rf)).any(), "record form differs from rf"
        base = np.where(isnf, np.float64(NF_BASE), 10.0)
        ub = base - R.rec_value(h & 0x7FFF)
        _none_bad(~key | (ub + 2.0 ** -21 >= v64), f"record ({dom}) bounds the screen value", req, alloc, h, v)
        _none_bad(~key | (ub + 2.0 ** -21 + eps >= ex), f"record ({dom}) bounds the score", req, alloc, h, ex)
        assert ((h[key & ~isnf] <= 0x4900).all() and ((h[key & isnf] & 0x7FFF) <= 0x42C0).all())
        if row == 6:
            _none_bad(~ok | ((h == 0xFFFF) == ~rf), "feasible domain: a key iff the pair fits", req, alloc, h)
        else:
            assert (h[ok] != 0xFFFF).all()
    for k, e in worst.items():
        print(f"screen: worst |{k} - score| = {e:.3e}")
    return worst


def check_rec_w(w, w2, out):
    """screen_rec_w is the true round-down to f16 (value(h) <= w < value(h + 1)), equal to the statement, and both
    halves of the packed round-toward-zero conversion are that record"""
    st = rec_w_statement(w, w2)
    for row, x in ((0, w), (1, w2)):
        h = out[row].astype(np.int64)
        _none_bad(h == st[row], "screen_rec_w vs the statement", x, h)
        lo, hi = R.rec_value(h), R.rec_value(h + 1)
        _none_bad((lo <= x.astype(np.float64)) & (x.astype(np.float64) < hi), "screen_rec_w rounds down", x, h)
    _none_bad(out[2] == out[0], "cvt_pkrtz low half", w, out[2], out[0])
    _none_bad(out[3] == out[1], "cvt_pkrtz high half", w2, out[3], out[1])
    nfr = w <= NF_BASE  # the non-fitting records: the same patterns with bit 15
    assert ((0x8000 | out[2][nfr].astype(np.int64)) == (0x8000 | R.screen_rec_w(w[nfr]))).all()
    assert int(out[0].max()) == 0x4900 and int(out[0][nfr].max()) == 0x42C0 and int(out[0].min()) == 0


def check_threshold(L, rec, out):
    """the thresholds and the needed test are the statement's, and have the superset property of
    test_pass2_two_form_threshold_is_a_superset"""
    st = threshold_statement(L, rec)
    for row, name in enumerate(["screen_rec_threshold", "screen_rec_threshold_nf", "screen_rec_needed",
                                "screen_rec_needed(-1, -1)"]):
        _none_bad(out[row] == st[row], name, L, rec, out[row], st[row])
    h = rec.astype(np.int64)
    Ld = L.astype(np.float64)
    isnf = (h & 0x8000) != 0
    haskey = np.where(isnf, (h & 0x7FFF) <= 0x42C0, h <= 0x4900)
    base = np.where(isnf, np.float64(NF_BASE), 10.0)
    with np.errstate(invalid="ignore"):
        need = haskey & ((base - R.rec_value(h & 0x7FFF)) + 2.0 ** -21 + 1.0 + np.float64(EPS) >= Ld)
    got = out[2] == 1
    _none_bad(~need | got, "a needed record is not admitted", L, rec)
    assert not got[h == 0xFFFF].any(), "the no-key pattern was admitted"
    assert got[(h == 0) & (Ld <= 11.0)].all(), "an always-needed record was refused"
    assert not out[3].any(), "an inactive lane needs nothing"
    assert (out[0][Ld == 0] >= 0x4900 + 1).all() and (out[0][Ld == 0] < 0xFFFF).all() and (Ld == 0).any()


# ---- wave family ----------------------------------------------------------------------------------------------------
RUNS = (1, 2, 4, 8, 16, 32)
KCS = (2, 4, 8, 16)
LIST_ROW0 = (0, 2, 6, 14)
LIST_STEPS = 24
KEY_KINDS = ("random", "ties", "few", "empties", "all-empty", "negative", "-inf valid", "inf+denormal")


def key_code(k):
    """ksched_device.h key_code: order-preserving f64 -> u64"""
    u = np.ascontiguousarray(k, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def _order(code, idx):
    """per row: the permutation that sorts (code desc, idx asc)"""
    return np.lexsort((idx, ~code), axis=-1)


def wave_cases(seed, nc, kind_name):
    """nc cases of one key kind.  Arg-best inputs (key, idx, aux) by kind; sort inputs (code, idx): the keys'
    codes in even cases, random 64-bit codes of the kinds of test_merge_network.py in odd ones ((code, idx) distinct
    except the empty (0, kNoIdx)); no NaN and no -0.0 key."""
    rng = np.random.default_rng(seed)
    kind = np.full(nc, KEY_KINDS.index(kind_name))
    idx = np.argsort(rng.random((nc, 1 << 10)), axis=1)[:, :64].astype(np.int32) * 977 + rng.integers(0, 900, (nc, 1)).astype(np.int32)
    key = rng.uniform(0.0, 10.0, (nc, 64))
    tie = rng.uniform(0.0, 10.0, (nc, 1))
    few = rng.uniform(0.0, 10.0, (nc, 3))
    key = np.where((kind == 1)[:, None], tie, key)
    key = np.where((kind == 2)[:, None], np.take_along_axis(few, rng.integers(0, 3, (nc, 64)), axis=1), key)
    key = np.where((kind == 5)[:, None], -rng.uniform(0.0, 1e3, (nc, 64)) * rng.integers(0, 2, (nc, 64)) - 1e-9, key)
    special = np.array([np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, -1e-310, 1.0, -1.0, 1.7e308, -1.7e308])
    key = np.where((kind == 7)[:, None], special[rng.integers(0, special.size, (nc, 64))], key)
    nvalid = rng.integers(0, 64, nc)
    nvalid = np.where(kind == 4, 0, np.where((kind == 3) | (kind == 6), nvalid, 64))
    lanes = np.argsort(rng.random((nc, 64)), axis=1)
    empty = lanes >= nvalid[:, None]
    key = np.where((kind == 6)[:, None], -np.inf, key)
    key = np.where(empty, -np.inf, key)
    kidx = np.where(empty, NO_IDX, idx).astype(np.int32)
    aux = np.where(empty, -1, rng.integers(0, 1 << 20, (nc, 64))).astype(np.int32)
    # sort inputs
    code = key_code(key)
    rcode = rng.integers(1, 1 << 63, (nc, 64), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nc, 64), dtype=np.uint64)
    rt = rng.integers(1, 1 << 63, (nc, 1), dtype=np.uint64)
    rf = rng.integers(1, 1 << 63, (nc, 3), dtype=np.uint64)
    rcode = np.where((kind == 1)[:, None], rt, rcode)
    rcode = np.where((kind == 2)[:, None], np.take_along_axis(rf, rng.integers(0, 3, (nc, 64)), axis=1), rcode)
    code = np.where((np.arange(nc) % 2 == 1)[:, None], rcode, code)
    code = np.where(empty, np.uint64(0), code)
    runs_code, runs_idx = [], []
    for run in RUNS:  # aligned sorted runs of `run` pairs
        c3, i3 = code.reshape(nc, 64 // run, run), kidx.reshape(nc, 64 // run, run)
        o = _order(c3, i3)
        runs_code.append(np.take_along_axis(c3, o, axis=-1).reshape(nc, 64))
        runs_idx.append(np.take_along_axis(i3, o, axis=-1).reshape(nc, 64))
    cut = rng.integers(0, 2, nc).astype(np.int32)
    nv = rng.integers(0, 65, nc).astype(np.int32)
    nv[::7], nv[3::7] = 0, 64
    return dict(ncases=nc, kind=kind, sort_code=np.ascontiguousarray(np.stack(runs_code)),
                sort_idx=np.ascontiguousarray(np.stack(runs_idx)), key=np.ascontiguousarray(key), idx=kidx, aux=aux,
                cut=cut, nv=nv)


def _better(ka, ia, kb, ib):
    return (ka > kb) | ((ka == kb) & (ia < ib))


def wave_statement(cs):
    """the wave entry point's arrays from the CPU side: the sort by the network of tests/test_merge_network.py, the
    rest by direct restatements of ksched_device.h / ksched_merge.h"""
    from test_merge_network import network
    nc = cs["ncases"]
    lane = np.arange(64)
    u = np.zeros((12, nc, 64), np.uint64)
    v = np.zeros((13, nc, 64), np.int32)
    for r, run in enumerate(RUNS):
        code, idx = cs["sort_code"][r].copy(), cs["sort_idx"][r].copy()
        for m, hb in network(run):
            pc, pi = code[:, lane ^ m], idx[:, lane ^ m]
            pb = _better(pc, pi, code, idx)
            take = np.where((lane & hb) != 0, ~pb, pb)
            code, idx = np.where(take, pc, code), np.where(take, pi, idx)
        u[r], v[r] = code, idx
    c0, i0 = cs["sort_code"][0], cs["sort_idx"][0]
    v[6] = _better(c0[:, :, None], i0[:, :, None], c0[:, None, :], i0[:, None, :]).sum(axis=1)  # wave_rank
    u[6] = c0.max(axis=1, keepdims=True)
    u[7] = c0.sum(axis=1, keepdims=True, dtype=np.uint64)
    v[7] = i0.min(axis=1, keepdims=True)
    u[11] = np.bitwise_or.reduce(c0, axis=1, keepdims=True)
    key, kidx, aux = cs["key"], cs["idx"], cs["aux"]
    bk, bi, ba = key[:, 0].copy(), kidx[:, 0].copy(), aux[:, 0].copy()  # wave_argbest: a reduction by better()
    for l in range(1, 64):
        t = _better(key[:, l], kidx[:, l], bk, bi)
        bk, bi, ba = np.where(t, key[:, l], bk), np.where(t, kidx[:, l], bi), np.where(t, aux[:, l], ba)
    u[8], v[8], v[10] = bk.view(np.uint64)[:, None], bi[:, None], ba[:, None]
    mine = np.where(kidx == NO_IDX, np.uint64(0), key_code(key))  # wave_argbest_fast
    best = mine.max(axis=1, keepdims=True)
    mi = np.where(mine == best, kidx, NO_IDX).min(axis=1, keepdims=True)
    src = np.argmax((mine == best) & (kidx == mi), axis=1)[:, None]
    none = best == 0
    u[9] = np.where(none, np.float64(-np.inf).view(np.uint64), np.take_along_axis(key, src, 1).view(np.uint64))
    v[9] = np.where(none, NO_IDX, np.take_along_axis(kidx, src, 1))
    v[11] = np.where(none, -1, np.take_along_axis(aux, src, 1))
    u[10] = key_code(key)
    nv, cut = cs["nv"], cs["cut"]
    last = np.take_along_axis(key, np.maximum(nv - 1, 0)[:, None].astype(np.int64), 1)[:, 0]  # list_thr_bits
    with np.errstate(all="ignore"):
        t = np.where((cut != 0) & (nv > 0), (last - 5e-5).astype(np.float32), F(-np.inf)).astype(np.float32)
    v[12] = t.view(np.int32)[:, None]
    return dict(u=u.reshape(12, nc * 64), v=v.reshape(13, nc * 64))


def check_wave(cs, out):
    nc = cs["ncases"]
    u, v = out["u"].reshape(12, nc, 64), out["v"].reshape(13, nc, 64)
    c0, i0 = cs["sort_code"][0], cs["sort_idx"][0]
    o = _order(c0, i0)
    want_c, want_i = np.take_along_axis(c0, o, 1), np.take_along_axis(i0, o, 1)
    for r, run in enumerate(RUNS):  # lane r holds rank r of sorted(key=(-code, idx)), empties last
        bad = ((u[r] != want_c) | (v[r] != want_i)).any(axis=1)
        assert not bad.any(), f"wave_sort_desc<{run}>: {bad.sum()} cases differ, e.g. {np.nonzero(bad)[0][:4]}"
    pos = np.empty_like(o)
    np.put_along_axis(pos, o, np.broadcast_to(np.arange(64), o.shape), 1)
    nval = (i0 != NO_IDX).sum(axis=1, keepdims=True)
    pos = np.where(i0 == NO_IDX, nval, pos)  # every empty pair ranks after the valid ones
    assert (v[6] == pos).all(), "wave_rank"
    assert (u[6] == c0.max(axis=1, keepdims=True)).all(), "wave_max_u64"
    assert (u[7] == c0.sum(axis=1, keepdims=True, dtype=np.uint64)).all(), "wave_sum_i64"
    assert (v[7] == i0.min(axis=1, keepdims=True)).all(), "wave_min_i32"
    assert (u[11] == np.bitwise_or.reduce(c0, axis=1, keepdims=True)).all(), "wave_or_u64"
    key, kidx, aux = cs["key"], cs["idx"], cs["aux"]
    assert not np.isnan(key).any() and not (np.signbit(key) & (key == 0)).any()
    b = np.lexsort((kidx, -key), axis=-1)[:, :1]  # the best by (key desc, idx asc)
    wk, wi, wa = (np.take_along_axis(x, b, 1) for x in (key, kidx, aux))
    for row_u, row_i, row_a, name in ((8, 8, 10, "wave_argbest"), (9, 9, 11, "wave_argbest_fast")):
        bad = ((u[row_u] != wk.view(np.uint64)) | (v[row_i] != wi) | (v[row_a] != wa)).any(axis=1)
        assert not bad.any(), f"{name}: {bad.sum()} cases differ, e.g. {np.nonzero(bad)[0][:4]}"
    allempty = (kidx == NO_IDX).all(axis=1)
    name = KEY_KINDS[int(cs["kind"][0])]
    assert allempty.all() if name == "all-empty" else not allempty.all()
    assert ((u[9][allempty] == np.float64(-np.inf).view(np.uint64)) & (v[9][allempty] == NO_IDX) & (v[11][allempty] == -1)).all()
    # key_code: strictly increasing over the distinct keys
    ks, first = np.unique(key.ravel(), return_index=True)
    kc = u[10].ravel()[first]
    if name == "inf+denormal":
        assert ks.size == 12 and np.isinf(ks[0]) and np.isinf(ks[-1])
    elif name in ("random", "few", "empties", "negative"):
        assert ks.size > 1000
    assert (ks[1:] > ks[:-1]).all() and (kc[1:] > kc[:-1]).all() and kc[0] > 0, "key_code is not strictly increasing"
    assert (u[10] == key_code(key)).all()
    nv, cut = cs["nv"], cs["cut"]
    last = np.take_along_axis(key, np.maximum(nv - 1, 0)[:, None].astype(np.int64), 1)[:, 0]
    with np.errstate(all="ignore"):
        t = np.where((cut != 0) & (nv > 0), (last - 5e-5).astype(np.float32), F(-np.inf)).astype(np.float32)
    assert (v[12] == t.view(np.int32)[:, None]).all(), "list_thr_bits"
    assert ((cut != 0) & (nv == 0)).any() and ((cut != 0) & (nv == 64)).any() and ((cut == 0) & (nv > 0)).any()


def list_cases(seed, n):
    """n sequences of LIST_STEPS (key, idx) entries ([steps][n]): distinct idx within a sequence, a third of the
    sequences with tied keys, some entries skipped (kNoIdx), some sequences shorter than KC or empty"""
    rng = np.random.default_rng(seed)
    S = LIST_STEPS
    idx = (np.argsort(rng.random((n, 64)), axis=1)[:, :S] * 1009 + rng.integers(0, 1000, (n, 1))).astype(np.int32).T
    key = rng.uniform(-2.0, 10.0, (S, n))
    few = rng.uniform(0.0, 10.0, (3, n))
    key = np.where((np.arange(n) % 3 == 1)[None, :], np.take_along_axis(few, rng.integers(0, 3, (S, n)), axis=0), key)
    key = np.where(rng.random((S, n)) < 0.02, -np.inf, key)
    keep = rng.integers(0, S + 1, n)
    keep = np.where(np.arange(n) % 4 == 0, keep, S)
    skip = (rng.random((S, n)) < 0.1) | (np.argsort(rng.random((S, n)), axis=0) >= keep[None, :])
    idx = np.where(skip, NO_IDX, idx).astype(np.int32)
    return dict(n=n, key=np.ascontiguousarray(key), idx=np.ascontiguousarray(idx))


def list_statement(ls):
    """list_insert_ordered restated: one pass per entry, the entry sinking to its place"""
    n, key, idx = ls["n"], ls["key"], ls["idx"]
    ok, oi = np.zeros((30, n)), np.zeros((30, n), np.int32)
    for kc, row0 in zip(KCS, LIST_ROW0):
        k = np.full((kc, n), -np.inf)
        x = np.full((kc, n), NO_IDX, np.int32)
        for j in range(key.shape[0]):
            ck, ci, live = key[j].copy(), idx[j].copy(), idx[j] != NO_IDX
            moved = np.zeros(n, bool)
            for q in range(kc):
                sw = live & (moved | _better(ck, ci, k[q], x[q]))
                moved = sw
                tk, ti = k[q].copy(), x[q].copy()
                k[q], x[q] = np.where(sw, ck, tk), np.where(sw, ci, ti)
                ck, ci = np.where(sw, tk, ck), np.where(sw, ti, ci)
        ok[row0:row0 + kc], oi[row0:row0 + kc] = k, x
    return dict(key=ok, idx=oi)


def check_list(ls, out):
    """every list is the top KC of its sequence by (key desc, idx asc), (-inf, kNoIdx) where it is shorter"""
    key = np.where(ls["idx"] == NO_IDX, -np.inf, ls["key"]).T
    idx = ls["idx"].T
    o = np.lexsort((idx, -key), axis=-1)
    sk, si = np.take_along_axis(key, o, 1).T, np.take_along_axis(idx, o, 1).T
    nvalid = (idx != NO_IDX).sum(axis=1)
    assert (nvalid == 0).any() and (nvalid < 16).any() and (nvalid == LIST_STEPS).any()
    for kc, row0 in zip(KCS, LIST_ROW0):
        bad = ((bits64(out["key"][row0:row0 + kc]) != bits64(sk[:kc])) | (out["idx"][row0:row0 + kc] != si[:kc])).any(axis=0)
        assert not bad.any(), f"list_insert_ordered<{kc}>: {bad.sum()} sequences differ, e.g. {np.nonzero(bad)[0][:4]}"


# ---- the score role's slot helpers (ksched_pipe.h: bound_slots, sort_desc_u32, topk_merge_u32) ----------------------
SLOT_STEPS = 6
SLOT_ROWS = 4   # rows per step of the screened scan (k_pipe's kSPU)
SLOT_KCS = ((4, 0), (8, 20))  # (KC, first output row): bound_slots' maximum form, its insertion form


def slot_cases(seed, n):
    """x [2][steps][4][n]: lower bounds as pass 1 makes them (f32 bit patterns, 0 = no bound), a third of the elements
    with few distinct values, a third mostly without a bound"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.9, 11.0, (2, SLOT_STEPS, SLOT_ROWS, n)).astype(np.float32).view(np.uint32)
    few = rng.uniform(0.9, 11.0, (3, n)).astype(np.float32).view(np.uint32)
    pick = rng.integers(0, 3, x.shape)
    x = np.where(np.arange(n) % 3 == 1, np.take_along_axis(few[None, None], pick.reshape(1, 1, -1, n), axis=2).reshape(x.shape), x)
    x = np.where((np.arange(n) % 3 == 2) & (rng.random(x.shape) < 0.85), np.uint32(0), x)
    x = np.where(rng.random(x.shape) < 0.1, np.uint32(0), x)
    x[..., 0] = 0                      # no bound at all
    x[..., 1] = np.uint32(0xFFFFFFFF)  # the extremes of the unsigned compare
    x[:, :, :, 2] = np.arange(1, 2 * SLOT_STEPS * SLOT_ROWS + 1, dtype=np.uint32).reshape(2, SLOT_STEPS, SLOT_ROWS) << 7
    return dict(n=n, x=np.ascontiguousarray(x.astype(np.uint32)))


def slots_statement(sc):
    """bound_slots (both forms), sort_desc_u32 and topk_merge_u32 restated"""
    n, x = sc["n"], sc["x"]
    out = np.zeros((60, n), np.uint32)
    for kc, row0 in SLOT_KCS:
        ts = []
        for h in range(2):
            t = np.zeros((kc, n), np.uint32)
            for j in range(SLOT_STEPS):
                for uu in range(SLOT_ROWS):
                    if SLOT_ROWS % kc == 0:
                        t[uu % kc] = np.maximum(t[uu % kc], x[h, j, uu])
                    else:
                        xv = x[h, j, uu].copy()
                        for q in range(kc):
                            hi, lo = np.maximum(t[q], xv), np.minimum(t[q], xv)
                            t[q], xv = hi, lo
            out[row0 + h * kc:row0 + (h + 1) * kc] = t
            t = t.copy()
            for i in range(1, kc):
                for j in range(i, 0, -1):
                    a, c = t[j - 1].copy(), t[j].copy()
                    t[j - 1], t[j] = np.maximum(a, c), np.minimum(a, c)
            out[row0 + (2 + h) * kc:row0 + (3 + h) * kc] = t
            ts.append(t)
        v = np.maximum(ts[0], ts[1][::-1])
        d = kc // 2
        while d >= 1:
            for i in range(kc):
                if (i & d) == 0:
                    a, b = v[i].copy(), v[i + d].copy()
                    v[i], v[i + d] = np.maximum(a, b), np.minimum(a, b)
            d >>= 1
        out[row0 + 4 * kc:row0 + 5 * kc] = v
    return out


def check_slots(sc, out):
    """bound_slots in both forms: every slot is one of its set's inputs (or the initial 0) and the KC-th largest slot is
    at most the KC-th largest input -- the maximum form keeps each slot's rows' maximum, the insertion form the KC
    largest inputs; sort_desc_u32 and topk_merge_u32 against a plain sort"""
    n, x = sc["n"], sc["x"]
    desc = lambda a: np.sort(a, axis=0)[::-1]  # noqa: E731
    for kc, row0 in SLOT_KCS:
        srt = []
        for h in range(2):
            inp = x[h].reshape(-1, n)
            t = out[row0 + h * kc:row0 + (h + 1) * kc]
            isin = (t[:, None, :] == inp[None, :, :]).any(axis=1) | (t == 0)
            assert isin.all(), f"bound_slots<{kc}>: a slot is none of the inputs"
            assert (t.min(axis=0) <= desc(inp)[kc - 1]).all(), f"bound_slots<{kc}>: the KC-th slot exceeds the KC-th input"
            if SLOT_ROWS % kc == 0:
                want = np.stack([x[h][:, [u for u in range(SLOT_ROWS) if u % kc == q]].reshape(-1, n).max(axis=0) for q in range(kc)])
                assert (t == want).all(), f"bound_slots<{kc}> (maximum form)"
            else:
                assert (t == desc(inp)[:kc]).all(), f"bound_slots<{kc}> (insertion form)"
            s = out[row0 + (2 + h) * kc:row0 + (3 + h) * kc]
            assert (s == desc(t)).all(), f"sort_desc_u32<{kc}>"
            srt.append(s)
        m = out[row0 + 4 * kc:row0 + 5 * kc]
        assert (m == desc(np.concatenate(srt))[:kc]).all(), f"topk_merge_u32<{kc}>"
    assert (out[:, 0] == 0).all() and (out[[0, 20], 1] == 0xFFFFFFFF).all()
