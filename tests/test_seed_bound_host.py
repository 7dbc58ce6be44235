"""The seeded score scan, stated in numpy (tests/seed_ref.py), is sound for ANY seed mask: every pair of a pod's exact
top-KC list (f64 keys in the reference's operation order, ties by row) is in the needed set.  Checked on random,
adversarial and c4-like workgroups, for the all-node and the feasible domain, with these seed masks: empty, full,
random, the previous batch's needed rows (after placements changed the state), and masks with fewer than KC usable
rows."""
import numpy as np
import pytest

from seed_ref import exact_topk, seeded_scan

KC = 4


def random_wg(rng, rows=240, pods=64):
    ac = rng.integers(500, 64000, rows)
    am = rng.integers(1 << 18, 1 << 26, rows)
    ap = rng.integers(1, 110, rows)
    rc = rng.integers(0, 4000, pods)
    rm = rng.integers(0, 1 << 22, pods)
    rp = rng.integers(0, 3, pods)
    return rc, rm, rp, ac, am, ap


def adversarial_wg(rng, rows=240, pods=64):
    """NaN rows (zero, negative and >= 2^52 allocatables), fractions at 1 and 1 +- 2^-20, pods that fit nowhere, runs of
    identical rows (ties)."""
    rc, rm, rp, ac, am, ap = random_wg(rng, rows, pods)
    ac[0:6] = [0, 1 << 52, (1 << 52) + 5, -3, 0, 1 << 60]
    am[4:8] = [0, 1 << 52, 0, 1 << 53]
    ap[8:10] = 0
    ac[10:40] = 16000; am[10:40] = 32 << 20; ap[10:40] = 110       # ties
    rc[0:8] = 16000; rm[0:8] = 1 << 20; rp[0:8] = 1                 # fraction exactly 1 on the tied rows
    ac[40:44] = [1 << 20, (1 << 20) + 1, (1 << 20) - 1, 1 << 21]
    rc[8:12] = 1 << 20                                              # fractions at 1, 1 -+ 2^-20, 1/2
    rc[12:20] = 10 ** 6                                             # fits nowhere (cpu)
    rp[20:24] = 500                                                 # fits nowhere (pods)
    rc[24:26] = -1; rm[26:28] = 1 << 52                             # unscreenable requests
    return rc, rm, rp, ac, am, ap


def c4_like_wg(rng, rows=430, pods=64, used=0.0):
    """cpu millicores, memory KiB, pod counts; `used` of the capacity already taken."""
    cap_c = rng.choice([4000, 8000, 16000, 32000, 64000], rows)
    cap_m = rng.choice([8, 16, 32, 64, 128], rows).astype(np.int64) << 20
    ac = (cap_c * (1 - used * rng.random(rows))).astype(np.int64)
    am = (cap_m * (1 - used * rng.random(rows))).astype(np.int64)
    ap = (110 * (1 - used * rng.random(rows))).astype(np.int64)
    rc = rng.choice([100, 250, 500, 1000, 2000, 4000], pods)
    rm = rng.choice([128, 256, 512, 1024, 4096], pods).astype(np.int64) << 10
    rp = np.ones(pods, np.int64)
    return rc, rm, rp, ac, am, ap


def seed_masks(rng, wg, dom_all):
    rc, rm, rp, ac, am, ap = wg
    rows = len(ac)
    yield "empty", np.zeros(rows, bool)
    yield "full", np.ones(rows, bool)
    yield "random", rng.random(rows) < 0.1
    few = np.zeros(rows, bool)
    few[rng.choice(rows, KC - 1, replace=False)] = True
    yield "fewer_than_kc", few
    nan_only = np.zeros(rows, bool)
    nan_only[:10] = True  # (the adversarial workgroup's unscreenable rows)
    yield "first_rows", nan_only
    # the previous batch's needed rows: other pods, on the state before placements took the best rows' resources
    prc, prm, prp = rng.permutation(rc), rng.permutation(rm), rng.permutation(rp)
    need, _ = seeded_scan(prc, prm, prp, ac, am, ap, np.ones(rows, bool), KC, dom_all=dom_all)
    yield "previous_batch", need.any(axis=1)


def check(wg, rng, dom_all, active=None):
    rc, rm, rp, ac, am, ap = wg
    top = exact_topk(rc, rm, rp, ac, am, ap, KC, dom_all)
    for name, seed in seed_masks(rng, wg, dom_all):
        if name == "previous_batch":
            # placements between the batches: the seed rows lose resources (some go non-fitting)
            ac, am, ap = ac.copy(), am.copy(), ap.copy()
            hit = np.nonzero(seed)[0][::2]
            ac[hit] -= np.minimum(ac[hit], 3000); am[hit] //= 2; ap[hit] = np.maximum(ap[hit] - 2, 0)
            top = exact_topk(rc, rm, rp, ac, am, ap, KC, dom_all)
        need, L = seeded_scan(rc, rm, rp, ac, am, ap, seed, KC, active=active, dom_all=dom_all)
        usable = int(seed.sum())
        if usable < KC:
            assert not L.any(), f"{name}: fewer than KC seed rows must give L = 0"
        for p in range(len(rc)):
            if active is not None and not active[p]:
                assert not need[:, p].any(), f"{name}: inactive pod {p} needs rows"
                continue
            miss = [r for r in top[p] if not need[r, p]]
            assert not miss, f"{name} dom_all={dom_all}: pod {p} top-KC rows {miss} are not needed (L {L[p]})"


@pytest.mark.parametrize("dom_all", [True, False], ids=["all_nodes", "feasible"])
@pytest.mark.parametrize("seed", range(3))
def test_random_workgroups(seed, dom_all):
    rng = np.random.default_rng(100 + seed)
    check(random_wg(rng), rng, dom_all)


@pytest.mark.parametrize("dom_all", [True, False], ids=["all_nodes", "feasible"])
@pytest.mark.parametrize("seed", range(3))
def test_adversarial_workgroups(seed, dom_all):
    rng = np.random.default_rng(200 + seed)
    check(adversarial_wg(rng), rng, dom_all)


@pytest.mark.parametrize("used", [0.0, 0.6, 0.98], ids=["fresh", "mid", "late"])
def test_c4_like_workgroups(used):
    rng = np.random.default_rng(300)
    check(c4_like_wg(rng, used=used), rng, True)


def test_inactive_lanes_need_nothing():
    rng = np.random.default_rng(400)
    active = np.arange(64) < 40
    check(adversarial_wg(rng), rng, True, active=active)


def test_weaker_seeds_only_add_pairs():
    """A subset of the seed rows never gives a larger L, so never a smaller needed set."""
    rng = np.random.default_rng(500)
    rc, rm, rp, ac, am, ap = c4_like_wg(rng, used=0.5)
    full = np.ones(len(ac), bool)
    sub = rng.random(len(ac)) < 0.2
    nf, Lf = seeded_scan(rc, rm, rp, ac, am, ap, full, KC)
    ns, Ls = seeded_scan(rc, rm, rp, ac, am, ap, sub, KC)
    assert (Ls <= Lf).all() and (ns | ~nf).all()
