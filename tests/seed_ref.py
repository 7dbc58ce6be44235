"""CPU statement of the seeded score scan (score_role in k8s-scheduler_amd/csrc/ksched_pipe.hip, KC <= 4 kernels): the
workgroup's bound L per pod from the seed rows alone, then one pass that tests every pair's f32 screen against L
(ksched_device.h screen_need).  Built on tests/screen_ref.py's bit-exact f32 statements; one score workgroup, rows in
node order, all-node or feasible domain, no labels."""
import numpy as np

from screen_ref import EPS, F, exact_score, screen_fast

ONE_PLUS_EPS = F(1.0) + EPS   # the device's f32 constant 1.0f + kScreenEps
ONE_MINUS_EPS = F(1.0) - EPS


def screen_need(v, amb, el, L):
    """ksched_device.h screen_need: needed unless the screen proves the pair below L; an ambiguous pair always is."""
    with np.errstate(invalid="ignore"):
        below = (np.asarray(v, np.float32) + ONE_PLUS_EPS) < np.asarray(L, np.float32)
    return np.asarray(amb, bool) | (np.asarray(el, bool) & ~below)


def pair_grid(rc, rm, rp, ac, am, ap):
    """[rows][pods] grids of the six int64 inputs."""
    r = [np.broadcast_to(np.asarray(x, np.int64)[None, :], (len(ac), len(rc))) for x in (rc, rm, rp)]
    a = [np.broadcast_to(np.asarray(x, np.int64)[:, None], (len(ac), len(rc))) for x in (ac, am, ap)]
    return r + a


def seeded_scan(rc, rm, rp, ac, am, ap, seed, kc=4, active=None, dom_all=True):
    """(needed [rows][pods], L [pods]) of one batch: `seed` is the workgroup's seed-row mask [rows]."""
    g = pair_grid(rc, rm, rp, ac, am, ap)
    v, mx, amb, rf = screen_fast(*g)
    active = np.ones(len(rc), bool) if active is None else np.asarray(active, bool)
    el = np.ones_like(rf) if dom_all else rf
    with np.errstate(invalid="ignore"):
        lo_ok = ~(rf & (mx >= F(0.999))) & (v > EPS)
        x = np.where(np.asarray(seed, bool)[:, None] & active[None, :] & el & lo_ok & ~amb, v + ONE_MINUS_EPS, F(0)).astype(np.float32)
    # every bound is 0 ("none") or a positive float: the KC-th largest per pod, 0 with fewer than KC rows
    pad = np.zeros((kc, x.shape[1]), np.float32)
    L = -np.sort(-np.concatenate([x, pad]), axis=0)[kc - 1]
    need = screen_need(v, amb, el, L[None, :]) & active[None, :]
    return need, L


def exact_topk(rc, rm, rp, ac, am, ap, kc=4, dom_all=True):
    """[pods] lists of the rows of the exact top-KC (key desc, row asc) among the eligible pairs."""
    g = pair_grid(rc, rm, rp, ac, am, ap)
    key = exact_score(*g)
    fit = (g[3] >= g[0]) & (g[4] >= g[1]) & (g[5] >= g[2])
    el = np.ones_like(fit) if dom_all else fit
    out = []
    for p in range(key.shape[1]):
        rows = np.nonzero(el[:, p])[0]
        order = np.lexsort((rows, -key[rows, p]))
        out.append(rows[order[:kc]])
    return out


def bound_insert_top(x, kc=4):
    """ksched_pipe.h bound_insert<kc>, step by step: x [steps][n] u32 bounds into a sorted (descending) top-kc list."""
    x = np.asarray(x, np.uint32)
    t = np.zeros((kc, x.shape[1]), np.uint32)
    for xv in x:
        xv = xv.copy()
        for q in range(kc):
            hi = np.maximum(t[q], xv)
            xv = np.minimum(t[q], xv)
            t[q] = hi
    return t
