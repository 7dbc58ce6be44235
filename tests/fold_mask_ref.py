"""The screened commit's two folds over a round's guessed columns (csrc/ksched_commit.h commit_spc_batch, wave 0, lane =
pod), in numpy, each in its plain form -- every wave's partial best, every column of [c, f) -- and in its masked form,
which reads only the waves and columns that step 2 marked (SpcSmem::fm):

  t* fold       t* = best of the confirmed best (rbk, rbi, rbs) and the waves' partial bests, waves in ascending order.
                A wave's partial best is -inf in every lane unless it keyed a column exactly; a wave that keyed none
                writes no partials (its rows keep garbage) and sets no bit.
  confirm fold  for the confirmed columns k of [c, f) in ascending order: fcc += D[k], and the column's key S[:, k]
                takes over the confirmed best where it is better(); rb2, the f32 upper bound of every key that is not
                the best, rises.  A column is marked when some pod needed its exact key or it changed the predicate of
                a pod after its own.

better() is the commit's: key descending, node index ascending; -inf never wins (the folds test for it), NaN -- a
skipped column's kSkipKey -- never wins and never raises rb2.  Column k is pod k's guess; only pods after k use it.
"""
import numpy as np

NEG_INF = -np.inf
NO_IDX = np.int32(0x7fffffff)
LANES = 64


def better(ka, ia, kb, ib):
    with np.errstate(invalid="ignore"):
        return (ka > kb) | ((ka == kb) & (ia < ib))


def f32_ru(x):
    """RU_f32 of the f64 values x (__double2float_ru); NaN stays NaN"""
    y = x.astype(np.float32)
    low = y.astype(np.float64) < x
    return np.where(low, np.nextafter(y, np.float32(np.inf)), y).astype(np.float32)


def column_wave(k, c, waves):
    return (k - c) % waves


def step2(S, gn, gs, keyed, c, cend, waves):
    """the waves' partial bests over their keyed columns (lanes after the column's pod only), and the two masks a
    correct step 2 leaves: the waves that keyed a column, the columns the confirm fold has to visit (without D's part)"""
    pk = np.full((waves, LANES), NEG_INF)
    pi = np.full((waves, LANES), NO_IDX, np.int32)
    ps = np.full((waves, LANES), -1, np.int32)
    wmask = 0
    lane = np.arange(LANES)
    for k in range(c, cend):
        if gn[k] < 0 or not keyed[k]:
            continue
        w = column_wave(k, c, waves)
        wmask |= 1 << w
        v = S[:, k]
        up = (lane > k) & (v != NEG_INF) & better(v, gn[k], pk[w], pi[w])
        pk[w] = np.where(up, v, pk[w])
        pi[w] = np.where(up, gn[k], pi[w])
        ps[w] = np.where(up, gs[k], ps[w])
    return pk, pi, ps, wmask


def column_mask(gn, keyed, D, c, cend):
    """bit k: column k was keyed exactly, or changed the predicate of a pod after k"""
    m = 0
    for k in range(c, cend):
        if gn[k] >= 0 and (keyed[k] or (D[k, k + 1:] != 0).any()):
            m |= 1 << k
    return m


def tstar_fold(rbk, rbi, rbs, pk, pi, ps, wmask=None):
    """wmask None: every wave; else the set waves, lowest first"""
    tk, ti, ts = rbk.copy(), rbi.copy(), rbs.copy()
    waves = pk.shape[0]
    for w in range(waves):
        if wmask is not None and not (wmask >> w) & 1:
            continue
        up = (pk[w] != NEG_INF) & better(pk[w], pi[w], tk, ti)
        tk = np.where(up, pk[w], tk)
        ti = np.where(up, pi[w], ti)
        ts = np.where(up, ps[w], ts)
    return tk, ti, ts


def confirm_fold(rbk, rbi, rbs, fcc, rb2, S, D, gn, gs, c, f, cmask=None):
    """cmask None: every column of [c, f); else its set bits inside [c, f), lowest first.  rb2 None: not tracked."""
    rbk, rbi, rbs, fcc = rbk.copy(), rbi.copy(), rbs.copy(), fcc.copy()
    b2 = None if rb2 is None else rb2.copy()
    visited = 0
    for k in range(c, f):
        if cmask is not None and not (cmask >> k) & 1:
            continue
        if gn[k] < 0:
            continue
        visited += 1
        v = S[:, k]
        fcc = fcc + D[k].astype(np.int32)
        up = (v != NEG_INF) & better(v, gn[k], rbk, rbi)
        if b2 is not None:
            o = np.where(up, rbk, v)
            with np.errstate(invalid="ignore"):
                b2 = np.where(o > b2.astype(np.float64), f32_ru(o), b2).astype(np.float32)
        rbk = np.where(up, v, rbk)
        rbi = np.where(up, gn[k], rbi)
        rbs = np.where(up, gs[k], rbs)
    return rbk, rbi, rbs, fcc, b2, visited
