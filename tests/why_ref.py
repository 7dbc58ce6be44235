"""Shared by the ksched_schedule_full_why tests: the CPU restatement of "the reasons a pod that fits nowhere saw at its
turn", built on full_ref and dryrun_ref as they are.  The identity: the state pod i saw is the end state of
full_ref.schedule_full on the pods [0, i) with these gangs -- the closed gangs before i's gang keep their offsets and
minima; the earlier members of i's own, still open, gang become gangs of one, so their commits stand (a gang of one that
finds a node is accepted): that is "tentative".  The codes are then dryrun_ref.codes(c, i, dryrun_ref.after(that
result)), the waiver decided from that state's any words as dryrun_ref derives them.  Every NO_FIT pod of the full
reference must have no node with code 0 under the identity; why() asserts it, pod by pod.

at_gang_start: a deliberately WRONG variant -- the codes against the state at the START of the pod's gang, which forgets
the tentative commits.  at_end: the codes against the call's end state, which is what ksched_explain_full answers
afterwards.  The tests use both on the CPU only, to prove that a case can tell "at its turn" from either."""
import dataclasses

import numpy as np

import dryrun_ref as DR
import full_ref as FR

NUM_REASONS_FULL = DR.NUM_REASONS_FULL


def _prefix(c, i, tentative):
    """Pods [0, i) of case c with the gangs the identity names (tentative) or with i's own gang cut away (not)."""
    if c.gang_off is None:
        return dataclasses.replace(FR.pods(c, 0, i), gang_off=None, gang_min=None)
    off = np.asarray(c.gang_off, np.int64)
    g = int(np.searchsorted(off, i, side="right")) - 1  # i's gang: off[g] <= i < off[g + 1]
    lo = int(off[g])
    hi = i if tentative else lo
    new_off = np.concatenate([off[:g + 1], np.arange(lo + 1, hi + 1, dtype=np.int64)])
    gmin = None
    if c.gang_min is not None:
        gmin = np.concatenate([np.asarray(c.gang_min, np.int32)[:g], np.ones(hi - lo, np.int32)])
    return dataclasses.replace(FR.pods(c, 0, hi), gang_off=new_off, gang_min=gmin)


def state_before(O, c, i, tentative=True):
    """The rows and tables pod i saw (dryrun_ref.Tables); tentative=False: those at the start of its gang."""
    sub = _prefix(c, i, tentative)
    if sub.cl.n_pods == 0:
        return DR.initial(c)
    return DR.after(FR.schedule_full(O, sub))


def why(O, c, ref, limit=None):
    """ref: full_ref.schedule_full(O, c).  Returns (pods int32[r], counts int64[r, 14], reasons uint8[r, n], nofit) for
    the first `limit` (None: all) NO_FIT pods of the call, in pod order; nofit is their total."""
    nf = np.flatnonzero(ref[0] == -1)
    take = nf if limit is None else nf[:limit]
    n = c.cl.n_nodes
    reasons = np.zeros((len(take), n), np.uint8)
    counts = np.zeros((len(take), NUM_REASONS_FULL), np.int64)
    for r, i in enumerate(take):
        reasons[r], _ = DR.codes(c, int(i), state_before(O, c, int(i)))
        counts[r] = np.bincount(reasons[r], minlength=NUM_REASONS_FULL)
        assert counts[r, 0] == 0 and ref[2][i] == 0, (int(i), counts[r].tolist())  # the identity: NO_FIT saw no eligible node
    return take.astype(np.int32), counts, reasons, int(len(nf))


def at_gang_start(O, c, pods):
    """The wrong variant: per-node codes of the given pods against the state at the start of each pod's gang."""
    return np.stack([DR.codes(c, int(i), state_before(O, c, int(i), tentative=False))[0] for i in pods]) \
        if len(pods) else np.zeros((0, c.cl.n_nodes), np.uint8)


def at_end(c, ref, pods):
    """What a dry run after the call says: per-node codes of the given pods against the end state."""
    t = DR.after(ref)
    return np.stack([DR.codes(c, int(i), t)[0] for i in pods]) if len(pods) else np.zeros((0, c.cl.n_nodes), np.uint8)


def same(got, want, node_rows=None):
    """got: Engine.schedule_full_why(...)[4] (trimmed); want: why() above with the same limit.  node_rows: the per-node
    rows the call asked for (None: as many as it recorded).  nofit, the pod list, all 14 columns of every row and every
    byte of the per-node rows, exactly."""
    gp, gc, gr, gn = got
    wp, wc, wr, wn = want
    assert gn == wn, ("nofit", gn, wn)
    assert gp.dtype == np.int32 and gp.tolist() == wp.tolist(), ("pods", gp.tolist(), wp.tolist())
    assert gc.dtype == np.int64 and gc.shape == wc.shape, (gc.shape, wc.shape)
    bad = np.argwhere(gc != wc)
    assert bad.size == 0, f"counts: first difference at row {bad[0].tolist()} (pod {wp[bad[0][0]]}): got {gc[bad[0][0]].tolist()}, want {wc[bad[0][0]].tolist()}"
    rows = len(wp) if node_rows is None else min(node_rows, len(wp))
    if rows == 0 and gr is None:
        return
    assert gr is not None and gr.dtype == np.uint8 and gr.shape == (rows, wr.shape[1]), (None if gr is None else gr.shape, rows)
    bad = np.argwhere(gr != wr[:rows])
    assert bad.size == 0, f"reasons: first difference at {bad[0].tolist()} (pod {wp[bad[0][0]]}): got {gr[tuple(bad[0])]}, want {wr[tuple(bad[0])]}"
