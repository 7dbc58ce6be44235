"""The screened commit's fold masks (csrc/ksched_commit.h SpcSmem::fm: the waves whose partial bests the check and the
wave-0 state read, the guessed columns the confirm fold visits) on the small conflict shapes of
test_gpu_commit_conflict.py -- c4 1000 x 4000, c3 200 x 2000, c5hc 2000 x 3000 at K16 / B64, and c3 at K4 / B32 with
chunk lists of 4 for short batches and short lists -- each with the masks on and with KSCHED_NO_FOLD_MASK=1: bit-exact
against the CPU oracle (node index, score bits, feasible count, final state), the commit's decision counters
(KSCHED_COMMIT_STAMPS words 12-14, 16-21, 31) equal both ways, and the masks' own counters (words 32-37) show that the
folds both read and skipped.  A wave that keyed nothing leaves its partial rows as own[] filled them, so a wrong wave
bit reads table garbage, not -inf, and the oracle comparison sees it.

Words: [32] checks that read no wave's partials, [33] partial rows read over all checks, [34] batches whose wave-0 state
read none, [35] confirm-fold columns visited, [36] skipped, [37] batches in which a check read none after an earlier
check of the batch had read some (the rows then still hold that round's bests).

Counts with the masks on -- {checks that read none of rounds, rows read, wave-0 states that read none of batches, fold
columns visited / skipped, batches with a later empty round}:
  c4        1000 x 4000: 127 of 309,  761,  67 of  92,  657 / 2425, 59
  c3         200 x 2000:  48 of 226,  670,  71 of  73,  877 /  471, 32
  c5hc      2000 x 3000:  10 of 570, 3164,  31 of  63,  807 /    0,  9
  c3 K4/B32  200 x 2000: 147 of 285,  258, 113 of 117,  669 /  724, 53
and with KSCHED_NO_FOLD_MASK=1 12 rows in every check (c4 3708 = 12 x 309) and every column visited (c4 3082).
"""
import ctypes as C

import pytest

from test_gpu_commit_conflict import case
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

K16 = dict(topk=16, batch=64)
RUNS = {"c4": ("c4", K16), "c3": ("c3", K16), "c5hc": ("c5hc", K16), "c3_k4_b32": ("c3", dict(topk=4, batch=32, chunk_topk=4))}
DECISIONS = (12, 13, 14, 16, 17, 18, 19, 20, 21, 31)
WAVES = 12  # the persistent commit workgroup's
WORDS = {}


def run(monkeypatch, rid, masks):
    """the run's 48 counter words; computed once per (shape, masks) and checked against the oracle there"""
    if (rid, masks) in WORDS:
        return WORDS[rid, masks]
    from ksched import MODE_BATCHED, Engine, _lib as L
    name, kw = RUNS[rid]
    cl, want = case(name)
    monkeypatch.setenv("KSCHED_COMMIT_STAMPS", "1")
    if masks:
        monkeypatch.delenv("KSCHED_NO_FOLD_MASK", raising=False)
    else:
        monkeypatch.setenv("KSCHED_NO_FOLD_MASK", "1")
    w = (C.c_int64 * 48)()
    with Engine(mode=MODE_BATCHED, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, **kw) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
        oi, os_, of = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        got = (oi, os_, of, e.read_nodes(), e.stats())
        L.check(L.lib().ksched_get_commit_stamps(e._ctx, 48, w), e._ctx, "get_commit_stamps")
    assert_same(got, want, f"{rid}/{'masks' if masks else 'no_fold_mask'}")
    assert got[4]["pipeline"] == "persistent", got[4]
    w = [int(x) for x in w]
    print(f"{rid}/{'masks' if masks else 'no_fold_mask'}: rounds {w[12]} batches {w[14]} guessed columns {w[18]} keyed {w[19]} | "
          f"checks that read none {w[32]}, rows read {w[33]}, wave-0 states that read none {w[34]}, "
          f"fold columns visited {w[35]} skipped {w[36]}, batches with a later empty round {w[37]}")
    WORDS[rid, masks] = w
    return w


@pytest.mark.parametrize("rid", list(RUNS))
def test_masks_on(gpu_available, oracle_mod, monkeypatch, rid):
    w = run(monkeypatch, rid, True)
    assert 0 <= w[32] <= w[12] and 0 <= w[34] <= w[14], w
    assert 0 <= w[33] <= WAVES * (w[12] - w[32]), w   # no row read in a check that read none
    assert w[33] >= w[12] - w[32], w                  # and at least one in every other
    assert w[35] >= 0 and w[36] >= 0 and w[35] + w[36] <= w[18], w  # confirmed guessed columns, each visited or skipped
    off = run(monkeypatch, rid, False)  # (shared with the test below; run here when this test is selected alone)
    assert w[35] + w[36] == off[35], (w, off)  # exactly the columns the unmasked fold visits


@pytest.mark.parametrize("rid", list(RUNS))
def test_masks_off_same_decisions(gpu_available, oracle_mod, monkeypatch, rid):
    off = run(monkeypatch, rid, False)
    on = run(monkeypatch, rid, True)
    assert [off[i] for i in DECISIONS] == [on[i] for i in DECISIONS], (off, on)
    assert off[33] == WAVES * off[12] and off[32] == 0 and off[34] == 0, off  # every wave's row in every check
    assert off[36] == 0 and off[37] == 0, off                                  # no column skipped
    assert off[35] == on[35] + on[36], (off, on)                               # the masks only split the same columns


def test_every_path_runs(gpu_available, oracle_mod, monkeypatch):
    """over the shapes together the masked folds read and skip: checks and wave-0 states with and without partials,
    fold columns visited and skipped; c5hc, which keys about half its columns, is the mostly-full case; and in some
    batch a round keys nothing after an earlier round keyed a column"""
    ws = {rid: run(monkeypatch, rid, True) for rid in RUNS}
    tot = lambda i: sum(w[i] for w in ws.values())
    assert tot(32) > 0 and tot(12) - tot(32) > 0, ws   # checks that read nothing / something
    assert tot(34) > 0 and tot(14) - tot(34) > 0, ws   # wave-0 states
    assert tot(35) > 0 and tot(36) > 0, ws             # fold columns visited / skipped
    c5 = ws["c5hc"]
    assert 2 * (c5[12] - c5[32]) > c5[12], c5          # most of its checks read partials
    assert tot(37) > 0, ws                             # stale partial rows behind an empty mask
