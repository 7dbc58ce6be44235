"""The persistent commit's touched-node columns (csrc/ksched_commit.h touch_column: the inherited entries of
export(b - 1), the guessed columns of every round, the columns of the one-by-one step) on the three small conflict
shapes of test_gpu_commit_conflict.py at K16 / B64, with the screen on and off (KSCHED_NO_TOUCH_SCREEN=1): bit-exact
against the CPU oracle (node index, score bits, feasible count, final state), and the commit's own counts
(KSCHED_COMMIT_STAMPS words 16-21: columns per wave, of them keyed exactly) show that every class ran both its
skipped and its keyed path.

Counts on the parent build (143d778), screen on -- {inherited, keyed, guessed, keyed, one-by-one, keyed}:
  c4   1000 x 4000: 1534 / 224, 6734 / 1012, 386 / 113; 307 rounds, 270 failed guesses, 91 batches
  c5hc 2000 x 3000: 1140 / 1140, 5891 / 5724, 2157 / 2115; 558 rounds, 530 failed guesses, 62 batches
  c3    200 x 2000:   62 / 7, 3690 / 800, 277 / 131; 224 rounds, 216 failed guesses, 71 batches
so every class skips and keys on c4 and on c3 alone.  With the screen off every inherited entry is keyed; a guessed or
one-by-one column is still skipped where no pod follows its own in the batch (c4: 6597 of 6734, 383 of 386).  c3 is
here also for its pods that fit nowhere (347: each is a column with gn < 0 in its round, skipped wave-uniformly) and
its short last batch (2000 = 31 * 64 + 16).  The counts are decisions of the commit, not timings: a change that takes
no decision leaves the column counts (words 16, 18, 20) as they are.
"""
import ctypes as C

import pytest

from test_gpu_commit_conflict import case
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

NAMES = ("c4", "c5hc", "c3")
COUNTS = {}


def run_counted(name, label):
    from ksched import MODE_BATCHED, Engine, _lib as L
    cl, want = case(name)
    w = (C.c_int64 * 32)()
    with Engine(mode=MODE_BATCHED, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, topk=16, batch=64) as e:
        e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
        oi, os_, of = e.schedule(cl.req_cpu, cl.req_mem, cl.req_pods, cl.selector)
        got = (oi, os_, of, e.read_nodes(), e.stats())
        L.check(L.lib().ksched_get_commit_stamps(e._ctx, 32, w), e._ctx, "get_commit_stamps")
    assert_same(got, want, f"{name}/{label}")
    assert got[4]["pipeline"] == "persistent", got[4]
    cnt = [int(w[i]) for i in range(16, 22)] + [int(w[12]), int(w[14])]  # ... + rounds, batches
    print(f"{name}/{label}: inherited {cnt[0]} keyed {cnt[1]}, guessed {cnt[2]} keyed {cnt[3]}, "
          f"one-by-one {cnt[4]} keyed {cnt[5]}; rounds {int(w[12])} failed guesses {int(w[13])} batches {int(w[14])}")
    return cnt


@pytest.mark.parametrize("name", NAMES)
def test_columns_screened(gpu_available, oracle_mod, monkeypatch, name):
    monkeypatch.setenv("KSCHED_COMMIT_STAMPS", "1")
    cnt = run_counted(name, "screen")
    COUNTS[name] = cnt
    for cls in range(3):
        assert 0 <= cnt[2 * cls + 1] <= cnt[2 * cls], cnt


@pytest.mark.parametrize("name", NAMES)
def test_columns_unscreened(gpu_available, oracle_mod, monkeypatch, name):
    monkeypatch.setenv("KSCHED_COMMIT_STAMPS", "1")
    monkeypatch.setenv("KSCHED_NO_TOUCH_SCREEN", "1")
    cnt = run_counted(name, "no_touch_screen")
    assert cnt[1] == cnt[0] > 0, cnt  # every inherited entry keyed exactly
    # a guessed or one-by-one column is keyed unless no pod follows its own, the batch's last pod: at most one such
    # column per round, one such step per batch
    assert 0 <= cnt[2] - cnt[3] <= cnt[6] and cnt[3] > 0, cnt
    assert 0 <= cnt[4] - cnt[5] <= cnt[7] and cnt[5] > 0, cnt
    if name in COUNTS:  # the screen only ever removes exact keys
        assert all(cnt[i] >= COUNTS[name][i] for i in (1, 3, 5)), (cnt, COUNTS[name])
        assert all(cnt[i] == COUNTS[name][i] for i in (0, 2, 4)), (cnt, COUNTS[name])


def test_every_class_skips_and_keys(gpu_available, oracle_mod, monkeypatch):
    """over the shapes together: inherited entries, guessed columns and one-by-one columns each with skipped and with
    exactly keyed columns; c3 with its columns of gn < 0 and its short last batch"""
    monkeypatch.setenv("KSCHED_COMMIT_STAMPS", "1")
    for name in NAMES:
        if name not in COUNTS:
            COUNTS[name] = run_counted(name, "screen")
    for cls, what in enumerate(("inherited entries", "guessed columns", "one-by-one columns")):
        cols = sum(COUNTS[n][2 * cls] for n in NAMES)
        keyed = sum(COUNTS[n][2 * cls + 1] for n in NAMES)
        assert keyed > 0, f"{what}: none keyed exactly {COUNTS}"
        assert cols - keyed > 0, f"{what}: none skipped {COUNTS}"
    cl, want = case("c3")
    assert int((want[0] < 0).sum()) > 0       # pods that fit nowhere: gn = -2 in their round
    assert cl.req_cpu.shape[0] % 64 == 16     # a short last batch
    assert COUNTS["c3"][2] > 0                # beside columns that were guessed
