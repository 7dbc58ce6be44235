#!/usr/bin/env python3
"""Per-batch distributions of the persistent pipeline's phase stamps (KSCHED_TRACE_DUMP raw file: [cap][16]
u64: wall-clock stamps at 100 MHz and the commit's counters in column 16, the columns of print_persist_trace in ksched_diag.hip).  The stderr summary
gives means; a mean can hide a few long stalls, so this prints percentiles and the stalls.

  python tools/trace_dist.py gpurun_out/trace_c4.bin [lag=3]
"""
import sys

import numpy as np

COLS = 54


def main():
    t = np.fromfile(sys.argv[1], dtype=np.uint64).reshape(-1, COLS).astype(np.int64)
    lag = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    n = t.shape[0]
    b = np.arange(lag, n)
    ok = (t[b, 0] > 0) & (t[b, 1] > 0) & (t[b, 2] > 0) & (t[b, 3] > 0) & (t[b, 4] > 0) & (t[b - lag, 4] > 0)
    b = b[ok]
    us = lambda x: x * 0.01  # noqa: E731  100 MHz ticks -> us
    ph = {
        "to-score (commit(b-L) end -> WG0 score start)": t[b, 0] - t[b - lag, 4],
        "score (WG0 start -> last arrival)": t[b, 1] - t[b, 0],
        "merge (last arrival -> last merge)": t[b, 2] - t[b, 1],
        "to-commit (last merge -> commit past wait)": t[b, 3] - t[b, 2],
        "commit (past wait -> end)": t[b, 4] - t[b, 3],
        "commit gap (commit(b-1) end -> past wait)": t[b, 3] - t[b - 1, 4],
        "period (commit(b-1) end -> commit(b) end)": t[b, 4] - t[b - 1, 4],
        "wg0 score busy (start -> its arrival)": t[b, 5] - t[b, 0],
        "loop top -> past wait": t[b, 3] - t[b, 15],
    }
    if (t[b, 22] > 0).all():  # two commit workgroups: P1, the hand-off, the rest
        ph["P1: past merges' wait -> past the hand-off"] = t[b, 22] - t[b, 3]
        p1 = b[(t[b, 27] > 0) & (t[b, 30] > 0)]
        if len(p1) == len(b):  # P1's split: the lists loaded and hashed, the rest of P1, the hand-off itself
            ph["  past the wait -> lists hashed"] = t[b, 30] - t[b, 3]
            ph["  -> P1 done (key columns, thresholds)"] = t[b, 27] - t[b, 30]
            ph["  -> past the hand-off"] = t[b, 22] - t[b, 27]
            ei = t[b, 26] > 0
            print(f"inherited keys loaded before the merges' wait in {ei.sum()} of {len(b)} batches, "
                  f"{0.01 * (t[b, 3] - t[b, 26])[ei].mean() if ei.any() else 0:.2f} us before its end")
        ph["commit(b-1) end -> past the hand-off"] = t[b, 22] - t[b - 1, 4]
        ph["past the hand-off -> commit end"] = t[b, 4] - t[b, 22]
    sub = {}
    bs = b[(t[b, 22] > 0) & (t[b, 23] > 0) & (t[b, 24] > 0) & (t[b, 25] > 0) & (t[b, 49] > 0) & (t[b, 53] > 0)
           & (t[b - 1, 53] > 0) & ((t[b, 16] & 0xffff) == 1)]
    if len(bs):  # single-round batches: the chain from commit(b-1)'s record to commit(b)'s
        sub = {
            "record(b-1) issued -> past the hand-off": t[bs, 22] - t[bs - 1, 53],
            "  hand-off -> export(b-1) in slots": t[bs, 23] - t[bs, 22],
            "  -> its keys": t[bs, 24] - t[bs, 23],
            "  -> rounds start (wave-0 state)": t[bs, 25] - t[bs, 24],
            "  -> guess done": t[bs, 49] - t[bs, 25],
            "  -> evaluation done": t[bs, 50] - t[bs, 49],
            "  -> check done": t[bs, 51] - t[bs, 50],
            "  -> wave 0 past the rounds": t[bs, 52] - t[bs, 51],
            "  -> record issued (export, plan)": t[bs, 53] - t[bs, 52],
            "record(b-1) -> record(b)": t[bs, 53] - t[bs - 1, 53],
            "record(b) -> commit end (publish, outputs)": t[bs, 4] - t[bs, 53],
        }
    print(f"{len(b)} batches (lag {lag})")
    print(f"{'phase':48s} {'mean':>7s} {'p10':>7s} {'p50':>7s} {'p90':>7s} {'p99':>7s} {'max':>9s}  (us)")
    for k, v in ph.items():
        v = us(v.astype(np.float64))
        q = np.percentile(v, [10, 50, 90, 99])
        print(f"{k:48s} {v.mean():7.2f} {q[0]:7.2f} {q[1]:7.2f} {q[2]:7.2f} {q[3]:7.2f} {v.max():9.1f}")
    if sub:
        print(f"single-round batches ({len(bs)}), the commit chain:")
        for k, v in sub.items():
            v = us(v.astype(np.float64))
            q = np.percentile(v, [10, 50, 90, 99])
            print(f"{k:48s} {v.mean():7.2f} {q[0]:7.2f} {q[1]:7.2f} {q[2]:7.2f} {q[3]:7.2f} {v.max():9.1f}")
    sc = b[(t[b, 11] > 0) & (t[b, 12] > 0) & (t[b, 14] > 0) & (t[b, 8] > 0) & (t[b, 9] > 0) & (t[b, 10] > 0)]
    if len(sc):  # WG 0 wave 0's stamps of the screened scan (score_role)
        pairs = (t[sc, 13] >> 32) & 0xffffffff
        onp = pairs != 0xffffffff
        if (t[sc, 37] > 0).all():  # the seeded scan (KC <= 4 kernels): stamp 37 is behind the bound's barrier
            head = {
                "  seed pass (start -> 11)": t[sc, 11] - t[sc, 0],
                "  the other waves' seed pass (11 -> 37)": t[sc, 37] - t[sc, 11],
                "  bound (37 -> 12)": t[sc, 12] - t[sc, 37],
                "  single pass (12 -> 14)": t[sc, 14] - t[sc, 12],
            }
        else:
            head = {
                "  pass 1 (start -> 11)": t[sc, 11] - t[sc, 0],
                "  bound (11 -> 12)": t[sc, 12] - t[sc, 11],
                "  pass 2 (12 -> 14)": t[sc, 14] - t[sc, 12],
            }
        scan = {
            **head,
            "  exact phase (14 -> 8)": t[sc, 8] - t[sc, 14],
            "  barrier after the exact phase (8 -> 9)": t[sc, 9] - t[sc, 8],
            "  rank and entry stores (9 -> 10)": t[sc, 10] - t[sc, 9],
            "  drain, barrier, arrival (10 -> 5)": t[sc, 5] - t[sc, 10],
            "  scan in all (start -> 5)": t[sc, 5] - t[sc, 0],
        }
        print(f"screened scan, WG 0 wave 0 ({len(sc)} batches; pair lists in {onp.sum()}, "
              f"{pairs[onp].mean() if onp.any() else 0:.1f} pairs each, {(t[sc, 13] & 0xffffffff).mean():.2f} rows needed):")
        for k, v in scan.items():
            v = us(v.astype(np.float64))
            q = np.percentile(v, [10, 50, 90, 99])
            print(f"{k:48s} {v.mean():7.2f} {q[0]:7.2f} {q[1]:7.2f} {q[2]:7.2f} {q[3]:7.2f} {v.max():9.1f}")
    per = us((t[b, 4] - t[b - 1, 4]).astype(np.float64))
    med = np.median(per)
    slow = per > 3 * med
    print(f"stalls (period > 3 x median {med:.1f} us): {slow.sum()} batches, {per[slow].sum() / 1e3:.2f} ms of "
          f"{per.sum() / 1e3:.2f} ms")
    order = np.argsort(-per)[:8]
    for i in order:
        bb = b[i]
        c = int(t[bb, 16])
        print(f"  batch {bb}: period {per[i]:.1f} us | score {us(t[bb, 1] - t[bb, 0]):.1f} merge {us(t[bb, 2] - t[bb, 1]):.1f}"
              f" to-commit {us(t[bb, 3] - t[bb, 2]):.1f} commit {us(t[bb, 4] - t[bb, 3]):.1f} | rounds {c & 0xffff}"
              f" rescues {(c >> 16) & 0xff} (waited {us(t[bb, 17]):.1f} us) done {(c >> 24) & 0xff} failed {(c >> 32) & 0xffff}"
              f" one-by-one {c >> 48} | kcycles pro {t[bb, 18] / 1e3:.1f} guess {t[bb, 19] / 1e3:.1f} eval {t[bb, 20] / 1e3:.1f}"
              f" check {t[bb, 21] / 1e3:.1f}")
    cc = t[b, 16]
    rounds, resc, done = cc & 0xffff, (cc >> 16) & 0xff, (cc >> 24) & 0xff
    seq = cc >> 48
    print(f"pods resolved one by one: {seq.sum()} ({seq.sum() / max(len(b), 1):.2f} per batch)")
    cm = us((t[b, 4] - t[b, 3]).astype(np.float64))
    rw = us(t[b, 17].astype(np.float64))
    print(f"rescue waits: {rw.sum() / 1e3:.2f} ms in total, {us(float(t[b, 17].sum())) / max(int(resc.sum()), 1):.1f} us per rescue")
    print("commit time by rescues in the batch:")
    for r in range(int(resc.max()) + 1 if len(resc) else 0):
        s = resc == r
        if s.any():
            print(f"  {r} rescues: {s.sum()} batches, commit mean {cm[s].mean():.1f} p50 {np.median(cm[s]):.1f} max {cm[s].max():.1f} us,"
                  f" rounds mean {rounds[s].mean():.2f}, resolved {done[s].mean():.1f}")
    # The check step's split (columns 33-36: fold of the confirmed columns, probe, commit of the resolved pod, of it
    # the wait for a listed record's state; 38-39: the t* fold over the waves' partial bests, the rescue leg -- look-ahead,
    # rescue and re-key) is written only by a library built with -DKSCHED_COMMIT_SPLIT=1
    # (tools/build_split.sh); the rescans (29) by every build.  Columns 31-32 (the guess step's set-up / fixpoint) have
    # no writer in this tree (they printed as zeros) and are no longer printed.
    split = bool((t[b][:, 33:37] != 0).any())
    print("commit time by rounds (kcycles per batch: prologue / guess / evaluate / check):")
    for lo, hi in ((0, 1), (1, 2), (2, 3), (3, 5), (5, 10), (10, 1 << 16)):
        s = (rounds >= lo) & (rounds < hi)
        if s.any():
            kc = [t[b[s], c].mean() / 1e3 for c in (18, 19, 20, 21, 29, 33, 34, 35, 36, 38, 39)]
            tail = (f"fold {kc[5]:.1f} probe {kc[6]:.1f} pod {kc[7]:.1f} [state load {kc[8]:.1f}] t* {kc[9]:.1f} rescue {kc[10]:.1f} " if split else "")
            print(f"  rounds [{lo},{hi}): {s.sum()} batches, commit mean {cm[s].mean():.1f} max {cm[s].max():.1f} us, total"
                  f" {cm[s].sum() / 1e3:.2f} ms | {kc[0]:.1f} / {kc[1]:.1f} / {kc[2]:.1f} / {kc[3]:.1f}"
                  f" (check: {tail}rescan {kc[4]:.1f})")
    ck = [float(t[b, c].sum()) / 1e6 for c in (21, 33, 34, 35, 36, 29, 38, 39)]
    if split:
        print(f"check step, Mcycles over the call: {ck[0]:.1f} = fold {ck[1]:.1f} + probe {ck[2]:.1f} + pod {ck[3]:.1f}"
              f" [state load {ck[4]:.1f}] + rescan {ck[5]:.1f} + t* fold {ck[6]:.1f} + rescue leg {ck[7]:.1f}"
              f" + rest {ck[0] - ck[1] - ck[2] - ck[3] - ck[5] - ck[6] - ck[7]:.1f}")
    else:
        print(f"check step, Mcycles over the call: {ck[0]:.1f}, of it rescans {ck[5]:.1f} (no split: the library was not"
              f" built with KSCHED_COMMIT_SPLIT)")
    # which phase of the chain is the long one when the period is long
    chain = us((t[b, 4] - t[b - lag, 4]).astype(np.float64))
    print(f"chain (commit(b-L) end -> commit(b) end): mean {chain.mean():.1f} p50 {np.median(chain):.1f} us = "
          f"{lag} x {chain.mean() / lag:.2f}")


if __name__ == "__main__":
    main()
