#!/usr/bin/env python3
"""CPU simulation of the seeded score scan on the real states of a run -- beside
tests/diag/screen_sim.py and screen_sim_classes.py, whose states, keys and pair accounting it uses.

  python tests/diag/seed_sim.py c4 [G=232] [t0,t1,...] [margin=6e-4] [lag=1]

For the batch of pods [t, t+64) at the state before pod t it compares the needed (row, pod) pairs per workgroup under
  today   the KC-th largest of the 48 (wave, slot) maxima over all rows (the parent's pass 1), and
  seeded  the exact KC-th largest key over the seed rows: the rows that the batch `lag` batches earlier needed (under
          its own seeded bound, from all rows for the first), re-keyed for the new pods on the new state;
and reports the seed rows per workgroup (mean / max), the largest number of seed rows any ONE wave holds (the seed
pass takes as long as its fullest wave), and for each cap (seed rows > rows / d -> seed from all rows) the share of
workgroups past it and the pairs with the cap applied.  f64 keys of the sequential schedule; exploration tool.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_sim as S  # noqa: E402  (also puts the package and the oracle on sys.path)
from screen_sim_classes import class_bound  # noqa: E402

KC, W, SPU = 4, 12, 4


def by_workgroup(K, n, G):
    R = (n + G - 1) // G
    Kp = np.full((K.shape[0], G * R), -np.inf)
    Kp[:, :n] = K
    return Kp.reshape(K.shape[0], R, G)  # [pod, row, workgroup]


def seeded_bound(Kw, seed):
    """seed [row, workgroup] -> L [pod, workgroup]: the KC-th largest key over the seed rows (-inf with fewer)."""
    Ks = np.where(seed[None, :, :], Kw, -np.inf)
    return -np.sort(-Ks, axis=1)[:, KC - 1, :]


def needed(Kw, L, margin):
    return (Kw + margin >= L[:, None, :]) & np.isfinite(Kw)


def stats(need):
    per_wg = need.sum(1).sum(0)
    return f"{per_wg.mean():.0f} / {per_wg.max()}"


def main():
    from ksched import cluster
    cfg = sys.argv[1] if len(sys.argv) > 1 else "c4"
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 232
    ts = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [192]
    margin = float(sys.argv[4]) if len(sys.argv) > 4 else 6e-4
    lag = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    cl = cluster.make_cluster(cfg)
    cache = f"/tmp/screen_sim_{cfg}_idx.npy"
    if not os.path.exists(cache) or np.load(cache).shape[0] < max(ts):
        import oracle as O
        np.save(cache, O.schedule(cl, nthreads=min(os.cpu_count() or 8, 16), n_pods=max(ts))[0])
    idx = np.load(cache)
    n = cl.n_nodes
    for t in ts:
        t0 = t - 64 * lag
        assert t0 >= 0, "the seeding batch lies before the run"
        # the seeding batch's needed rows, under a bound from all rows
        K0 = by_workgroup(S.keys(cl, slice(t0, t0 + 64), *S.state_at(cl, idx, t0)), n, G)
        seed = needed(K0, seeded_bound(K0, np.ones(K0.shape[1:], bool)), margin).any(0)  # [row, workgroup]
        Kw = by_workgroup(S.keys(cl, slice(t, t + 64), *S.state_at(cl, idx, t)), n, G)
        rows = Kw.shape[1]
        today = needed(Kw, class_bound(Kw, KC, W, SPU), margin)
        full = needed(Kw, seeded_bound(Kw, np.ones_like(seed)), margin)
        sd = needed(Kw, seeded_bound(Kw, seed), margin)
        per_wg = seed.sum(0)
        per_wave = np.array([seed[w::W, :].sum(0) for w in range(W)])  # [wave, workgroup]
        print(f"{cfg} before pod {t} (seeds from the batch {lag} before), {rows} rows per workgroup: pairs per workgroup "
              f"mean / max: today {stats(today)}, seeded {stats(sd)}, all rows as seeds {stats(full)} | seed rows per "
              f"workgroup {per_wg.mean():.0f} / {per_wg.max()}, fullest wave {per_wave.max(0).mean():.1f} / {per_wave.max()}"
              f" | workgroups over 704 pairs: today {(today.sum(1).sum(0) > 704).sum()}, seeded {(sd.sum(1).sum(0) > 704).sum()}")
        for d in (8, 4, 2):
            over = per_wg * d > rows
            capped = np.where(over[None, None, :], full, sd)
            print(f"    cap rows / {d}: {over.mean():.3f} of the workgroups past it, pairs {stats(capped)}, seed pass rows of "
                  f"the fullest wave {np.where(over, (rows + W - 1) // W, per_wave.max(0)).mean():.1f}")


if __name__ == "__main__":
    main()
