#!/usr/bin/env python3
"""CPU simulation of the pair lists for a bound taken from class maxima, on the real
states of a run -- beside tests/diag/screen_sim.py, whose states and keys it uses.

  python tests/diag/screen_sim_classes.py c4 [G=232] [t0,t1,...] [margin=6e-4]

Wave w's row r = w + k W sits in slot k % SPU; class (w mod m, slot) keeps the maximum key of its rows and the bound
L is the KC-th largest class maximum (m = 12: today's 48 wave slots; m = 6, 3, 1: 24, 12, 4 classes).  For the batch
of pods [t, t+64) it prints the needed (row, pod) pairs per workgroup, the workgroups past the ranking waves' 704 lanes
and past the 1,024-pair limit, and the pods past the pair cap of 48 and past 8 pairs.  Exploration tool.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_sim as S  # noqa: E402  (also puts the package and the oracle on sys.path)


def class_bound(Kw, KC, W=12, SPU=4, wmod=None):
    """Kw: keys [pod, row, workgroup] -> L [pod, workgroup], the KC-th largest maximum over the classes
    (w % wmod, slot).  The classes partition the rows, so L never exceeds the KC-th largest key; with fewer classes
    than KC there is no bound (-inf: every row passes)."""
    wmod = W if wmod is None else wmod
    cls = {}
    for w in range(W):
        for u in range(SPU):
            rows = Kw[:, w::W, :][:, u::SPU, :]
            m = rows.max(axis=1) if rows.shape[1] else np.full((Kw.shape[0], Kw.shape[2]), -np.inf)
            key = (w % wmod, u)
            cls[key] = np.maximum(cls[key], m) if key in cls else m
    m = np.stack(list(cls.values()), axis=1)
    if m.shape[1] < KC:
        return np.full((Kw.shape[0], Kw.shape[2]), -np.inf)
    return -np.sort(-m, axis=1)[:, KC - 1, :]


def pairs_report(Kw, L, margin):
    """Needed (row, pod) pairs for bound L [pod, workgroup]: per workgroup mean / max, workgroups over 704 pairs
    (the ranking waves' lanes) and over 1,024 (the row path), pods over the pair cap of 48 in a workgroup."""
    need = (Kw + margin >= L[:, None, :]) & np.isfinite(Kw)
    per_pod = need.sum(1)          # [pod, workgroup]
    per_wg = per_pod.sum(0)        # [workgroup]
    return (f"pairs per workgroup mean {per_wg.mean():.0f} max {per_wg.max()}, workgroups over 704: {(per_wg > 704).sum()}"
            f" over 1024: {(per_wg > 1024).sum()}, pods over 48 pairs: {(per_pod > 48).sum()}, pods over 8 pairs: "
            f"{(per_pod > 8).mean():.4f} of all")


def main():
    from ksched import cluster
    cfg = sys.argv[1] if len(sys.argv) > 1 else "c4"
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 232
    ts = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0]
    margin = float(sys.argv[4]) if len(sys.argv) > 4 else 6e-4  # eps and the records' 2^-11
    KC, W, SPU = 4, 12, 4
    cl = cluster.make_cluster(cfg)
    idx = None
    if max(ts) > 0:  # the sequential schedule, cached as screen_sim.py caches it
        cache = f"/tmp/screen_sim_{cfg}_idx.npy"
        if not os.path.exists(cache):
            import oracle as O
            np.save(cache, O.schedule(cl, nthreads=os.cpu_count() or 8, n_pods=max(ts))[0])
        idx = np.load(cache)
    n = cl.n_nodes
    for t in ts:
        K = S.keys(cl, slice(t, t + 64), *S.state_at(cl, idx, t))
        R = (n + G - 1) // G
        Kp = np.full((K.shape[0], G * R), -np.inf)
        Kp[:, :n] = K
        Kw = Kp.reshape(K.shape[0], R, G)  # [pod, row, workgroup]
        for wmod in (12, 6, 3, 1):
            print(f"{cfg} t={t} G={G} classes={wmod * SPU:2d} (wave mod {wmod:2d}, slot): "
                  f"{pairs_report(Kw, class_bound(Kw, KC, W, SPU, wmod), margin)}")


if __name__ == "__main__":
    main()
