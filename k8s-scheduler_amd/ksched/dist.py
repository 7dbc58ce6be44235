"""Node-sharded multi-GPU scheduling (one process per GPU).

The node list is cut into contiguous shards, one per rank (global index = shard offset + local
index, so the lowest-index tie-break is unchanged).  Every rank scores all pending pods against its
shard; per speculative batch the ranks exchange their local top-K candidate records (with the
candidates' snapshot node state) by ONE RCCL all-gather issued inside the engine, merge them
identically, and replay the same ordered commit -- each rank writes back only the nodes it owns.
Two exchange transports: the persistent pipeline's device-side exchange (ksched_xchg_*: merger
workgroups write every pod's list straight into each rank's receive ring over xGMI, no launch per
batch), or one RCCL all-gather per batch in the stream pipeline.  torch.distributed only hands out
the 128-byte RCCL unique id and the 128-byte ring handles (IPC handle + epoch hint).
"""
from __future__ import annotations

import os
from typing import Tuple

import numpy as np


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [lo, hi) of n nodes for `rank` of `world` (sizes differ by at most one)."""
    lo = n * rank // world
    hi = n * (rank + 1) // world
    return lo, hi


def env_rank() -> Tuple[int, int, int]:
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    return rank, world, local


def broadcast_bytes(payload, rank: int, src: int = 0) -> bytes:
    """Broadcast a small bytes object from `src` over the default torch.distributed group."""
    import torch.distributed as dist
    obj = [payload if rank == src else None]
    dist.broadcast_object_list(obj, src=src)
    return obj[0]


def setup_exchange(eng, rank: int, world: int, pg=None) -> bool:
    """Device-side candidate exchange (ksched_xchg_*): every rank exports its receive ring's IPC handle,
    the handles are all-gathered over torch.distributed (`pg`, default group), every rank maps them.
    All ranks agree on the outcome: if any rank fails, every rank turns the exchange off again
    (ksched_xchg_close) and False is returned -- no two ranks ever run different transports."""
    import torch.distributed as dist
    ok, h = 1, b""
    try:
        h = eng.xchg_export()
    except Exception:
        ok = 0
    hs = [None] * world
    dist.all_gather_object(hs, (ok, h), group=pg)
    ok = int(all(x[0] for x in hs))
    if ok:
        try:
            eng.xchg_import([x[1] for x in hs])
        except Exception:
            ok = 0
    flags = [None] * world
    dist.all_gather_object(flags, ok, group=pg)
    agreed = all(flags)
    if not agreed:
        eng.xchg_close()
    return agreed


def make_sharded_engine(cl, rank: int, world: int, device: int, mode=None, group=None, comm: bool = True,
                        xchg: bool = False, pg=None, **kw):
    """Engine for this rank's node shard of cluster `cl`.  world > 1: joined to the other ranks by an
    RCCL communicator (one process per GPU, torch.distributed hands out the id; comm=False skips it), or
    -- `group` given -- by an in-process rank group (ranks as threads of this process on one device).
    xchg=True also sets up the device-side exchange of the persistent pipeline (setup_exchange);
    the returned engine's `xchg_ready` tells whether it took."""
    from . import _lib as L
    from .engine import Engine
    lo, hi = shard_range(cl.n_nodes, rank, world)
    if mode is None:
        mode = L.MODE_BATCHED if (world > 1 or cl.mode != "exact") else L.MODE_EXACT
    eng = Engine(mode=mode, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, device=device,
                 rank=rank, nranks=world, node_offset=lo, nodes_global=cl.n_nodes, **kw)
    eng.load_nodes(cl.alloc_cpu[lo:hi], cl.alloc_mem[lo:hi], cl.alloc_pods[lo:hi],
                   labels=None if cl.labels is None else cl.labels[lo:hi],
                   price=None if cl.price is None else cl.price[lo:hi])
    if group is not None:
        eng.set_group(group)
    elif world > 1:
        if comm:
            uid = Engine.unique_id() if rank == 0 else None
            uid = broadcast_bytes(uid, rank)
            eng.set_comm(uid)
        if xchg and not setup_exchange(eng, rank, world, pg=pg) and not comm:
            raise RuntimeError("node-sharded engine: the device exchange could not be set up on every rank "
                               "and no RCCL communicator was requested (comm=False)")
    return eng, (lo, hi)


def merge_ranked(priority: int, shards):
    """The global ranked lists from the node shards' (ksched_rank_merge, host only: no context, no device traffic).
    shards: one Engine.rank() result (idx, score, reason, count, feasible) per rank, in rank order, for the same
    pods and k.  Returns the same five arrays for the whole cluster (best-price: price ascending)."""
    import ctypes as C
    from . import _lib as L
    r = len(shards)
    idx, score, reason, count, feas = (np.ascontiguousarray(np.stack([s[j] for s in shards]), dtype=t)
                                       for j, t in enumerate((np.int32, np.float64, np.uint8, np.int32, np.int32)))
    m, k = idx.shape[1], idx.shape[2]
    oi = np.empty((m, k), np.int32); os_ = np.empty((m, k), np.float64); orr = np.empty((m, k), np.uint8)
    oc = np.empty(m, np.int32); of = np.empty(m, np.int32)
    L.check(L.lib().ksched_rank_merge(int(priority), r, m, k, L.ptr(idx, C.c_int32), L.ptr(score, C.c_double),
                                      L.ptr(reason, C.c_uint8), L.ptr(count, C.c_int32), L.ptr(feas, C.c_int32),
                                      L.ptr(oi, C.c_int32), L.ptr(os_, C.c_double), L.ptr(orr, C.c_uint8),
                                      L.ptr(oc, C.c_int32), L.ptr(of, C.c_int32)), what="rank_merge")
    return oi, os_, orr, oc, of


def merge_preempt(shards):
    """The cluster's preemption answer from the node shards' (numpy, host only).  shards: one Engine.preempt() result
    (node, nvictims, max_prio, sum_prio, candidates, victims) per rank, in rank order, for the same pods and vcap.
    Per pod the shard with the smallest (max_prio, sum_prio, nvictims, node) among those with a candidate wins --
    ksched_preempt's own order, nodes being global indices -- and `candidates` is the sum over the shards.  Returns the
    same six arrays plus shard int32[m], the winning rank (-1: NO_FIT everywhere): the victims are that rank's row
    as it stands, indices into the table that rank loaded."""
    node, nv, mx, sm, cand, vic = (np.stack([np.asarray(s[j]) for s in shards]) for j in range(6))
    m = node.shape[1]
    none = node < 0
    # lexsort: last key first; shards without a candidate sort behind every other
    order = np.lexsort((np.where(none, np.iinfo(np.int32).max, node), nv, sm, mx, none), axis=0)
    win = order[0]
    at = np.arange(m)
    shard = np.where(none[win, at], -1, win).astype(np.int32)
    return (node[win, at], nv[win, at], mx[win, at], sm[win, at], cand.sum(axis=0).astype(np.int32), vic[win, at], shard)


def gather_node_state(local_state, world: int):
    """Concatenate every rank's (cpu, mem, pods) node state in rank order (torch.distributed)."""
    import torch
    import torch.distributed as dist
    out = []
    for arr in local_state:
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64))
        parts = [None] * world
        dist.all_gather_object(parts, t.numpy())
        out.append(np.concatenate(parts))
    return tuple(out)


def make_local_xchg_group(cl, world: int, device: int = 0, rings: str = "plain", **kw):
    """`world` node-sharded ranks of cluster `cl` as contexts of THIS process on ONE device, joined by the
    device-side exchange (ksched_xchg_join_local_ex; rings: "plain", "uncached" = xchg_export's ring kind, "ipc" =
    also mapped through IPC handles): their persistent kernels run as one cooperative launch, so all ranks'
    grids are resident at once.  The caller runs each rank's schedule calls in its own thread.  Returns
    [(engine, (lo, hi)) per rank]."""
    from . import _lib as L
    from .engine import Engine
    out = [make_sharded_engine(cl, r, world, device=device, mode=L.MODE_BATCHED, comm=False, **kw)
           for r in range(world)]
    Engine.xchg_join_local([e for e, _ in out], rings=rings)
    return out
