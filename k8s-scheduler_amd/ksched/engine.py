"""Python front-end of the C-ABI engine (one context = one GPU = one node shard).

    eng = Engine(priority=PRIORITY_RESOURCE, mode=MODE_EXACT)
    eng.load_nodes(alloc_cpu, alloc_mem, alloc_pods, labels=None, price=None)
    idx, score, feasible = eng.schedule(req_cpu, req_mem, req_pods, selector=None)

`schedule` is the batched equivalent of the reference's schedulePods loop
(anchor/schedule.go:185-197): pods are resolved strictly in order and every placement is committed
before the next pod is evaluated.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L

# ksched_stats.pipeline (include/ksched.h KSCHED_PIPE_*)
PIPELINES = {0: "none", 1: "exact", 2: "stream", 3: "stream-sequential", 4: "persistent"}


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


class _Constraints:
    """The constraint arguments of the schedule_* calls and rank_full as the library takes them: contiguous arrays of
    its types (None stays None: a NULL pointer; gang_min and enforce only with gang_off and group), the gang_placed
    buffer, and each constraint's arguments as ctypes values in the prototypes' order.  check(p): every length against
    the pod count."""

    def __init__(self, engine, gang_off=None, gang_min=None, group=None, enforce=None, req_ext=None, member=None,
                 anti_host=None, anti_zone=None, aff_group=None, aff_zone=None):
        def arr(a, dtype, given=True):
            return None if a is None or not given else np.ascontiguousarray(a, dtype=dtype)

        def flags(a, given=True):
            return None if a is None or not given else np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)
        off = arr(gang_off, np.int64)
        ng = 0 if off is None else off.shape[0] - 1
        gmin = arr(gang_min, np.int32, off is not None)
        assert ng >= 0 and (gmin is None or gmin.shape[0] == ng)
        gr = arr(group, np.int32)
        self.per_pod = [gr, flags(enforce, gr is not None)] + [arr(m, np.uint64) for m in (member, anti_host, anti_zone)] + [
            arr(aff_group, np.int32), flags(aff_zone)]
        self.req_ext = arr(req_ext, np.int64)
        self.ext_rows = getattr(engine, "_ext_shape", (None,))[0]  # the load_ext() table's, where one was loaded
        self.gp = np.empty(ng, np.int32)
        self.placed = L.ptr(self.gp, C.c_int32)
        self.gang_arrays = (off, gmin)  # (held while the pointers are in use)
        self.gangs = (ng, L.ptr(off, C.c_int64), L.ptr(gmin, C.c_int32))
        types = (C.c_int32, C.c_uint8, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint8)
        ptrs = tuple(L.ptr(a, t) for a, t in zip(self.per_pod, types))
        self.spread, self.ext, self.affinity = ptrs[:2], (L.ptr(self.req_ext, C.c_int64),), ptrs[2:]

    def check(self, p):
        assert all(a is None or a.shape == (p,) for a in self.per_pod)
        re_ = self.req_ext
        assert re_ is None or (re_.ndim == 2 and re_.shape == (re_.shape[0] if self.ext_rows is None else self.ext_rows, p))


class Group:
    """In-process rank group (ksched_group): R contexts of this process on one device exchange their
    per-batch candidate lists through a shared device ring instead of RCCL.  Each rank's Engine calls
    set_group(); the ranks then run the same schedule calls concurrently (one thread each)."""

    def __init__(self, nranks: int, device: int = -1):
        h = C.c_void_p()
        L.check(L.lib().ksched_group_create(int(nranks), int(device), C.byref(h)), what="group_create")
        self._h = h
        self.nranks = nranks

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ksched_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, mode: int = L.MODE_AUTO, priority: int = L.PRIORITY_RESOURCE, domain: int = L.DOMAIN_ALL,
                 use_labels: bool = False, batch: int = 0, topk: int = 0, device: int = -1,
                 rank: int = 0, nranks: int = 1, node_offset: int = 0, nodes_global: int = 0, exact_wgs: int = 0,
                 timing: bool = False, timing_every: int = 0, chunk_topk: int = 0,
                 commit_impl: int = 0, pipeline: int = L.PIPELINE_AUTO, pipe_wgs: int = 0):
        lb = L.lib()
        o = L.Opts()
        L.check(lb.ksched_default_opts(C.byref(o)), what="default_opts")
        o.mode, o.priority, o.domain, o.use_labels = mode, priority, domain, int(bool(use_labels))
        o.batch, o.topk, o.device = batch, topk, device
        o.rank, o.nranks, o.node_offset, o.nodes_global, o.exact_wgs = rank, nranks, node_offset, nodes_global, exact_wgs
        o.timing, o.timing_every, o.chunk_topk = int(bool(timing)), timing_every, chunk_topk
        o.commit_impl = commit_impl
        o.pipeline, o.pipe_wgs = pipeline, pipe_wgs
        ctx = L.CTX()
        L.check(lb.ksched_create(C.byref(o), C.byref(ctx)), what="create")
        self._ctx = ctx
        self.opts = o
        self.n = -1
        self.p = 0

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            L.lib().ksched_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc, what):
        L.check(rc, self._ctx, what)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        L.check(L.lib().ksched_get_unique_id(buf), what="get_unique_id")
        return buf.raw

    def set_comm(self, uid: bytes):
        assert len(uid) == 128
        self._chk(L.lib().ksched_set_comm(self._ctx, uid), "set_comm")

    def xchg_export(self) -> bytes:
        """Allocate this rank's receive ring of the device-side exchange; returns its IPC handle."""
        buf = C.create_string_buffer(L.XCHG_HANDLE_BYTES)
        self._chk(L.lib().ksched_xchg_export(self._ctx, buf), "xchg_export")
        return buf.raw

    def xchg_import(self, handles):
        """Map every rank's ring (handles in rank order, as xchg_export returned them)."""
        blob = b"".join(handles)
        assert len(blob) == L.XCHG_HANDLE_BYTES * self.opts.nranks
        self._chk(L.lib().ksched_xchg_import(self._ctx, blob), "xchg_import")

    def xchg_close(self):
        """Turn the device exchange off on this rank (the ranks must agree on the transport)."""
        self._chk(L.lib().ksched_xchg_close(self._ctx), "xchg_close")

    @staticmethod
    def xchg_join_local(engines, rings: str = "plain"):
        """Ranks as threads of this process on one device (engines[r] = rank r): the device exchange, the ranks'
        persistent kernels as ONE cooperative launch (ksched_xchg_join_local_ex).  rings: "plain" device memory,
        "uncached" (allocated, zeroed and tagged exactly as xchg_export's) or "ipc" (uncached, and every peer's
        ring mapped from its IPC handle as xchg_import does)."""
        flags = {"plain": 0, "uncached": L.XCHG_RINGS_UNCACHED, "ipc": L.XCHG_RINGS_IPC}[rings]
        arr = (L.CTX * len(engines))(*[e._ctx for e in engines])
        L.check(L.lib().ksched_xchg_join_local_ex(arr, len(engines), flags), engines[0]._ctx, "xchg_join_local")

    @staticmethod
    def close_group(engines):
        """Close the ranks of a local group: every rank's peer maps first (xchg_close), then the contexts."""
        for e in engines:
            if e._ctx:
                L.lib().ksched_xchg_close(e._ctx)
        for e in engines:
            e.close()

    @property
    def xchg_ready(self) -> bool:
        return bool(L.lib().ksched_xchg_ready(self._ctx))

    def set_group(self, group: "Group"):
        self._chk(L.lib().ksched_set_group(self._ctx, group._h), "set_group")
        self._group = group  # keep the group alive as long as this context

    # -- nodes ---------------------------------------------------------------------------------
    def load_nodes(self, alloc_cpu, alloc_mem, alloc_pods, labels=None, price=None):
        ac, am, ap = _i64(alloc_cpu), _i64(alloc_mem), _i64(alloc_pods)
        n = ac.shape[0]
        assert am.shape[0] == n and ap.shape[0] == n
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint64)
        pr = None if price is None else np.ascontiguousarray(price, dtype=np.float32)
        self._chk(L.lib().ksched_load_nodes(self._ctx, n, L.ptr(ac, C.c_int64), L.ptr(am, C.c_int64),
                                            L.ptr(ap, C.c_int64), L.ptr(lab, C.c_uint64), L.ptr(pr, C.c_float)),
                  "load_nodes")
        self.n = n

    def apply_delta(self, node_idx, d_cpu, d_mem, d_pods):
        ix = np.ascontiguousarray(node_idx, dtype=np.int32)
        dc, dm, dp = _i64(d_cpu), _i64(d_mem), _i64(d_pods)
        self._chk(L.lib().ksched_apply_delta(self._ctx, ix.shape[0], L.ptr(ix, C.c_int32), L.ptr(dc, C.c_int64),
                                             L.ptr(dm, C.c_int64), L.ptr(dp, C.c_int64)), "apply_delta")

    def explain(self, req_cpu: int, req_mem: int, req_pods: int, selector: int = 0, per_node: bool = True):
        """Predicate outcome of ONE pod against the current node state (anchor/predicate.go:127-157).
        Returns (counts int64[NUM_REASONS], reasons uint8[n] | None)."""
        cnt = np.zeros(L.NUM_REASONS, np.int64)
        rs = np.empty(max(self.n, 0), np.uint8) if per_node else None
        self._chk(L.lib().ksched_explain(self._ctx, int(req_cpu), int(req_mem), int(req_pods), int(selector),
                                         L.ptr(cnt, C.c_int64), L.ptr(rs, C.c_uint8)), "explain")
        return cnt, rs

    def explain_batch(self):
        """Reason counts (int64[p, NUM_REASONS]) of every NO_FIT pod of the last schedule call at its
        own turn, computed on the device; rows of other pods are zero.  Returns (counts, n_nofit)."""
        cnt = np.zeros((self.p, L.NUM_REASONS), np.int64)
        nf = C.c_int64(0)
        self._chk(L.lib().ksched_explain_batch(self._ctx, self.p, L.ptr(cnt, C.c_int64), C.byref(nf)),
                  "explain_batch")
        return cnt, nf.value

    def explain_pod(self, pod: int, per_node: bool = True):
        """Per-node reasons of pod `pod` of the last schedule call against the state it saw at its turn.
        Returns (counts int64[NUM_REASONS], reasons uint8[n] | None)."""
        cnt = np.zeros(L.NUM_REASONS, np.int64)
        rs = np.empty(max(self.n, 0), np.uint8) if per_node else None
        self._chk(L.lib().ksched_explain_pod(self._ctx, int(pod), L.ptr(cnt, C.c_int64), L.ptr(rs, C.c_uint8)),
                  "explain_pod")
        return cnt, rs

    def rank(self, req_cpu, req_mem, req_pods, selector=None, k: int = 16):
        """Ranked dry run (ksched_rank): for each pod shape, its k best eligible nodes against the current node
        state, in the scheduler's order; nothing is committed.  Returns (idx int32[m, k] (-1 past count),
        score f64[m, k] (score, or price), reason uint8[m, k] (REASON_* of that node), count int32[m],
        feasible int32[m]).  Entry 0 is what schedule() would pick for that pod if it were next."""
        rc, rm, rp = _i64(req_cpu), _i64(req_mem), _i64(req_pods)
        m = rc.shape[0]
        assert rm.shape[0] == m and rp.shape[0] == m
        sel = None if selector is None else np.ascontiguousarray(selector, dtype=np.uint64)
        kk = max(int(k), 0)
        idx = np.empty((m, kk), np.int32); score = np.empty((m, kk), np.float64); reason = np.empty((m, kk), np.uint8)
        count = np.empty(m, np.int32); feas = np.empty(m, np.int32)
        self._chk(L.lib().ksched_rank(self._ctx, m, L.ptr(rc, C.c_int64), L.ptr(rm, C.c_int64), L.ptr(rp, C.c_int64),
                                      L.ptr(sel, C.c_uint64), int(k), L.ptr(idx, C.c_int32), L.ptr(score, C.c_double),
                                      L.ptr(reason, C.c_uint8), L.ptr(count, C.c_int32), L.ptr(feas, C.c_int32)),
                  "rank")
        return idx, score, reason, count, feas

    def load_bound(self, node_idx, cpu, mem, prio):
        """The bound-pod table of preempt() (ksched_load_bound): pod t is bound to local node node_idx[t], holds
        (cpu[t], mem[t]) and one pod slot there and has priority prio[t].  A snapshot: load_nodes() invalidates it,
        schedule calls and apply_delta() leave it alone."""
        ix = np.ascontiguousarray(node_idx, dtype=np.int32)
        bc, bm = _i64(cpu), _i64(mem)
        bp = np.ascontiguousarray(prio, dtype=np.int32)
        nb = ix.shape[0]
        assert bc.shape[0] == nb and bm.shape[0] == nb and bp.shape[0] == nb
        self._chk(L.lib().ksched_load_bound(self._ctx, nb, L.ptr(ix, C.c_int32), L.ptr(bc, C.c_int64),
                                            L.ptr(bm, C.c_int64), L.ptr(bp, C.c_int32)), "load_bound")

    def preempt(self, req_cpu, req_mem, req_pods, selector, prio, vcap: int = 16):
        """Preemption dry run (ksched_preempt): for each pod, the node where the cheapest set of lower-priority bound
        pods would have to go for it to fit, against the current node state and the load_bound() table; nothing is
        committed.  Returns (node int32[m] (global index | NO_FIT), nvictims int32[m] (in full, even above vcap),
        max_prio int32[m], sum_prio int64[m] (the chosen node's key), candidates int32[m], victims int32[m, vcap]
        (table indices, most important first, -1 past the end))."""
        rc, rm, rp = _i64(req_cpu), _i64(req_mem), _i64(req_pods)
        m = rc.shape[0]
        pr = np.ascontiguousarray(prio, dtype=np.int32)
        assert rm.shape[0] == m and rp.shape[0] == m and pr.shape[0] == m
        sel = None if selector is None else np.ascontiguousarray(selector, dtype=np.uint64)
        node = np.empty(m, np.int32); nv = np.empty(m, np.int32); mx = np.empty(m, np.int32)
        sm = np.empty(m, np.int64); cand = np.empty(m, np.int32)
        vic = np.empty((m, max(int(vcap), 0)), np.int32)
        self._chk(L.lib().ksched_preempt(self._ctx, m, L.ptr(rc, C.c_int64), L.ptr(rm, C.c_int64), L.ptr(rp, C.c_int64),
                                         L.ptr(sel, C.c_uint64), L.ptr(pr, C.c_int32), int(vcap), L.ptr(node, C.c_int32),
                                         L.ptr(nv, C.c_int32), L.ptr(mx, C.c_int32), L.ptr(sm, C.c_int64),
                                         L.ptr(cand, C.c_int32), L.ptr(vic, C.c_int32)), "preempt")
        return node, nv, mx, sm, cand, vic

    def load_bound_constrained(self, node_idx, cpu, mem, prio, bound_ext=None, bound_spread=None):
        """load_bound() with the table's two extra columns (ksched_load_bound_constrained): bound_ext[r, t] >= 0, int64
        [R, nb] (None: no columns), is what table pod t holds of extended resource r; bound_spread[t], uint64[nb]
        (None: zeros), has bit s where the pod is counted in group s of the load_spread() table.  preempt() ignores
        both."""
        ix = np.ascontiguousarray(node_idx, dtype=np.int32)
        bc, bm = _i64(cpu), _i64(mem)
        bp = np.ascontiguousarray(prio, dtype=np.int32)
        nb = ix.shape[0]
        assert bc.shape[0] == nb and bm.shape[0] == nb and bp.shape[0] == nb
        be = None if bound_ext is None else np.ascontiguousarray(bound_ext, dtype=np.int64)
        bs = None if bound_spread is None else np.ascontiguousarray(bound_spread, dtype=np.uint64)
        assert (be is None or (be.ndim == 2 and be.shape[1] == nb)) and (bs is None or bs.shape == (nb,))
        self._chk(L.lib().ksched_load_bound_constrained(
            self._ctx, nb, L.ptr(ix, C.c_int32), L.ptr(bc, C.c_int64), L.ptr(bm, C.c_int64), L.ptr(bp, C.c_int32),
            0 if be is None else be.shape[0], L.ptr(be, C.c_int64), L.ptr(bs, C.c_uint64)), "load_bound_constrained")

    def preempt_constrained(self, req_cpu, req_mem, req_pods, selector, prio, group=None, enforce=None, req_ext=None,
                            vcap: int = 16):
        """preempt() under the load_ext() columns and the load_spread() table (ksched_preempt_constrained): a node is
        a candidate, and a bound pod is reprieved, only where the pod also holds its extended requests and satisfies
        its spread constraint with the victims' amounts returned and their counts taken off; against the
        load_bound_constrained() table.  group and req_ext switch their constraint on as in schedule_constrained().
        Nothing is committed and no table moves.  Returns preempt()'s six columns."""
        rc, rm, rp = _i64(req_cpu), _i64(req_mem), _i64(req_pods)
        m = rc.shape[0]
        pr = np.ascontiguousarray(prio, dtype=np.int32)
        assert rm.shape[0] == m and rp.shape[0] == m and pr.shape[0] == m
        sel = None if selector is None else np.ascontiguousarray(selector, dtype=np.uint64)
        cs = _Constraints(self, None, None, group, enforce, req_ext)
        cs.check(m)
        node = np.empty(m, np.int32); nv = np.empty(m, np.int32); mx = np.empty(m, np.int32)
        sm = np.empty(m, np.int64); cand = np.empty(m, np.int32)
        vic = np.empty((m, max(int(vcap), 0)), np.int32)
        self._chk(L.lib().ksched_preempt_constrained(
            self._ctx, m, L.ptr(rc, C.c_int64), L.ptr(rm, C.c_int64), L.ptr(rp, C.c_int64), L.ptr(sel, C.c_uint64),
            L.ptr(pr, C.c_int32), *cs.spread, *cs.ext, int(vcap), L.ptr(node, C.c_int32), L.ptr(nv, C.c_int32),
            L.ptr(mx, C.c_int32), L.ptr(sm, C.c_int64), L.ptr(cand, C.c_int32), L.ptr(vic, C.c_int32)),
            "preempt_constrained")
        return node, nv, mx, sm, cand, vic

    def read_nodes(self):
        ac = np.empty(self.n, np.int64); am = np.empty(self.n, np.int64); ap = np.empty(self.n, np.int64)
        self._chk(L.lib().ksched_read_nodes(self._ctx, self.n, L.ptr(ac, C.c_int64), L.ptr(am, C.c_int64),
                                            L.ptr(ap, C.c_int64)), "read_nodes")
        return ac, am, ap

    def save_state(self):
        self._chk(L.lib().ksched_save_state(self._ctx), "save_state")

    def restore_state(self):
        self._chk(L.lib().ksched_restore_state(self._ctx), "restore_state")

    # -- pods ----------------------------------------------------------------------------------
    def upload_pods(self, req_cpu, req_mem, req_pods, selector=None):
        rc, rm, rp = _i64(req_cpu), _i64(req_mem), _i64(req_pods)
        p = rc.shape[0]
        sel = None if selector is None else np.ascontiguousarray(selector, dtype=np.uint64)
        self._keep = (rc, rm, rp, sel)
        self._chk(L.lib().ksched_upload_pods(self._ctx, p, L.ptr(rc, C.c_int64), L.ptr(rm, C.c_int64),
                                             L.ptr(rp, C.c_int64), L.ptr(sel, C.c_uint64)), "upload_pods")
        self.p = p

    def run(self):
        self._chk(L.lib().ksched_run(self._ctx), "run")

    def sync(self):
        self._chk(L.lib().ksched_sync(self._ctx), "sync")

    def results(self):
        oi = np.empty(self.p, np.int32); os_ = np.empty(self.p, np.float64); of = np.empty(self.p, np.int32)
        self._chk(L.lib().ksched_download_results(self._ctx, self.p, L.ptr(oi, C.c_int32), L.ptr(os_, C.c_double),
                                                  L.ptr(of, C.c_int32)), "download_results")
        return oi, os_, of

    def stats(self) -> dict:
        s = L.Stats()
        self._chk(L.lib().ksched_get_stats(self._ctx, C.byref(s)), "get_stats")
        return dict(pods=s.pods, placed=s.placed, batches=s.batches, truncations=s.truncations,
                    pair_evals=s.pair_evals, device_ms=s.device_ms, kernel_ms=list(s.kernel_ms),
                    kernel_launches=list(s.kernel_launches), kernel_pairs=list(s.kernel_pairs),
                    pipeline=PIPELINES.get(int(s.pipeline), str(int(s.pipeline))), rescues=s.rescues,
                    exact_rows=s.exact_rows, scan_rows=s.scan_rows)

    def seed_stats(self) -> dict:
        """The seeded score scan's counters of the last persistent run, summed over the score workgroups."""
        w = (C.c_int64 * 5)()
        self._chk(L.lib().ksched_get_seed_stats(self._ctx, w), "get_seed_stats")
        return dict(seeded_scans=w[0], seed_rows=w[1], zero_bound_scans=w[2], after_unscreened=w[3], past_cap=w[4])

    def commit_stamps(self) -> dict:
        """The persistent commit's counts of the last run (zeros unless KSCHED_COMMIT_STAMPS was set at create)."""
        w = (C.c_int64 * 32)()
        self._chk(L.lib().ksched_get_commit_stamps(self._ctx, 32, w), "get_commit_stamps")
        return dict(rounds=w[12], failed_guesses=w[13], batches=w[14], early_merged=w[15], early_inh=w[29],
                    early_inh_tried=w[30], guess_iterations=w[5], full_scans=w[8], one_by_one=w[31])

    def set_timing(self, on: bool, every: int = 0):
        """Sampled per-kernel HIP-event timing for the following calls (every: one batch in N)."""
        self._chk(L.lib().ksched_set_timing(self._ctx, int(bool(on)), int(every)), "set_timing")

    def set_timeout(self, ms: int):
        """Bound (ms) of every device-side wait of the persistent pipeline (ksched_set_timeout)."""
        self._chk(L.lib().ksched_set_timeout(self._ctx, int(ms)), "set_timeout")

    def schedule(self, req_cpu, req_mem, req_pods, selector=None):
        """schedulePods over the given pending pods (in order).  Returns (idx, score, feasible)."""
        self.upload_pods(req_cpu, req_mem, req_pods, selector)
        self.run()
        self.sync()
        return self.results()

    def _schedule_with(self, name, req_cpu, req_mem, req_pods, selector, k, extra, tail=()):
        """What the constrained schedule calls share: the contiguous request arrays and their length check, the three
        outputs, the call of ksched_<name> -- extra, the call's constraint arguments out of k (_Constraints, checked
        here against the pod count), go between the selectors and the outputs, tail after them -- and self.p.  Returns
        (idx, score, feasible)."""
        rc, rm, rp = _i64(req_cpu), _i64(req_mem), _i64(req_pods)
        p = rc.shape[0]
        assert rm.shape[0] == p and rp.shape[0] == p
        sel = None if selector is None else np.ascontiguousarray(selector, dtype=np.uint64)
        k.check(p)
        oi = np.empty(p, np.int32); os_ = np.empty(p, np.float64); of = np.empty(p, np.int32)
        self._chk(getattr(L.lib(), "ksched_" + name)(self._ctx, p, L.ptr(rc, C.c_int64), L.ptr(rm, C.c_int64),
                                                     L.ptr(rp, C.c_int64), L.ptr(sel, C.c_uint64), *extra,
                                                     L.ptr(oi, C.c_int32), L.ptr(os_, C.c_double), L.ptr(of, C.c_int32),
                                                     *tail), name)
        self.p = p
        return oi, os_, of

    def schedule_gangs(self, req_cpu, req_mem, req_pods, selector, gang_off, gang_min=None):
        """The pending pods in all-or-nothing groups (ksched_schedule_gangs): gang g is pods [gang_off[g],
        gang_off[g + 1]) and is bound only if at least gang_min[g] of its members (None: all) find a node; a
        rejected gang's commits are undone before the next gang is evaluated.  One launch of the exact kernel,
        whatever the engine's mode.  Returns (idx, score, feasible, gang_placed): idx is GANG_REJECTED for a member
        that found a node in a rejected gang; gang_placed[g] = members bound (0 for a rejected gang)."""
        k = _Constraints(self, gang_off=_i64(gang_off), gang_min=gang_min)
        return self._schedule_with("schedule_gangs", req_cpu, req_mem, req_pods, selector, k, k.gangs,
                                   (k.placed,)) + (k.gp,)

    def load_spread(self, node_domain, max_skew, counts=None, n_domains=None):
        """The spread table of schedule_spread() (ksched_load_spread): node j lies in topology domain node_domain[j]
        (-1: it does not carry the key; the ids must be compact -- every id below the largest is carried by a node),
        group s allows max_skew[s], counts[s, d] (None: zeros) matching pods are already bound in domain d.  The
        counts then live in the engine and move with every schedule_spread(); load_nodes() invalidates the table,
        apply_delta() and restore_state() leave it alone.  n_domains: the number of domains where neither the counts
        nor the largest id says it."""
        nd = np.ascontiguousarray(node_domain, dtype=np.int32)
        sk = np.ascontiguousarray(max_skew, dtype=np.int32)
        assert nd.ndim == 1 and sk.ndim == 1 and nd.shape[0] == max(self.n, 0)
        S = sk.shape[0]
        if counts is None:
            D, cn = (int(nd.max()) + 1 if nd.size else 0) if n_domains is None else int(n_domains), None
        else:
            cn = np.ascontiguousarray(counts, dtype=np.int32)
            assert cn.ndim == 2 and cn.shape[0] == S and n_domains in (None, cn.shape[1])
            D = cn.shape[1]
        self._chk(L.lib().ksched_load_spread(self._ctx, D, L.ptr(nd, C.c_int32), S, L.ptr(sk, C.c_int32),
                                             L.ptr(cn, C.c_int32)), "load_spread")
        self._spread_shape = (S, D)

    def read_spread(self):
        """The spread table's counts, int32[S, D], as the last schedule_spread() (or load_spread()) left them."""
        S, D = getattr(self, "_spread_shape", (0, 0))
        out = np.empty((max(S, 1), max(D, 1)), np.int32)  # (never a null pointer: an engine without a table answers E_STATE)
        self._chk(L.lib().ksched_read_spread(self._ctx, L.ptr(out, C.c_int32)), "read_spread")
        return out[:S, :D]

    def schedule_spread(self, req_cpu, req_mem, req_pods, selector, group, enforce=None):
        """schedule() under one topology spread constraint per pod (ksched_schedule_spread): pod i belongs to group
        group[i] of the load_spread() table (-1: none) and, where enforce[i] (None: every pod), may only land in a
        domain whose count stays within the group's max_skew of the emptiest domain; every placed pod of a group is
        counted.  One launch of the exact kernel, whatever the engine's mode.  Returns (idx, score, feasible)."""
        k = _Constraints(self, group=np.ascontiguousarray(group, dtype=np.int32), enforce=enforce)
        return self._schedule_with("schedule_spread", req_cpu, req_mem, req_pods, selector, k, k.spread)

    def load_ext(self, node_ext):
        """The extended-resource table of schedule_ext() (ksched_load_ext): node_ext[r, j], int64 [R, n] with R in
        1..EXT_MAX, is node j's allocatable amount of resource r -- capacity minus what bound pods hold; any int64.  The
        table then lives in the engine and moves with every schedule_ext(); load_nodes() invalidates it,
        apply_delta() and restore_state() leave it alone."""
        ne = np.ascontiguousarray(node_ext, dtype=np.int64)
        assert ne.ndim == 2 and ne.shape[1] == max(self.n, 0)
        self._chk(L.lib().ksched_load_ext(self._ctx, ne.shape[0], L.ptr(ne, C.c_int64)), "load_ext")
        self._ext_shape = ne.shape

    def read_ext(self):
        """The extended-resource table, int64[R, n], as the last schedule_ext() (or load_ext()) left it."""
        R, n = getattr(self, "_ext_shape", (0, 0))
        out = np.empty(max(R * n, 1), np.int64)  # (never a null pointer: an engine without a table answers E_STATE)
        self._chk(L.lib().ksched_read_ext(self._ctx, L.ptr(out, C.c_int64)), "read_ext")
        return out[:R * n].reshape(R, n)

    def schedule_ext(self, req_cpu, req_mem, req_pods, selector, req_ext=None):
        """schedule() with the load_ext() table's columns in the fit predicate (ksched_schedule_ext): req_ext[r, i] >= 0,
        int64 [R, p] (None: zeros), is pod i's request for resource r; a zero request is not checked, any other must
        not exceed the node's column, and the placed pod's requests are subtracted from its node's columns.  One
        launch of the exact kernel, whatever the engine's mode.  Returns (idx, score, feasible)."""
        k = _Constraints(self, req_ext=req_ext)
        return self._schedule_with("schedule_ext", req_cpu, req_mem, req_pods, selector, k, k.ext)

    def schedule_constrained(self, req_cpu, req_mem, req_pods, selector, gang_off=None, gang_min=None, group=None,
                             enforce=None, req_ext=None):
        """schedule_gangs(), schedule_spread() and schedule_ext() in one launch of the exact kernel
        (ksched_schedule_constrained): a pod's node must fit, satisfy its spread constraint and hold its extended
        requests; a placed pod commits its node row, the load_ext() columns and the load_spread() count, and a rejected
        gang undoes all three.  Each constraint is off where its argument is None: gang_off (every pod a gang of one),
        group (no pod in a spread group; no table needed, a loaded one stays), req_ext (the same for the ext table).
        Returns (idx, score, feasible, gang_placed); gang_placed is empty when gang_off is None."""
        k = _Constraints(self, gang_off, gang_min, group, enforce, req_ext)
        return self._schedule_with("schedule_constrained", req_cpu, req_mem, req_pods, selector, k,
                                   k.gangs + k.spread + k.ext, (k.placed,)) + (k.gp,)

    def load_affinity(self, node_domain=None, node_member=None, node_anti_host=None, node_anti_zone=None, n_domains=None):
        """The affinity table of schedule_affinity() (ksched_load_affinity): node j lies in zone node_domain[j] (-1: it
        does not carry the zone key; the ids must be compact; None: there is no zone key), and of the pods bound on it
        node_member[j] has bit s where one belongs to selector group s, node_anti_host[j] / node_anti_zone[j] where one
        carries a required anti-affinity term against group s at host / zone scope (uint64[n]; None: zeros).  The words
        then live in the engine and gain bits with every schedule_affinity(); load_nodes() invalidates the table,
        apply_delta() and restore_state() leave it alone.  n_domains: the number of zones where the largest id does
        not say it."""
        n = max(self.n, 0)
        nd = None if node_domain is None else np.ascontiguousarray(node_domain, dtype=np.int32)
        assert nd is None or nd.shape == (n,)
        if n_domains is None:
            n_domains = 0 if nd is None or not nd.size else int(nd.max()) + 1
        masks = [None if m is None else np.ascontiguousarray(m, dtype=np.uint64)
                 for m in (node_member, node_anti_host, node_anti_zone)]
        assert all(m is None or m.shape == (n,) for m in masks)
        self._chk(L.lib().ksched_load_affinity(self._ctx, int(n_domains), L.ptr(nd, C.c_int32),
                                               *(L.ptr(m, C.c_uint64) for m in masks)), "load_affinity")

    def read_affinity(self):
        """The affinity table's node words (node_member, node_anti_host, node_anti_zone), uint64[n] each, as the last
        schedule_affinity() (or load_affinity()) left them."""
        out = [np.zeros(max(self.n, 0), np.uint64) for _ in range(3)]
        self._chk(L.lib().ksched_read_affinity(self._ctx, *(L.ptr(o, C.c_uint64) for o in out)), "read_affinity")
        return tuple(out)

    def schedule_affinity(self, req_cpu, req_mem, req_pods, selector, member=None, anti_host=None, anti_zone=None,
                          aff_group=None, aff_zone=None):
        """schedule() under required inter-pod affinity and anti-affinity (ksched_schedule_affinity): pod i belongs to
        the groups of member[i], refuses nodes (anti_host[i]) / zones (anti_zone[i]) that hold a pod of the named
        groups, is refused where a bound pod's term names one of its groups, and -- aff_group[i] >= 0 -- needs a pod
        of that group on its node (aff_zone[i] == 0) or in its zone, unless it is the first of its own group.  uint64[p]
        masks, int32[p] group, uint8[p] scope; None: zeros (no group).  One launch of the exact kernel, whatever the
        engine's mode.  Returns (idx, score, feasible)."""
        k = _Constraints(self, member=member, anti_host=anti_host, anti_zone=anti_zone, aff_group=aff_group, aff_zone=aff_zone)
        return self._schedule_with("schedule_affinity", req_cpu, req_mem, req_pods, selector, k, k.affinity)

    def schedule_full(self, req_cpu, req_mem, req_pods, selector, gang_off=None, gang_min=None, group=None, enforce=None,
                      req_ext=None, member=None, anti_host=None, anti_zone=None, aff_group=None, aff_zone=None):
        """schedule_constrained() and schedule_affinity() in one launch of the exact kernel (ksched_schedule_full): a
        pod's node must fit, satisfy its spread constraint, hold its extended requests and pass its affinity and
        anti-affinity terms; a placed pod commits its node row, the load_ext() columns, the load_spread() count and the
        load_affinity() words, and a rejected gang undoes all four -- the affinity words, which only ever gain bits, go
        back to their values before the gang's first member.  gang_off, group and req_ext switch their constraint on as
        in schedule_constrained(); affinity is on where any of its five arguments is given (None then: zeros, no
        group).  Returns (idx, score, feasible, gang_placed); gang_placed is empty when gang_off is None."""
        k = _Constraints(self, gang_off, gang_min, group, enforce, req_ext, member, anti_host, anti_zone, aff_group, aff_zone)
        return self._schedule_with("schedule_full", req_cpu, req_mem, req_pods, selector, k,
                                   k.gangs + k.spread + k.ext + k.affinity, (k.placed,)) + (k.gp,)

    def schedule_full_why(self, req_cpu, req_mem, req_pods, selector, gang_off=None, gang_min=None, group=None,
                          enforce=None, req_ext=None, member=None, anti_host=None, anti_zone=None, aff_group=None,
                          aff_zone=None, why_rows=None, node_rows=0, trim=True):
        """schedule_full(), and what every pod that fits nowhere saw AT ITS TURN (ksched_schedule_full_why): the same
        launch, the same results and state, and for the first why_rows (None: the pod count) NO_FIT pods, in pod order,
        the nodes per reason code -- against the rows and tables of that moment, the tentative commits of the pod's own
        gang included, which no later call can see -- and for the first node_rows of them every node's code.  Returns
        (idx, score, feasible, gang_placed, why) with why = (pods int32[r], counts int64[r, NUM_REASONS_FULL], reasons
        uint8[min(r, node_rows), n] | None (node_rows 0), nofit): r = min(nofit, why_rows) recorded rows, nofit the
        call's NO_FIT pods in all.  trim=False returns all why_rows / node_rows rows as the library filled them: -1
        and zeros past the recorded ones."""
        k = _Constraints(self, gang_off, gang_min, group, enforce, req_ext, member, anti_host, anti_zone, aff_group, aff_zone)
        wr =_i64(req_cpu).shape[0] if why_rows is None else int(why_rows)
        nr, n = int(node_rows), max(self.n, 0)
        # (the library refuses shapes these cannot hold before it writes: never a buffer sized from a refused argument)
        pods = np.empty(max(wr, 0), np.int32)
        counts = np.empty((max(wr, 0), L.NUM_REASONS_FULL), np.int64)
        ok = 0 <= nr <= wr and nr * n <= L.WHY_MAX_NODE_BYTES
        reasons = np.empty((nr, n), np.uint8) if nr > 0 and ok else None
        nofit = np.zeros(1, np.int64)
        out = self._schedule_with("schedule_full_why", req_cpu, req_mem, req_pods, selector, k,
                                  k.gangs + k.spread + k.ext + k.affinity,
                                  (k.placed, wr, L.ptr(pods if wr > 0 else None, C.c_int32),
                                   L.ptr(counts if wr > 0 else None, C.c_int64), nr, L.ptr(reasons, C.c_uint8),
                                   L.ptr(nofit, C.c_int64)))
        total = int(nofit[0])
        r = min(total, wr) if trim else wr
        return out + (k.gp, (pods[:r], counts[:r], None if nr == 0 else reasons[:min(r, nr)], total))

    def rank_full(self, req_cpu, req_mem, req_pods, selector=None, k: int = 16, group=None, enforce=None, req_ext=None,
                  member=None, anti_host=None, anti_zone=None, aff_group=None, aff_zone=None):
        """rank() under constraints (ksched_rank_full): for each pod shape its k best nodes among those
        schedule_full() would call eligible, against the node rows and the load_spread() / load_ext() /
        load_affinity() tables as they stand; nothing is committed and no table moves.  group, req_ext and the five
        affinity arguments switch their constraint on as in schedule_full().  Returns (idx, score, reason, count,
        feasible, reason_counts): rank()'s five arrays -- reason with the REASON_* codes up to NUM_REASONS_FULL,
        feasible counting eligible nodes -- and reason_counts int64[m, NUM_REASONS_FULL], the nodes per code."""
        rc, rm, rp = _i64(req_cpu), _i64(req_mem), _i64(req_pods)
        m = rc.shape[0]
        assert rm.shape[0] == m and rp.shape[0] == m
        sel = None if selector is None else np.ascontiguousarray(selector, dtype=np.uint64)
        cs = _Constraints(self, None, None, group, enforce, req_ext, member, anti_host, anti_zone, aff_group, aff_zone)
        cs.check(m)
        kk = max(int(k), 0)
        idx = np.empty((m, kk), np.int32); score = np.empty((m, kk), np.float64); reason = np.empty((m, kk), np.uint8)
        count = np.empty(m, np.int32); feas = np.empty(m, np.int32); hist = np.empty((m, L.NUM_REASONS_FULL), np.int64)
        self._chk(L.lib().ksched_rank_full(
            self._ctx, m, L.ptr(rc, C.c_int64), L.ptr(rm, C.c_int64), L.ptr(rp, C.c_int64), L.ptr(sel, C.c_uint64),
            *cs.spread, *cs.ext, *cs.affinity, int(k), L.ptr(idx, C.c_int32), L.ptr(score, C.c_double),
            L.ptr(reason, C.c_uint8), L.ptr(count, C.c_int32), L.ptr(feas, C.c_int32), L.ptr(hist, C.c_int64)),
            "rank_full")
        return idx, score, reason, count, feas, hist

    def explain_full(self, req_cpu: int, req_mem: int, req_pods: int, selector: int = 0, group: int = -1,
                     enforce: bool = True, req_ext=None, member: int = 0, anti_host: int = 0, anti_zone: int = 0,
                     aff_group: int = -1, aff_zone: bool = False, per_node: bool = True):
        """explain() under constraints (ksched_explain_full): ONE pod against the current rows and tables, a constraint
        on where the pod uses it (group >= 0, req_ext given, an affinity word or group).  Returns (counts
        int64[NUM_REASONS_FULL], reasons uint8[n] | None)."""
        cnt = np.zeros(L.NUM_REASONS_FULL, np.int64)
        rs = np.empty(max(self.n, 0), np.uint8) if per_node else None
        re_ = None if req_ext is None else np.ascontiguousarray(req_ext, dtype=np.int64)
        assert re_ is None or re_.shape == (getattr(self, "_ext_shape", (re_.shape[0],))[0],)
        self._chk(L.lib().ksched_explain_full(
            self._ctx, int(req_cpu), int(req_mem), int(req_pods), int(selector), int(group), int(bool(enforce)),
            L.ptr(re_, C.c_int64), int(member), int(anti_host), int(anti_zone), int(aff_group), int(bool(aff_zone)),
            L.ptr(cnt, C.c_int64), L.ptr(rs, C.c_uint8)), "explain_full")
        return cnt, rs


def engine_for(cl, mode: Optional[int] = None, **kw) -> Engine:
    """Engine configured for a ksched.cluster.Cluster and loaded with its nodes."""
    if mode is None:
        mode = L.MODE_EXACT if cl.mode == "exact" else L.MODE_BATCHED
    e = Engine(mode=mode, priority=cl.priority, domain=cl.domain, use_labels=cl.use_labels, **kw)
    e.load_nodes(cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, labels=cl.labels, price=cl.price)
    return e
