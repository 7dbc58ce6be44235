"""The list-consuming kernels of the stream pipeline launched ALONE on hand-built lists (ksched_selftest_rank_merge,
ksched_selftest_commit: one launch of k_merge, k_commit or k_commit_spc through the engine's own launchers), against
the CPU statements of tests/commit_ref.py, bit for bit: hash-colliding node indices, cut lists shorter than K, full
inherited exports, counts that reach 0 by the touched nodes' deltas, merges of up to 64 ranks with ties, empty ranks
and cut inputs.  tests/test_commit_ref_host.py anchors the statements to the oracle and asserts, on the CPU, that the
generated cases reach every outcome; here one context without any node row runs them all.

What this does not prove: the persistent pipeline's flavour of commit_spc_batch (lag 3, the touched-node screen,
hand-off records, rescue), which runs only inside k_pipe, and k_merge_pod; they keep their parity tests."""
import ctypes as C

import numpy as np
import pytest

import commit_ref as CR

pytestmark = pytest.mark.gpu

KERNEL = {CR.COMMIT_SEQUENTIAL: "k_commit", CR.COMMIT_SPECULATIVE: "k_commit_spc"}


class Device:
    def __init__(self, ctx):
        from ksched import _lib as L
        self.L, self.lib, self.ctx = L, L.lib(), ctx
        self.results = {}

    def commit_raw(self, impl, K, B, opts, f53, pods, lists, fc0, xin):
        nb = len(pods[0])
        p = self.L.ptr
        rc, rm, rp = (np.ascontiguousarray(a, dtype=np.int64) for a in pods[:3])
        sel = np.ascontiguousarray(pods[3], dtype=np.uint64) if opts[2] else None  # NULL without labels
        lists = np.ascontiguousarray(lists)
        fc0 = np.ascontiguousarray(fc0, dtype=np.int64)
        xbuf = CR.pack_export(xin)
        oi, osc, of = np.zeros(nb, np.int32), np.zeros(nb, np.float64), np.zeros(nb, np.int32)
        ox = np.zeros(CR.XHDR_BYTES + 2 * B * CR.XREC_DTYPE.itemsize, np.uint8)
        ctl = np.zeros(5, np.int64)
        rc_ = self.lib.ksched_selftest_commit(self.ctx, impl, K, B, opts[0], opts[1], int(opts[2]), int(f53), nb,
                                              p(rc, C.c_int64), p(rm, C.c_int64), p(rp, C.c_int64), p(sel, C.c_uint64),
                                              lists.ctypes.data, p(fc0, C.c_int64), xbuf.ctypes.data, p(oi, C.c_int32),
                                              p(osc, C.c_double), p(of, C.c_int32), ox.ctypes.data, p(ctl, C.c_int64))
        return rc_, dict(idx=oi, score=osc, feas=of, ctl=ctl.tolist(), xraw=ox)

    def commit(self, impl, case):
        key = (impl, case.B, case.family, case.seed, case.K, case.nb)
        if key not in self.results:
            rc_, out = self.commit_raw(impl, case.K, case.B, case.opts, case.f53, case.pods, case.lists, case.fc0, case.xin)
            self.L.check(rc_, self.ctx, f"selftest_commit {KERNEL[impl]} {case.name}")
            out["xout"] = CR.unpack_export(out.pop("xraw"))
            self.results[key] = out
        return self.results[key]

    def rank_merge(self, K, R, nb, blocks, O):
        buf = CR.pack_blocks(blocks)
        recs = np.zeros(nb * K, O.REC_DTYPE)
        fc = np.zeros(nb, np.int64)
        self.L.check(self.lib.ksched_selftest_rank_merge(self.ctx, K, R, nb, buf.ctypes.data, recs.ctypes.data,
                                                         self.L.ptr(fc, C.c_int64)), self.ctx, "selftest_rank_merge")
        return recs, fc


@pytest.fixture(scope="module")
def dev(gpu_available):
    from ksched import Engine
    with Engine() as e:  # no node rows are loaded: neither kernel reads any
        yield Device(e._ctx)


def _first_diff(got, want, done):
    """the first field in which a commit's results differ from the statement's, or None"""
    if got["ctl"][0] != want["ctl"][0]:
        return f"done: {got['ctl'][0]} != {want['ctl'][0]}"
    for name, g, w in (("node index", got["idx"][:done], want["idx"][:done]),
                       ("score bits", CR.bits(got["score"][:done]), CR.bits(want["score"][:done])),
                       ("feasible count", got["feas"][:done], want["feas"][:done])):
        bad = np.nonzero(g != w)[0]
        if bad.size:
            return f"pod {bad[0]}: {name} {g[bad[0]]} != {w[bad[0]]}"
    for k, name in ((1, "stats[0]"), (2, "stats[1]"), (3, "stats[2]"), (4, "plan[2]")):
        if got["ctl"][k] != want["ctl"][k]:
            return f"{name}: {got['ctl'][k]} != {want['ctl'][k]}"
    gx, wx = got["xout"], want["xout"]
    if not np.array_equal(gx["idx"], wx["idx"]):
        return f"export nodes: {sorted(set(gx['idx'].tolist()) ^ set(wx['idx'].tolist()))[:4]} on one side only"
    for f in ("cur", "sb", "labels"):
        bad = np.nonzero([not np.array_equal(g, w) for g, w in zip(gx[f], wx[f])])[0]
        if bad.size:
            return f"export of node {gx['idx'][bad[0]]}: {f} {gx[f][bad[0]].tolist()} != {wx[f][bad[0]].tolist()}"
    bad = np.nonzero(gx["price"].view(np.int32) != wx["price"].view(np.int32))[0]
    if bad.size:
        return f"export of node {gx['idx'][bad[0]]}: price"
    return None


def _want(O, case):
    t = CR.case_trace(O, case)
    return dict(idx=t["idx"], score=t["score"], feas=t["feas"], xout=t["xout"],
                ctl=CR.commit_stats(t["done"], t["idx"], case.nb)), t["done"]


@pytest.mark.parametrize("K", CR.KS)
@pytest.mark.parametrize("impl,B", CR.CONFIGS)
def test_commit_alone_is_the_statement(dev, oracle_mod, impl, B, K):
    """every generated case of this kernel, batch size and K: node index, score bits and feasible count over
    [0, done), done, the counters, the plan and the export as a set"""
    O = oracle_mod
    cases = [c for c in CR.commit_cases(O, B) if c.K == K]
    assert len(cases) == len(CR.FAMILIES) * 3 * len(CR.LADDER)
    bad = []
    for c in cases:
        want, done = _want(O, c)
        d = _first_diff(dev.commit(impl, c), want, done)
        if d:
            bad.append(f"{KERNEL[impl]} {c.name}: {d}")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("K", CR.KS)
def test_the_two_commits_agree(dev, oracle_mod, K):
    """k_commit_spc and k_commit on the same cases (batch 64), against each other"""
    O = oracle_mod
    bad = []
    for c in (c for c in CR.commit_cases(O, 64) if c.K == K):
        a, b = dev.commit(CR.COMMIT_SPECULATIVE, c), dev.commit(CR.COMMIT_SEQUENTIAL, c)
        d = _first_diff(a, b, min(a["ctl"][0], b["ctl"][0]))
        if d:
            bad.append(f"k_commit_spc != k_commit, {c.name}: {d}")
    assert not bad, "\n".join(bad[:12])


def _rec_diff(O, got, want, K):
    """all 56 bytes of every valid entry; idx == kNoIdx and valid == 0 for the rest; the cut flag in entry 0's pad"""
    g, w = got.reshape(-1, K), want.reshape(-1, K)
    for b in range(g.shape[0]):
        for q in range(K):
            if w[b, q]["valid"]:
                if g[b, q].tobytes() != w[b, q].tobytes():
                    f = next(n for n in O.REC_DTYPE.names if g[b, q][n].tobytes() != w[b, q][n].tobytes())
                    return f"pod {b} entry {q}: {f} {g[b, q][f]!r} != {w[b, q][f]!r}"
            elif g[b, q]["valid"] != 0 or g[b, q]["idx"] != CR.NO_IDX:
                return f"pod {b} entry {q}: not empty (idx {g[b, q]['idx']}, valid {g[b, q]['valid']})"
        if g[b, 0]["pad"] != w[b, 0]["pad"]:
            return f"pod {b}: cut flag {g[b, 0]['pad']} != {w[b, 0]['pad']}"
    return None


@pytest.mark.parametrize("K", CR.KS)
def test_rank_merge_alone_is_the_statement(dev, oracle_mod, K):
    O = oracle_mod
    bad = []
    cases = [mc for mc in CR.merge_cases(O) if mc.K == K]
    assert {mc.R for mc in cases} == set(CR.MERGE_RANKS)
    for mc in cases:
        want, cut, wfc = CR.rank_merge_ref(O, K, mc.blocks)
        got, fc = dev.rank_merge(K, mc.R, mc.nb, mc.blocks, O)
        d = _rec_diff(O, got, want, K)
        if d is None and not np.array_equal(fc, wfc):
            b = int(np.nonzero(fc != wfc)[0][0])
            d = f"pod {b}: feasible count {fc[b]} != {wfc[b]}"
        if d:
            bad.append(f"k_merge {mc.name}: {d}")
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("impl,B", [(CR.COMMIT_SPECULATIVE, 64), (CR.COMMIT_SEQUENTIAL, 48)])
def test_device_merge_into_device_commit(dev, oracle_mod, impl, B):
    """the device's merged lists, cut flags included, fed to the device's commit: the reference chain's results"""
    O = oracle_mod
    none = np.zeros(0, CR.XREC_DTYPE)
    bad, ran = [], 0
    for mc in CR.merge_cases(O):
        if mc.kind not in ("full", "cut1"):
            continue
        opts = mc.universe.opts
        wl, wcut, wfc = CR.rank_merge_ref(O, mc.K, mc.blocks)
        t = CR.commit_trace(O, opts, mc.K, mc.pods, wl, wcut, wfc, none)
        want = dict(idx=t["idx"], score=t["score"], feas=t["feas"], xout=t["xout"],
                    ctl=CR.commit_stats(t["done"], t["idx"], mc.nb))
        gl, gfc = dev.rank_merge(mc.K, mc.R, mc.nb, mc.blocks, O)
        rc_, got = dev.commit_raw(impl, mc.K, B, opts, False, mc.pods, gl, gfc, none)
        dev.L.check(rc_, dev.ctx, "selftest_commit")
        got["xout"] = CR.unpack_export(got.pop("xraw"))
        d = _first_diff(got, want, t["done"])
        if d:
            bad.append(f"k_merge -> {KERNEL[impl]}, {mc.name}: {d}")
        ran += 1
    assert ran >= 2 * len(CR.KS) * len(CR.MERGE_RANKS)
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("B", [1, 16, 31])
def test_speculative_commit_inherits_64_at_a_small_batch(dev, oracle_mod, B):
    """k_commit_spc admits an inherited export of 64 nodes whatever the batch size: more records than the engine's
    export buffer of 2 B holds.  The first min(B, 37) pods of the full-inheritance cases, at batch size B."""
    O = oracle_mod
    ran, bad = 0, []
    for c in CR.commit_cases(O, 64):
        if c.family != "inherit" or c.nb != 37 or len(c.xin) != 64:
            continue
        nb = min(B, c.nb)
        pods = tuple(a[:nb] for a in c.pods)
        lists, cut, fc0 = c.lists[:nb * c.K], c.cut[:nb], c.fc0[:nb]
        t = CR.commit_trace(O, c.opts, c.K, pods, lists, cut, fc0, c.xin)
        want = dict(idx=t["idx"], score=t["score"], feas=t["feas"], xout=t["xout"], ctl=CR.commit_stats(t["done"], t["idx"], nb))
        rc_, got = dev.commit_raw(CR.COMMIT_SPECULATIVE, c.K, B, c.opts, c.f53, pods, lists, fc0, c.xin)
        dev.L.check(rc_, dev.ctx, "selftest_commit")
        got["xout"] = CR.unpack_export(got.pop("xraw"))
        d = _first_diff(got, want, t["done"])
        if d:
            bad.append(f"k_commit_spc at B={B}, {c.name}: {d}")
        ran += 1
    assert ran >= 12 and not bad, "\n".join(bad[:12])


def test_what_the_engine_would_refuse_is_refused(dev, oracle_mod):
    """KSCHED_E_INVALID and no launch: K outside {4, 8, 16}, nb over B, B over 64 for the speculative kernel, an
    inherited export over 64 (speculative) or over B (sequential)"""
    O = oracle_mod
    c = next(c for c in CR.commit_cases(O, 48) if c.nb == 48 and c.K == 8)
    x65 = np.zeros(65, CR.XREC_DTYPE)
    x65["idx"] = np.arange(65)

    def rc(impl, K=8, B=48, pods=c.pods, lists=c.lists, xin=c.xin):
        return dev.commit_raw(impl, K, B, c.opts, c.f53, pods, lists, c.fc0, xin)[0]

    E = dev.L.E_INVALID
    assert rc(CR.COMMIT_SEQUENTIAL) == 0 and rc(CR.COMMIT_SPECULATIVE) == 0
    assert rc(CR.COMMIT_SEQUENTIAL, K=5) == E and rc(CR.COMMIT_SPECULATIVE, K=32) == E
    assert rc(CR.COMMIT_SEQUENTIAL, B=47) == E                    # nb > B
    assert rc(CR.COMMIT_SPECULATIVE, B=65) == E and rc(CR.COMMIT_SEQUENTIAL, B=129) == E
    assert rc(CR.COMMIT_SPECULATIVE, B=64, xin=x65) == E and rc(CR.COMMIT_SEQUENTIAL, B=64, xin=x65) == E
    assert rc(CR.COMMIT_SEQUENTIAL, B=65, xin=x65) == 0
    few = tuple(a[:16] for a in c.pods)  # a small batch: 65 inherited nodes refused by either kernel, 64 only by k_commit
    assert rc(CR.COMMIT_SPECULATIVE, B=16, pods=few, xin=x65) == E and rc(CR.COMMIT_SEQUENTIAL, B=16, pods=few, xin=x65) == E
    assert rc(CR.COMMIT_SEQUENTIAL, B=16, pods=few, xin=x65[:64]) == E and rc(CR.COMMIT_SEQUENTIAL, B=16, pods=few, xin=x65[:17]) == E
    assert rc(CR.COMMIT_SPECULATIVE, B=16, pods=few, xin=x65[:64]) == 0 and rc(CR.COMMIT_SEQUENTIAL, B=16, pods=few, xin=x65[:16]) == 0
    assert rc(2) == E                                             # not a kernel
    blocks = [(c.lists, c.fc0)]
    buf = CR.pack_blocks(blocks)
    out, fc = np.zeros(c.nb * 8, O.REC_DTYPE), np.zeros(c.nb, np.int64)
    for K, R in ((5, 1), (8, 0), (8, 65)):
        assert dev.lib.ksched_selftest_rank_merge(dev.ctx, K, R, c.nb, buf.ctypes.data, out.ctypes.data,
                                                  dev.L.ptr(fc, C.c_int64)) == E
