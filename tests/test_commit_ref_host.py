"""tests/commit_ref.py without a GPU: the two statements anchored to the oracle, and the coverage the generated cases
must have so that tests/test_gpu_commit_alone.py cannot pass vacuously.  Everything here is about the reference and
the generators alone; no device code runs."""
import collections

import numpy as np
import pytest

import commit_ref as CR


def _cluster(seed, opts, n=120, p=200, edge=True):
    from ksched import cluster
    return cluster.random_small(seed, n_nodes=n, n_pods=p, priority=opts[0], domain=opts[1], use_labels=opts[2], edge=edge)


OPTS = [(CR.PRIO_RESOURCE, CR.DOM_ALL, False), (CR.PRIO_RESOURCE, CR.DOM_FEASIBLE, True), (CR.PRIO_PRICE, CR.DOM_FEASIBLE, False),
        (CR.PRIO_PRICE, CR.DOM_FEASIBLE, True)]


def _universe(cl, opts):
    return CR._Universe(opts, cl.alloc_cpu, cl.alloc_mem, cl.alloc_pods, cl.labels, cl.price, cl.req_cpu, cl.req_mem,
                        cl.req_pods, cl.selector)


# ---- anchoring ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", CR.KS)
def test_commit_ref_is_the_oracles_commit_batch(oracle_mod, K):
    """cut = (cnt == K), nothing inherited: oracle.commit_batch bit for bit, on lists from oracle.local_topk"""
    O = oracle_mod
    stopped = 0
    for seed, opts in enumerate(OPTS * 2):
        u = _universe(_cluster(40 + seed, opts), opts)
        for nb in (1, 37, 64):
            pods = u.pods(slice(seed, seed + nb))
            recs, cut, fc = CR._true_lists(O, u, K, pods)
            done, touched, oi, os_, of = O.commit_batch(opts, K, pods[0], pods[1], pods[2], pods[3] if opts[2] else None,
                                                        recs, fc, nb + 1)
            d, idx, score, feas, xout = CR.commit_ref(O, opts, K, pods, recs, cut, fc, np.zeros(0, CR.XREC_DTYPE))
            assert d == done, (seed, nb)
            assert np.array_equal(idx[:d], oi[:d]) and np.array_equal(CR.bits(score[:d]), CR.bits(os_[:d]))
            assert np.array_equal(feas[:d], of[:d])
            t = touched[np.argsort(touched["idx"])]
            assert np.array_equal(xout["idx"], t["idx"]) and np.array_equal(xout["cur"], t["cur"])
            assert np.array_equal(xout["sb"], t["s0"])
            stopped += d < nb
    assert stopped > 0 or K == 16  # (these clusters never exhaust a list of 16)


@pytest.mark.parametrize("K", CR.KS)
def test_two_chained_commits_are_the_sequential_schedule(oracle_mod, K):
    """lag-2 inheritance: both batches' lists from the SAME snapshot, the second inheriting the first's export"""
    O = oracle_mod
    chained = 0
    for seed, opts in enumerate(OPTS * 2):
        cl = _cluster(70 + seed, opts)
        u = _universe(cl, opts)
        want = O.schedule(cl, n_pods=96)
        nb = 48
        p0, p1 = u.pods(slice(0, nb)), None
        r0, c0, f0 = CR._true_lists(O, u, K, p0)
        d0, i0, s0, fe0, x0 = CR.commit_ref(O, opts, K, p0, r0, c0, f0, np.zeros(0, CR.XREC_DTYPE))
        p1 = u.pods(slice(d0, d0 + nb))
        r1, c1, f1 = CR._true_lists(O, u, K, p1)
        d1, i1, s1, fe1, x1 = CR.commit_ref(O, opts, K, p1, r1, c1, f1, x0)
        got_i = np.concatenate([i0[:d0], i1[:d1]])
        got_s = np.concatenate([s0[:d0], s1[:d1]])
        got_f = np.concatenate([fe0[:d0], fe1[:d1]])
        n = d0 + d1
        assert np.array_equal(got_i, want[0][:n]) and np.array_equal(CR.bits(got_s), CR.bits(want[1][:n])), seed
        assert np.array_equal(got_f, want[2][:n]), seed
        chained += (d1 > 0) and len(x0) > 0
    assert chained > 0


def _same_entries(a, b):
    va, vb = a["valid"] != 0, b["valid"] != 0
    if not np.array_equal(va, vb):
        return False
    return all(np.array_equal(a[f][va], b[f][vb]) for f in ("idx", "a_cpu", "a_mem", "a_pods", "labels")) and \
        np.array_equal(CR.bits(a["key"][va]), CR.bits(b["key"][vb])) and \
        np.array_equal(a["price"][va].view(np.int32), b["price"][vb].view(np.int32))


def test_rank_merge_ref_is_the_oracles_merge(oracle_mod):
    """no cut input: oracle.merge_topk entry for entry; cut exactly when entries were left over"""
    O = oracle_mod
    seen = collections.Counter()
    for mc in CR.merge_cases(O):
        if mc.kind not in ("plain", "ties"):
            continue
        recs, cut, fc = CR.rank_merge_ref(O, mc.K, mc.blocks)
        want, wfc = O.merge_topk(mc.K, mc.R, mc.nb, np.concatenate([b[0] for b in mc.blocks]),
                                 np.concatenate([b[1] for b in mc.blocks]))
        assert _same_entries(recs, want) and np.array_equal(fc, wfc), mc.name
        valid_in = sum((b[0]["valid"].reshape(mc.nb, mc.K) != 0).sum(axis=1) for b in mc.blocks)
        assert np.array_equal(cut != 0, valid_in > mc.K), mc.name
        assert np.array_equal(recs["pad"].reshape(mc.nb, mc.K)[:, 0], cut)
        seen["left" if cut.any() else "all"] += 1
        assert _same_entries(recs, mc.whole[0]), mc.name  # and the unsharded universe's list
    assert seen["left"] and seen["all"]


def test_merge_cases_have_structure(oracle_mod):
    """empty ranks, ties that differ only by index across ranks, 0 / 1 / all inputs cut, leftovers, dropped entries"""
    O = oracle_mod
    seen = collections.Counter()
    for mc in CR.merge_cases(O):
        recs, cut, fc = CR.rank_merge_ref(O, mc.K, mc.blocks)
        out = recs.reshape(mc.nb, mc.K)
        for b in range(mc.nb):
            ls = [blk[0].reshape(mc.nb, mc.K)[b] for blk in mc.blocks]
            ncut = sum(int(l["pad"][0]) != 0 for l in ls)
            nonempty = sum(bool(l["valid"][0]) for l in ls)
            seen[("R", mc.R)] += 1
            seen["empty_rank"] += nonempty < mc.R
            seen["cut0"] += ncut == 0
            seen["cut1"] += ncut == 1 and nonempty > 1
            seen["cutall"] += ncut == nonempty and nonempty > 1
            seen["short_cut_input"] += any(int(l["pad"][0]) and 0 < np.count_nonzero(l["valid"]) < mc.K for l in ls)
            nout = int(np.count_nonzero(out[b]["valid"]))
            total = sum(int(np.count_nonzero(l["valid"])) for l in ls)
            seen["dropped"] += nout < min(total, mc.K)
            seen["leftover"] += total > mc.K
            v = out[b][:nout]
            src = {int(i): r for r, l in enumerate(ls) for i in l["idx"][l["valid"] != 0]}
            seen["cross_rank_tie"] += any(v["key"][q] == v["key"][q + 1] and src[int(v["idx"][q])] != src[int(v["idx"][q + 1])]
                                          for q in range(nout - 1))
            # whatever survives is the exact prefix of the unsharded list
            w = mc.whole[0].reshape(mc.nb, mc.K)[b]
            assert np.array_equal(v["idx"], w["idx"][:nout]), mc.name
    for k in [("R", r) for r in CR.MERGE_RANKS] + ["empty_rank", "cut0", "cut1", "cutall", "short_cut_input", "dropped",
                                                   "leftover", "cross_rank_tie"]:
        assert seen[k] > 0, k


def test_merge_then_commit_is_the_unsharded_commit(oracle_mod):
    """shards merged by rank_merge_ref, then committed, decide what the unsharded list decides, as far as both get"""
    O = oracle_mod
    whole_batch = 0
    for mc in CR.merge_cases(O):
        if mc.kind != "full":  # every full input flagged cut, as the pipeline does
            continue
        u, opts = mc.universe, mc.universe.opts
        recs, cut, fc = CR.rank_merge_ref(O, mc.K, mc.blocks)
        dm, im, sm, fm, xm = CR.commit_ref(O, opts, mc.K, mc.pods, recs, cut, fc, np.zeros(0, CR.XREC_DTYPE))
        wr, wc, wf = CR._true_lists(O, u, mc.K, mc.pods)
        dw, iw, sw, fw, xw = CR.commit_ref(O, opts, mc.K, mc.pods, wr, wc, wf, np.zeros(0, CR.XREC_DTYPE))
        d = min(dm, dw)
        assert np.array_equal(im[:d], iw[:d]) and np.array_equal(CR.bits(sm[:d]), CR.bits(sw[:d])), mc.name
        assert np.array_equal(fm[:d], fw[:d]), mc.name
        if not cut.any():
            assert dm == dw, mc.name
        whole_batch += dm == mc.nb
    assert whole_batch > 0


# ---- the generators' coverage -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", CR.BATCHES)
def test_commit_cases_cover_what_they_claim(oracle_mod, B):
    O = oracle_mod
    cases = CR.commit_cases(O, B)
    seen = collections.defaultdict(set)     # K -> outcomes
    axes = collections.defaultdict(set)     # (family, K) -> variants, nbs, remaps
    chains = collections.defaultdict(int)
    flips = collections.defaultdict(bool)   # K -> a pod with fc0 == 1 ended NO_FIT by the delta
    extra = collections.Counter()
    for c in cases:
        t = CR.case_trace(O, c)
        assert len(c.xin) <= (min(B, 64) if B <= 64 else B) and c.nb <= B and c.lists.size == c.nb * c.K
        v = c.lists["valid"] != 0
        assert (c.lists["idx"][v] >= 0).all() and (c.lists["idx"][v] <= (1 << 31) - 2).all()
        if c.f53:  # fast53's precondition, for every state the commit can reach
            mags = [np.abs(c.lists[f][v]).max(initial=0) for f in ("a_cpu", "a_mem", "a_pods")] + \
                   [np.abs(c.xin["cur"]).max(initial=0), np.abs(c.xin["sb"]).max(initial=0)] + \
                   [np.abs(p).sum() for p in c.pods[:3]]
            assert max(int(m) for m in mags[:5]) + sum(int(m) for m in mags[5:]) < 1 << 52, c.name
            extra["f53_large_state"] += max(int(m) for m in mags[:5]) >= 1 << 50
        seen[c.K] |= CR.outcomes(c, t)
        axes[(c.family, c.K)] |= {("v", c.opts, c.f53), ("nb", c.nb), ("map", c.remap), ("nbmap", c.nb, c.remap),
                                  ("nbv", c.nb, c.opts, c.f53)}
        flips[c.K] |= t["flip1"]
        st = CR.table_stats(c, t)
        if c.remap in ("spc", "thash"):
            chains[(c.remap, c.K)] = max(chains[(c.remap, c.K)], st[c.remap + "_chain"])
        if c.remap == "low16":
            lo = set(int(i) & 0xFFFF for i in t["table"])
            extra["filter_alias"] += len(t["table"]) > 1 and len(lo) == 1
        L = c.lists.reshape(c.nb, c.K)
        inh = set(int(i) for i in c.xin["idx"])
        listed = set(int(i) for i in c.lists["idx"][v])
        extra[("xin", len(c.xin))] += 1
        extra["slots_over_128"] += len(t["table"]) > 128
        extra["short_cut_list"] += bool(((c.cut != 0) & (np.count_nonzero(L["valid"], axis=1) < c.K)).any())
        extra["cut_one_entry"] += bool(((c.cut != 0) & (np.count_nonzero(L["valid"], axis=1) == 1)).any())
        extra["uncut_short"] += bool(((c.cut == 0) & (np.count_nonzero(L["valid"], axis=1) < c.K)).any())
        extra["no_entry_but_feasible"] += bool(((L["valid"][:, 0] == 0) & (c.fc0 > 0)).any())
        extra["entry0_inherited_for_all"] += c.nb > 1 and all(bool(l["valid"][0]) and int(l["idx"][0]) in inh for l in L)
        extra["inherited_in_no_list"] += bool(inh - listed)
        extra["same_list_64"] += c.nb == 64 and all(np.array_equal(L["idx"][0], l) for l in L["idx"])
        if c.opts[1] == CR.DOM_ALL and c.opts[0] == CR.PRIO_RESOURCE:
            # a pod's winner was a touched slot whose state was negative BEFORE that pod: it carried a key still
            extra[("negative_node_wins", c.K)] += t["neg_wins"]
        if c.family == "same" and c.nb == 64:
            extra["same_identical_pods" if len(set(c.pods[0].tolist())) == 1 else "same_zero_mix"] += 1
    for K in CR.KS:
        assert seen[K] >= set(CR.OUTCOMES), (K, set(CR.OUTCOMES) - seen[K])
        assert flips[K] and extra[("negative_node_wins", K)] > 0, K
        for m in ("spc", "thash"):
            assert chains[(m, K)] >= 32, (m, K, chains[(m, K)])
    for (fam, K), a in axes.items():
        assert len([x for x in a if x[0] == "v"]) == 12 and len([x for x in a if x[0] == "nbmap"]) == 12, (fam, K)
        assert len([x for x in a if x[0] == "nbv"]) == 36, (fam, K)
        assert {x[1] for x in a if x[0] == "nb"} == {1, 37, B}
    want = ["filter_alias", "short_cut_list", "cut_one_entry", "uncut_short", "no_entry_but_feasible",
            "entry0_inherited_for_all", "inherited_in_no_list", "f53_large_state", ("xin", 0), ("xin", 1),
            ("xin", min(B, 64))]
    if B == 64:
        want += ["same_list_64", "same_identical_pods", "same_zero_mix"]
    if B == 128:
        want += [("xin", 128), "slots_over_128"]
    for k in want:
        assert extra[k] > 0, (B, k)


def _wrong_batches(O, ignore_cut=False):
    """how many of the anchoring test's batches commit_ref decides differently from oracle.commit_batch"""
    n = 0
    for K in CR.KS:
        for seed, opts in enumerate(OPTS * 2):
            u = _universe(_cluster(40 + seed, opts), opts)
            for nb in (1, 37, 64):
                pods = u.pods(slice(seed, seed + nb))
                recs, cut, fc = CR._true_lists(O, u, K, pods)
                done, _, oi, os_, _ = O.commit_batch(opts, K, pods[0], pods[1], pods[2], pods[3] if opts[2] else None,
                                                     recs, fc, nb + 1)
                d, idx, score, _, _ = CR.commit_ref(O, opts, K, pods, recs, np.zeros_like(cut) if ignore_cut else cut, fc,
                                                    np.zeros(0, CR.XREC_DTYPE))
                m = min(d, done)
                n += d != done or not np.array_equal(idx[:m], oi[:m]) or not np.array_equal(CR.bits(score[:m]), CR.bits(os_[:m]))
    return n


def test_a_wrong_commit_ref_is_caught_by_the_oracle(oracle_mod, monkeypatch):
    """oracle.commit_batch tells the right statement from a subtly wrong one: the tie-break between t* and u* alone
    flipped, or the cut flag ignored.  Only the statement is mutated; no kernel is involved."""
    O = oracle_mod
    assert _wrong_batches(O) == 0
    monkeypatch.setattr(CR, "touched_beats_untouched", lambda tk, ti, uk, ui: tk > uk or (tk == uk and ti > ui))
    assert _wrong_batches(O) > 0
    monkeypatch.undo()
    assert _wrong_batches(O, ignore_cut=True) > 0


