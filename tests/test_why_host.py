"""ksched_schedule_full_why without a GPU: the library's export, the CPU restatement (why_ref, on full_ref and dryrun_ref
as they are) on the worked example of include/ksched.h, the conditions every case of test_gpu_why.py must meet --
asserted here from the reference and its deliberately wrong variants alone, so a generator that cannot tell "at its turn"
from "now" or from "at the gang's start" fails here and not on the device -- ksched.host's path from Kubernetes-shaped
objects on a stub engine, and the call's own argument checks as a stand-alone program, plain and under the host
sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import full_ref as FR
import why_ref as WR
from test_full_host import StubEngine, case, family, kube_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU = "amd.com/gpu"

_WHY = {}


# every generated case of test_gpu_why.py: name -> (n, p, generator arguments)
def why_cases():
    out = {}
    for pr in (0, 1):
        for dm in (0, 1):
            for lb in (False, True):
                for half in (False, True):
                    out[("family", pr, dm, lb, half)] = (64, 256, family(pr, dm, lb, half))
    out["workgroups"] = (64, 256, dict(domain=1))
    for n in (1, 63, 65):
        out[("nodes", n)] = (n, 256, dict(D=min(3, n), D_aff=min(3, n), domain=1))
    out["two_slots"] = (300, 256, dict(domain=1))
    out["eight_slots"] = (1100, 256, dict(domain=1, labels=True))
    out["no_zone_key"] = (64, 256, dict(D_aff=0, domain=1))
    return out


def why_case(O, name):
    """(case, full reference, why reference over ALL its NO_FIT pods) of a named input, computed once and shared by both
    test files (never modified)."""
    if name not in _WHY:
        n, p, kw = why_cases()[name]
        c, ref = case(O, n, p, **kw)
        _WHY[name] = (c, ref, WR.why(O, c, ref))
    return _WHY[name]


def differing(a, b):
    """Rows (pods) whose per-node codes differ anywhere."""
    return (a != b).any(axis=1)


def test_library_exports_the_why_call():
    from test_abi import header_symbols
    from ksched import _lib as L
    lb = L.lib()
    assert "ksched_schedule_full_why" in header_symbols() and hasattr(lb, "ksched_schedule_full_why")
    assert "ksched_schedule_full_why" in [s[0] for s in L.SIGNATURES]
    assert lb.ksched_abi_version() == 6  # added within ABI 6: the version number does not move
    assert lb.ksched_schedule_full_why(None, 0, *([None] * 4), 0, *([None] * 14), 0, None, None, 0, None, None) == L.E_INVALID


def test_worked_example_reference(oracle_mod):
    c = FR.worked_example()
    ref = FR.schedule_full(oracle_mod, c)
    pods, counts, reasons, nofit = WR.why(oracle_mod, c, ref)
    assert nofit == 1 and pods.tolist() == [2]
    assert reasons.tolist() == [[5, 5, 11, 5]]  # three nodes without a gpu, zone B without a train pod
    assert counts.tolist() == [[0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 1, 0, 0]]
    # what p2 saw: p0 and p1 tentatively on n0 and n1, the gpu column {0, 0, 1, 0} -- a state no call leaves behind
    t = WR.state_before(oracle_mod, c, 2)
    assert np.asarray(t.ext).tolist() == [[0, 0, 1, 0]] and t.words[0].tolist() == [1, 1, 0, 0]
    assert np.asarray(t.counts).tolist() == [[2, 0]]
    # the gang-start variant forgets them: n0-n2 would look eligible to p2
    assert WR.at_gang_start(oracle_mod, c, pods).tolist() == [[0, 0, 0, 5]]
    # (after the call gang 1 sits where gang 0 sat: on this input a dry run happens to give the same four codes)
    assert WR.at_end(c, ref, pods).tolist() == [[5, 5, 11, 5]]


@pytest.mark.parametrize("name", list(why_cases()), ids=str)
def test_gpu_cases_meet_their_conditions(name, oracle_mod):
    """From the reference alone: enough NO_FIT pods, and enough of them whose codes at their turn differ from the codes
    against the end state (what ksched_explain_full says afterwards) and from the gang-start variant (no tentative
    commits).  Every bound is the issue's; the reference reaches each of them on every case, so none is lowered."""
    c, ref, (pods, counts, reasons, nofit) = why_case(oracle_mod, name)
    assert nofit == len(pods) >= 20, nofit
    assert (counts[:, 0] == 0).all() and (counts.sum(axis=1) == c.cl.n_nodes).all()
    d_end = int(differing(WR.at_end(c, ref, pods), reasons).sum())
    d_start = int(differing(WR.at_gang_start(oracle_mod, c, pods), reasons).sum())
    print(f"{name}: NO_FIT {nofit}, differ from the end state {d_end}, from the gang start {d_start}, "
          f"codes {sorted(set(np.unique(reasons).tolist()))}")
    assert d_end >= 10, d_end
    assert d_start >= 5, d_start
    if name == "two_slots":  # codes in slot row k = 1
        assert len(np.unique(reasons[:, 256:])) >= 5
    if name == "eight_slots":  # ... and in the last slot rows of NPT = 8
        assert len(np.unique(reasons[:, 1024:])) >= 5 and c.req_ext.shape[0] == 4 and c.member is not None and c.group is not None


def test_cases_cover_every_code(oracle_mod):
    seen, labels_4, accepted = set(), False, {}
    for name, (n, p, kw) in why_cases().items():
        c, ref, (pods, _, reasons, _) = why_case(oracle_mod, name)
        codes = set(np.unique(reasons).tolist())
        seen |= codes
        labels_4 |= bool(kw.get("labels")) and 4 in codes
        assert kw.get("labels") or 4 not in codes  # (the label check exists under use_labels only)
        if kw.get("half"):
            off = np.asarray(c.gang_off)
            g = np.searchsorted(off, pods, side="right") - 1
            accepted[name] = int((ref[3][g] > 0).sum())
    assert seen == set(range(1, 14)), seen
    assert labels_4
    # half-required gangs: a member that fits nowhere in a gang that is accepted all the same keeps its row
    assert accepted and min(accepted.values()) >= 1, accepted


class WhyStubEngine(StubEngine):
    """test_full_host's stub, answering schedule_full_why from the two references."""

    def schedule_full_why(self, rc, rm, rp, sel, off, gmin, group, enforce, req_ext, *words, why_rows=None, node_rows=0):
        import dataclasses
        self.calls.append("schedule_full_why")
        cl = dataclasses.replace(self.cl, req_cpu=rc, req_mem=rm, req_pods=rp)
        c = FR.Case(cl, off, gmin, *self.spread, group, enforce, self.node_ext, req_ext, *self.aff, *words)
        ref = FR.schedule_full(self.O, c)
        pods, counts, reasons, nofit = WR.why(self.O, c, ref, limit=len(rc) if why_rows is None else why_rows)
        return ref[:4] + ((pods, counts, reasons[:node_rows] if node_rows else None, nofit),)


def test_fake_cluster_schedule_full_why_on_a_stub_engine(oracle_mod):
    from ksched import _lib as L
    from ksched.host import FakeCluster, FitError, GangRejected, node_from_kube, pod_from_kube
    nl, pl = kube_json()
    fc = FakeCluster.__new__(FakeCluster)  # (no device: the engine is the stub)
    fc.nodes = [node_from_kube(x) for x in nl["items"]]
    fc.pods = [pod_from_kube(x) for x in pl["items"]]
    fc.events, fc.use_labels, fc.priority, fc.domain = [], False, L.PRIORITY_BEST_PRICE, L.DOMAIN_FEASIBLE
    fc.engine = WhyStubEngine(oracle_mod, FR.worked_example().cl)
    res = fc.schedule_full_why()
    assert fc.engine.calls == ["load_spread", "load_ext", "load_affinity", "schedule_full_why"]
    assert [p.name for p, _ in res] == ["p0", "p1", "p2", "p3", "p4", "p5"]
    assert [getattr(r, "name", type(r)) for _, r in res] == [GangRejected, GangRejected, FitError, "n0", "n1", "n2"]
    events = [(e["involved"], e["message"]) for e in fc.events if e["reason"] == "FailedScheduling"]
    assert [who for who, _ in events] == ["p0", "p1", "p2"]
    assert events[0][1] == "pod (p0) rejected with its gang (job1): 2 of 3 members placed, 3 needed"
    assert events[2][1] == ("pod (p2) failed to fit in any node\n"
                            f"fit failure on node (n0): Insufficient {GPU}\n"
                            f"fit failure on node (n1): Insufficient {GPU}\n"
                            "fit failure on node (n2): node(s) didn't match pod affinity rules\n"
                            f"fit failure on node (n3): Insufficient {GPU}")
    # without the rows the event is schedule_full's
    fc.pods = [pod_from_kube(x) for x in pl["items"]]
    fc.events = []
    fc.schedule_full_why(node_rows=0)
    assert [e["message"] for e in fc.events if e.get("involved") == "p2"] == ["pod (p2) failed to fit in any node"]


def build_check(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "k8s-scheduler_amd", "csrc"),
                    os.path.join(ROOT, "tests", "diag", "why_check_main.cpp"), "-o", exe], check=True)
    return exe


def test_check_program_builds_and_passes(tmp_path):
    out = subprocess.run([build_check(tmp_path, "why_check", [])], check=True, capture_output=True, text=True).stdout
    assert "all checks passed" in out


def test_check_program_passes_under_the_host_sanitizers(tmp_path):
    """The same program, its own executable, built with the address and undefined-behaviour sanitizers and run directly:
    every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a
    report (and a failed run)."""
    exe = build_check(tmp_path, "why_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "all checks passed" in out
