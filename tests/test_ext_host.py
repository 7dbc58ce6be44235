"""ksched_schedule_ext without a GPU: the library's exports and the binding's constant, the CPU restatement (ext_ref) on
the worked example of include/ksched.h's rules, and ksched.host's ext_tables on Kubernetes-shaped nodes and pods."""
import ctypes as C
import json

import numpy as np
import pytest

import ext_ref as ER

GPU = "amd.com/gpu"


def test_library_exports_the_ext_calls():
    from test_abi import header_symbols
    from ksched import _lib as L
    lb = L.lib()
    syms = header_symbols()
    for s in ("ksched_load_ext", "ksched_read_ext", "ksched_schedule_ext"):
        assert s in syms and hasattr(lb, s), s
    assert L.EXT_MAX == 4
    assert any(ln.split()[:3] == ["#define", "KSCHED_EXT_MAX", "4"] for ln in open(L.HEADER_PATH).read().splitlines())
    one = np.zeros(1, np.int64)
    assert lb.ksched_load_ext(None, 1, L.ptr(one, C.c_int64)) == L.E_INVALID
    assert lb.ksched_read_ext(None, L.ptr(one, C.c_int64)) == L.E_INVALID
    assert lb.ksched_schedule_ext(None, 0, None, None, None, None, None, None, None, None) == L.E_INVALID


def test_worked_example_reference(oracle_mod):
    cl, node_ext, req_ext = ER.worked_example()
    idx, score, feas, ext, state, info = ER.schedule_ext(oracle_mod, cl, node_ext, req_ext)
    assert idx.tolist() == [0, 0, 2, -1]
    assert feas.tolist() == [2, 3, 1, 0]
    assert ext.tolist() == [[0, 0, 0]]
    assert score.tolist() == [float(np.float32(0.1)), float(np.float32(0.1)), 0.5, 0.0]
    assert state[0].tolist() == [64000 - 200, 64000, 64000 - 100] and state[2].tolist() == [108, 110, 109]
    assert info == dict(narrowed=3, moved=2, ext_nofit=1, zero_req=1, multi_col=0, exact_fit=2, overdrawn=0)
    assert oracle_mod.schedule(cl)[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("priority,domain", [(0, 0), (0, 1), (1, 1)])
def test_huge_column_is_the_plain_schedule(priority, domain, labels, oracle_mod):
    cl, _, req_ext = ER.adversarial(7, 64, 256, 1, priority, domain, labels)
    assert (req_ext > 0).sum() >= 50
    want = oracle_mod.schedule(cl)
    got = ER.schedule_ext(oracle_mod, cl, np.full((1, 64), 1 << 62, np.int64), req_ext)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert np.array_equal(got[2], want[2]) and all(np.array_equal(a, b) for a, b in zip(got[4], want[3]))
    assert (got[0] >= 0).any() and got[5]["narrowed"] == 0 and got[5]["moved"] == 0
    # the column moved by exactly what the placed pods asked for
    used = np.zeros(64, np.int64)
    np.add.at(used, got[0][got[0] >= 0], req_ext[0][got[0] >= 0])
    assert np.array_equal(got[3][0], (1 << 62) - used) and used.any()


def kube_json():
    """n0 (price 0.10, 2 GPUs, one held by the bound b0), n1 (0.20, no GPU key), n2 (0.50, 4 GPUs); pending: g0 (1 GPU),
    cpu0 (none), g1 (two containers of 1 GPU), g2 (2 GPUs), g3 (1 GPU)."""
    from ksched.host import PRICE_ANNOTATION, SCHEDULER_ANNOTATION

    def node(name, price, gpus):
        cap = {"cpu": "64", "memory": "16777216Ki", "pods": "110", "ephemeral-storage": "100"}
        if gpus is not None:
            cap[GPU] = str(gpus)
        return {"metadata": {"name": name, "annotations": {PRICE_ANNOTATION: price}}, "status": {"capacity": cap}}

    def pod(name, gpus, node_name=""):
        conts = [{"name": f"c{k}", "resources": {"requests": {"cpu": "100m", **({GPU: str(g)} if g else {})}}}
                 for k, g in enumerate(gpus)]
        return {"metadata": {"name": name, "annotations": {SCHEDULER_ANNOTATION: "hightower"}},
                "spec": {"nodeName": node_name, "containers": conts}}

    nodes = {"items": [node("n0", "0.10", 2), node("n1", "0.20", None), node("n2", "0.50", 4)]}
    pods = {"items": [pod("b0", [1], "n0"), pod("g0", [1]), pod("cpu0", [0]), pod("g1", [1, 1]), pod("g2", [2]),
                      pod("g3", [1])]}
    return nodes, pods


def objects():
    from ksched.host import node_from_kube, pod_from_kube
    nl, pl = kube_json()
    nodes = [node_from_kube(x) for x in json.loads(json.dumps(nl))["items"]]  # through JSON text, as the apiserver sends it
    pods = [pod_from_kube(x) for x in json.loads(json.dumps(pl))["items"]]
    return nodes, [p for p in pods if p.node_name], [p for p in pods if not p.node_name]


def test_loaders_keep_unknown_resources():
    nodes, bound, pending = objects()
    assert nodes[0].capacity[GPU] == "2" and GPU not in nodes[1].capacity and nodes[2].capacity["ephemeral-storage"] == "100"
    assert bound[0].containers[0].requests == {"cpu": "100m", GPU: "1"}
    assert [c.requests.get(GPU) for c in pending[2].containers] == ["1", "1"]


def test_ext_tables():
    from ksched.host import Container, Pod, ext_tables
    nodes, bound, pending = objects()
    names, node_ext, req_ext = ext_tables(nodes, bound, pending)
    assert names == [GPU]                                                        # cpu, memory and pods are not extended
    assert node_ext.tolist() == [[1, 0, 4]] and node_ext.dtype == np.int64         # n0: 2 - b0's 1; n1: absent is 0
    assert req_ext.tolist() == [[1, 0, 2, 2, 1]] and req_ext.dtype == np.int64     # g1: the sum over its containers
    # explicit names, in the caller's order; a name nobody asks for is a column of zero requests
    names, node_ext, req_ext = ext_tables(nodes, bound, pending, names=["ephemeral-storage", GPU])
    assert names == ["ephemeral-storage", GPU]
    assert node_ext.tolist() == [[100, 100, 100], [1, 0, 4]] and req_ext.tolist() == [[0] * 5, [1, 0, 2, 2, 1]]
    # default names are sorted; a bound pod on an unknown node is ignored, as one on a known node is counted
    more = pending + [Pod("h", [Container("c", {"hugepages-2Mi": "512", "a.example/nic": "1"})])]
    names, node_ext, req_ext = ext_tables(nodes, bound + [Pod("b1", [Container("c", {GPU: "3"})], node_name="n2")], more)
    assert names == ["a.example/nic", GPU, "hugepages-2Mi"]
    assert node_ext.tolist() == [[0, 0, 0], [1, 0, 1], [0, 0, 0]] and req_ext[:, -1].tolist() == [1, 0, 512]
    # no extended resource at all: one column of zeros
    names, node_ext, req_ext = ext_tables(nodes, bound, pending[1:2])
    assert names == [] and node_ext.tolist() == [[0, 0, 0]] and req_ext.tolist() == [[0]]


def test_ext_tables_errors():
    from ksched.host import Container, Pod, ext_tables
    nodes, bound, pending = objects()
    five = Pod("five", [Container("c", {f"x.example/r{k}": "1" for k in range(5)})])
    with pytest.raises(ValueError, match="at most 4"):
        ext_tables(nodes, bound, pending + [five])
    with pytest.raises(ValueError, match="at most 4"):
        ext_tables(nodes, bound, pending, names=["a", "b", "c", "d", "e"])
    for bad in ("1.5", "2Gi", "-1", "", "1e3", " 1"):
        with pytest.raises(ValueError, match="plain decimal integer"):
            ext_tables(nodes, bound, pending + [Pod("bad", [Container("c", {GPU: bad})])])
    with pytest.raises(ValueError, match="plain decimal integer"):  # a node's capacity and a bound pod's request too
        ext_tables(nodes, bound, pending, names=["memory"])
    with pytest.raises(ValueError, match="plain decimal integer"):
        ext_tables(nodes, bound + [Pod("b1", [Container("c", {GPU: "500m"})], node_name="n2")], pending)
