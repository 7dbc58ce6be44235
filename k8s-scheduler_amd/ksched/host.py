"""Host-side mirror of the reference's scheduling surface over an in-memory cluster.

The reference drives its hot path through
    schedulePod(pod)  -> predicate(pod) -> priorities(pod, nodes) -> bind(pod, node)
        anchor/schedule.go:68-89, anchor/predicate.go:107-176, anchor/priorities.go:25-63
    schedulePods()    -> for pod in pending: schedulePod(pod)     anchor/schedule.go:185-197
against kube-apiserver (getNodes/getPods, anchor/tools.go:53-108).  FakeCluster keeps the same
function names, argument meaning and error behaviour, with the apiserver replaced by in-memory lists
and the compute by the GPU engine (packing via the C-ABI's Go-exact parser, scoring/commit on device).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
from typing import Dict, List, Optional, Union

import numpy as np

from . import _lib as L
from .engine import Engine


class FitError(Exception):
    """schedulePod's "Unable to schedule pod (%s) failed to fit in any node" (anchor/schedule.go:74-76)."""


class NilNodeError(Exception):
    """The reference binds a nil *Node when no node scores > 0 and panics (anchor/priorities.go:55-62,
    anchor/schedule.go:208); the build reports it instead."""


class GangRejected(Exception):
    """The pod found a node, but fewer members of its gang than the gang needs did: nothing of the gang is bound
    (KSCHED_GANG_REJECTED; build extension, the reference has no pod groups)."""


class FatalParse(Exception):
    """The reference's errFatal on an unparseable quantity (anchor/predicate.go:15,31,39,49)."""


@dataclasses.dataclass
class Container:
    name: str = "c"
    requests: Dict[str, str] = dataclasses.field(default_factory=dict)


@dataclasses.dataclass(frozen=True)
class SpreadConstraint:
    """One topologySpreadConstraints entry with whenUnsatisfiable: DoNotSchedule (build extension)."""
    max_skew: int
    topology_key: str
    match_labels: tuple  # labelSelector.matchLabels as sorted (key, value) pairs

    def matches(self, labels: Dict[str, str]) -> bool:
        return all(labels.get(k) == v for k, v in self.match_labels)


@dataclasses.dataclass(frozen=True)
class AffinityTerm:
    """One requiredDuringSchedulingIgnoredDuringExecution entry of spec.affinity.podAffinity / podAntiAffinity (build
    extension)."""
    topology_key: str
    match_labels: tuple  # labelSelector.matchLabels as sorted (key, value) pairs

    def matches(self, labels: Dict[str, str]) -> bool:
        return all(labels.get(k) == v for k, v in self.match_labels)


@dataclasses.dataclass
class Pod:
    name: str
    containers: List[Container]
    node_name: str = ""
    annotations: Dict[str, str] = dataclasses.field(default_factory=dict)
    uid: str = ""
    node_selector: Dict[str, str] = dataclasses.field(default_factory=dict)
    priority: int = 0  # spec.priority (preemption; build extension, the reference knows no priorities)
    labels: Dict[str, str] = dataclasses.field(default_factory=dict)  # metadata.labels (topology spread groups)
    spread: Optional[SpreadConstraint] = None  # the first DoNotSchedule entry of spec.topologySpreadConstraints
    affinity: tuple = ()       # spec.affinity.podAffinity's required terms (AffinityTerm; affinity_tables admits one)
    anti_affinity: tuple = ()  # spec.affinity.podAntiAffinity's required terms, any number


@dataclasses.dataclass
class Node:
    name: str
    capacity: Dict[str, str]
    labels: int = 0
    price: Optional[str] = None  # price annotation (README.md:43-48)
    label_map: Dict[str, str] = dataclasses.field(default_factory=dict)


SCHEDULER_NAME = "hightower"                                # anchor/schedule.go:30
SCHEDULER_ANNOTATION = "scheduler.alpha.kubernetes.io/name"  # anchor/schedule.go:176
# The README's per-node price (README.md:37-48) has no key in the reference's code; the build reads
# it from this annotation (the upstream Hightower scheduler's key; build-defined).
PRICE_ANNOTATION = "hightower.com/cost"
# Pod groups (Kubernetes coscheduling's PodGroup as the kube-batch annotations; build extension): pods naming the
# same group are bound all-or-nothing, or when at least group-min-member of them fit.
GROUP_NAME_ANNOTATION = "scheduling.k8s.io/group-name"
GROUP_MIN_ANNOTATION = "scheduling.k8s.io/group-min-member"
# Inter-pod affinity's host scope: every node is its own domain of this key, whether or not it carries the label
HOSTNAME_KEY = "kubernetes.io/hostname"


def _as_obj(x):
    return json.loads(x) if isinstance(x, (str, bytes)) else x


class LabelVocab:
    """Build-defined label bitsets: every distinct "key=value" pair seen on a node
    gets one of 64 bits; a pod's nodeSelector becomes the OR of its pairs' bits.  A selector pair no
    node carries maps to a reserved bit no node has, so it fits nowhere (k8s nodeSelector meaning)."""
    UNSATISFIABLE = 63

    def __init__(self):
        self.bits: Dict[str, int] = {}

    def node_bits(self, labels: Dict[str, str]) -> int:
        v = 0
        for k, x in sorted(labels.items()):
            key = f"{k}={x}"
            if key not in self.bits:
                if len(self.bits) >= self.UNSATISFIABLE:
                    raise ValueError("more than 63 distinct node label pairs: widen the bitset")
                self.bits[key] = len(self.bits)
            v |= 1 << self.bits[key]
        return v

    def selector_bits(self, sel: Dict[str, str]) -> int:
        v = 0
        for k, x in sel.items():
            v |= 1 << self.bits.get(f"{k}={x}", self.UNSATISFIABLE)
        return v


def node_from_kube(obj: dict) -> Node:
    """One NodeList item (anchor/types.go:94-106): metadata.name/labels/annotations, status.capacity
    (allocatable is computed from Capacity, anchor/predicate.go:58-60)."""
    md = obj.get("metadata") or {}
    st = obj.get("status") or {}
    ann = md.get("annotations") or {}
    return Node(name=md.get("name", ""), capacity=dict(st.get("capacity") or {}), price=ann.get(PRICE_ANNOTATION),
                label_map=dict(md.get("labels") or {}))


def pod_from_kube(obj: dict) -> Pod:
    """One PodList item / watch event object (anchor/types.go:57-80): containers' resources.requests
    (limits are ignored, anchor/predicate.go:73-77) and spec.nodeName; spec.priority (absent: 0) for preemption;
    metadata.labels and the first DoNotSchedule entry of spec.topologySpreadConstraints (maxSkew, topologyKey,
    labelSelector.matchLabels) for topology spread -- ScheduleAnyway entries and any further ones are ignored; and the
    requiredDuringSchedulingIgnoredDuringExecution terms of spec.affinity.podAffinity / podAntiAffinity (topologyKey,
    labelSelector.matchLabels) for inter-pod affinity -- preferred terms are ignored, a term with matchExpressions or
    a namespaceSelector is a ValueError (it would otherwise match pods it must not)."""
    md = obj.get("metadata") or {}
    sp = obj.get("spec") or {}
    terms = {}
    for kind in ("podAffinity", "podAntiAffinity"):
        out = []
        for t in (((sp.get("affinity") or {}).get(kind) or {}).get("requiredDuringSchedulingIgnoredDuringExecution") or []):
            ls = t.get("labelSelector") or {}
            if ls.get("matchExpressions") or t.get("namespaceSelector"):
                raise ValueError(f"pod ({md.get('name', '')}): {kind} terms support labelSelector.matchLabels only")
            out.append(AffinityTerm(topology_key=t.get("topologyKey", ""),
                                    match_labels=tuple(sorted((ls.get("matchLabels") or {}).items()))))
        terms[kind] = tuple(out)
    spread = None
    for tc in (sp.get("topologySpreadConstraints") or []):
        if tc.get("whenUnsatisfiable", "DoNotSchedule") == "DoNotSchedule":
            ml = (tc.get("labelSelector") or {}).get("matchLabels") or {}
            spread = SpreadConstraint(max_skew=int(tc.get("maxSkew", 1)), topology_key=tc.get("topologyKey", ""),
                                      match_labels=tuple(sorted(ml.items())))
            break
    conts = [Container(name=c.get("name", ""), requests=dict((c.get("resources") or {}).get("requests") or {}))
             for c in (sp.get("containers") or [])]
    return Pod(name=md.get("name", ""), containers=conts, node_name=sp.get("nodeName") or "",
               annotations=dict(md.get("annotations") or {}), uid=md.get("uid", ""),
               node_selector=dict(sp.get("nodeSelector") or {}), priority=int(sp.get("priority") or 0),
               labels=dict(md.get("labels") or {}), spread=spread, affinity=terms["podAffinity"],
               anti_affinity=terms["podAntiAffinity"])


def _strv(items):
    arr = (C.c_char_p * max(1, len(items)))()
    for i, s in enumerate(items):
        arr[i] = None if s is None else s.encode()
    return arr


def pack_nodes(nodes: List[Node], bound: List[Pod]):
    """allocatableResource for every node given the bound pods (anchor/predicate.go:56-105)."""
    n = len(nodes)
    names = _strv([x.name for x in nodes])
    cc = _strv([x.capacity.get("cpu") for x in nodes])
    cm = _strv([x.capacity.get("memory") for x in nodes])
    cp = _strv([x.capacity.get("pods") for x in nodes])
    off = [0]
    ccpu, cmem, bnode = [], [], []
    for p in bound:
        bnode.append(p.node_name)
        for c in p.containers:
            ccpu.append(c.requests.get("cpu"))
            cmem.append(c.requests.get("memory"))
        off.append(len(ccpu))
    offa = np.asarray(off, dtype=np.int64)
    ac = np.zeros(n, np.int64); am = np.zeros(n, np.int64); ap = np.zeros(n, np.int64)
    rc = L.lib().ksched_pack_nodes(n, names, cc, cm, cp, len(bound), _strv(bnode), L.ptr(offa, C.c_int64),
                                   _strv(ccpu), _strv(cmem), L.ptr(ac, C.c_int64), L.ptr(am, C.c_int64),
                                   L.ptr(ap, C.c_int64))
    if rc == L.E_PARSE:
        raise FatalParse("quantity parse failed")
    if rc == L.E_UNKNOWN_NODE:
        raise KeyError("a bound pod names a node that is not in the node list")
    L.check(rc, what="pack_nodes")
    return ac, am, ap


def pack_pods(pods: List[Pod]):
    """requestedResource for every pending pod (anchor/predicate.go:69-81)."""
    off = [0]
    ccpu, cmem = [], []
    for p in pods:
        for c in p.containers:
            ccpu.append(c.requests.get("cpu"))
            cmem.append(c.requests.get("memory"))
        off.append(len(ccpu))
    offa = np.asarray(off, dtype=np.int64)
    k = len(pods)
    rc = np.zeros(k, np.int64); rm = np.zeros(k, np.int64); rp = np.zeros(k, np.int64)
    r = L.lib().ksched_pack_pods(k, L.ptr(offa, C.c_int64), _strv(ccpu), _strv(cmem), L.ptr(rc, C.c_int64),
                                 L.ptr(rm, C.c_int64), L.ptr(rp, C.c_int64))
    if r == L.E_PARSE:
        raise FatalParse("quantity parse failed")
    L.check(r, what="pack_pods")
    return rc, rm, rp


def group_gangs(pods: List[Pod]):
    """Pending pods -> the gangs of ksched_schedule_gangs.  Pods are stable-grouped by GROUP_NAME_ANNOTATION: a gang
    sits at the position of its first member and keeps its members' order; a pod without the annotation is a gang
    of one.  GROUP_MIN_ANNOTATION (on any member; the members must agree) is the gang's minimum, all members by
    default.  Returns (pods reordered, gang_off int64[g + 1], gang_min int32[g]); ValueError for a minimum that is
    not an integer in 1..size or that the members disagree on."""
    gangs: List[List[Pod]] = []
    by_name: Dict[str, int] = {}
    for pod in pods:
        name = pod.annotations.get(GROUP_NAME_ANNOTATION)
        if not name:
            gangs.append([pod])
        elif name in by_name:
            gangs[by_name[name]].append(pod)
        else:
            by_name[name] = len(gangs)
            gangs.append([pod])
    off = [0]
    mins = []
    for members in gangs:
        name = members[0].annotations.get(GROUP_NAME_ANNOTATION) or members[0].name
        stated = {m.annotations[GROUP_MIN_ANNOTATION] for m in members if GROUP_MIN_ANNOTATION in m.annotations}
        if len(stated) > 1:
            raise ValueError(f"gang ({name}): members disagree on {GROUP_MIN_ANNOTATION}: {sorted(stated)}")
        need = len(members)
        if stated:
            try:
                need = int(next(iter(stated)))
            except ValueError:
                raise ValueError(f"gang ({name}): {GROUP_MIN_ANNOTATION} is not an integer") from None
            if need < 1 or need > len(members):
                raise ValueError(f"gang ({name}): {GROUP_MIN_ANNOTATION} {need} is not in 1..{len(members)}")
        off.append(off[-1] + len(members))
        mins.append(need)
    return ([m for members in gangs for m in members], np.asarray(off, dtype=np.int64),
            np.asarray(mins, dtype=np.int32))


def spread_tables(nodes: List[Node], bound: List[Pod], pending: List[Pod]):
    """The inputs of ksched_load_spread / ksched_schedule_spread from Kubernetes objects.  The pending pods' constraints
    must share one topology key (ValueError on a second); domain ids are compacted over the values the nodes carry
    for it, in node order (a node without the label: -1); one group per distinct (selector, maxSkew), in the pending
    pods' order; a group's counts are the bound pods whose labels match its selector, per domain of their node.  A
    pending pod with a constraint enforces its group; one without a constraint whose labels match a group's selector
    only counts in (the first such) group.  Returns (node_domain int32[n], max_skew int32[S], counts int32[S, D],
    group int32[p], enforce uint8[p]); without any constraint, one domain and one empty group."""
    keys = []
    for pod in pending:
        if pod.spread is not None and pod.spread.topology_key not in keys:
            keys.append(pod.spread.topology_key)
    if len(keys) > 1:
        raise ValueError(f"topology spread: one topology key per call, the pending pods name {keys}")
    p = len(pending)
    if not keys:
        return (np.zeros(len(nodes), np.int32), np.ones(1, np.int32), np.zeros((1, 1), np.int32),
                np.full(p, -1, np.int32), np.zeros(p, np.uint8))
    ids: Dict[str, int] = {}
    node_domain = np.full(len(nodes), -1, np.int32)
    for j, nd in enumerate(nodes):
        v = nd.label_map.get(keys[0])
        if v is not None:
            node_domain[j] = ids.setdefault(v, len(ids))
    if not ids:
        raise ValueError(f"topology spread: no node carries the topology key {keys[0]!r}")
    groups: Dict[tuple, int] = {}
    for pod in pending:
        if pod.spread is not None:
            groups.setdefault((pod.spread.match_labels, pod.spread.max_skew), len(groups))
    cons = [SpreadConstraint(max_skew=sk, topology_key=keys[0], match_labels=ml) for ml, sk in groups]
    counts = np.zeros((len(cons), len(ids)), np.int32)
    by_name = {nd.name: j for j, nd in enumerate(nodes)}
    for pod in bound:
        d = node_domain[by_name[pod.node_name]] if pod.node_name in by_name else -1
        if d >= 0:
            for s, c in enumerate(cons):
                counts[s, d] += c.matches(pod.labels)
    group = np.full(p, -1, np.int32)
    enforce = np.zeros(p, np.uint8)
    for i, pod in enumerate(pending):
        if pod.spread is not None:
            group[i] = groups[(pod.spread.match_labels, pod.spread.max_skew)]
            enforce[i] = 1
        else:
            group[i] = next((s for s, c in enumerate(cons) if c.matches(pod.labels)), -1)
    return node_domain, np.asarray([c.max_skew for c in cons], np.int32), counts, group, enforce


def affinity_tables(nodes: List[Node], bound: List[Pod], pending: List[Pod]):
    """The inputs of ksched_load_affinity / ksched_schedule_affinity from Kubernetes objects.  A term's topologyKey is
    HOSTNAME_KEY (host scope) or the one zone key -- the only other key the bound and pending pods' terms name
    (ValueError on a second); zone ids are compacted over the values the nodes carry for it, in node order (a node
    without the label, or no zone key at all: -1).  The group vocabulary is the distinct selectors of the pending pods'
    terms and then of the bound pods' anti-affinity terms, in that order, at most AFF_MAX_GROUPS (ValueError beyond); a
    pod belongs to every group whose selector matches its labels.  The node words are the ORs over the bound pods of a
    node: their groups, and the groups their anti-affinity terms name per scope.  A pending pod may carry one affinity
    term (ValueError on a second) and any number of anti-affinity terms.  Returns (node_domain int32[n], node_member,
    node_anti_host, node_anti_zone uint64[n], member, anti_host, anti_zone uint64[p], aff_group int32[p], aff_zone
    uint8[p])."""
    keys = []
    for pod in pending + bound:
        for t in (pod.affinity if not pod.node_name else ()) + pod.anti_affinity:
            if t.topology_key != HOSTNAME_KEY and t.topology_key not in keys:
                keys.append(t.topology_key)
    if len(keys) > 1 or "" in keys:
        raise ValueError(f"inter-pod affinity: a topologyKey is {HOSTNAME_KEY} or one zone key, the pods name {keys}")
    n, p = len(nodes), len(pending)
    node_domain = np.full(n, -1, np.int32)
    if keys:
        ids: Dict[str, int] = {}
        for j, nd in enumerate(nodes):
            v = nd.label_map.get(keys[0])
            if v is not None:
                node_domain[j] = ids.setdefault(v, len(ids))
    groups: Dict[tuple, int] = {}
    for pod in pending:
        if len(pod.affinity) > 1:
            raise ValueError(f"inter-pod affinity: pod ({pod.name}) carries {len(pod.affinity)} required affinity terms, one is supported")
        for t in pod.affinity + pod.anti_affinity:
            groups.setdefault(t.match_labels, len(groups))
    for pod in bound:
        for t in pod.anti_affinity:
            groups.setdefault(t.match_labels, len(groups))
    if len(groups) > L.AFF_MAX_GROUPS:
        raise ValueError(f"inter-pod affinity: {len(groups)} distinct selectors, at most {L.AFF_MAX_GROUPS} per call")

    def words(pod):
        member = anti_host = anti_zone = 0
        for ml, s in groups.items():
            if all(pod.labels.get(k) == v for k, v in ml):
                member |= 1 << s
        for t in pod.anti_affinity:
            if t.topology_key == HOSTNAME_KEY:
                anti_host |= 1 << groups[t.match_labels]
            else:
                anti_zone |= 1 << groups[t.match_labels]
        return member, anti_host, anti_zone

    node_words = np.zeros((3, n), np.uint64)
    by_name = {nd.name: j for j, nd in enumerate(nodes)}
    for pod in bound:
        j = by_name.get(pod.node_name)
        if j is not None:
            node_words[:, j] |= np.array(words(pod), np.uint64)
    pod_words = np.zeros((3, p), np.uint64)
    aff_group = np.full(p, -1, np.int32)
    aff_zone = np.zeros(p, np.uint8)
    for i, pod in enumerate(pending):
        pod_words[:, i] = np.array(words(pod), np.uint64)
        if pod.affinity:
            aff_group[i] = groups[pod.affinity[0].match_labels]
            aff_zone[i] = pod.affinity[0].topology_key != HOSTNAME_KEY
    return (node_domain, node_words[0].copy(), node_words[1].copy(), node_words[2].copy(), pod_words[0].copy(),
            pod_words[1].copy(), pod_words[2].copy(), aff_group, aff_zone)


CORE_RESOURCES = ("cpu", "memory", "pods")


def _whole(q, what) -> int:
    """An extended-resource quantity: a plain decimal integer (Kubernetes admits only whole numbers for them)."""
    s = str(q)
    if not (s.isascii() and s.isdigit()):
        raise ValueError(f"extended resource quantity {q!r} ({what}) is not a plain decimal integer")
    return int(s)


def ext_tables(nodes: List[Node], bound: List[Pod], pending: List[Pod], names: Optional[List[str]] = None):
    """The inputs of ksched_load_ext / ksched_schedule_ext from Kubernetes objects.  names: the extended resources, by
    default the sorted names that the pending pods' containers request other than cpu, memory and pods; more than
    EXT_MAX is a ValueError.  A quantity is a plain decimal integer string (ValueError otherwise: no suffixes, no
    fractions).  A node's amount is capacity[name] (absent: 0) minus the requests of the bound pods on it; a pod's
    request is the sum over its containers.  Returns (names, node_ext int64[R, n], req_ext int64[R, p]); without any
    name, one column "" of zeros (the table needs at least one)."""
    if names is None:
        names = sorted({k for pod in pending for c in pod.containers for k in c.requests if k not in CORE_RESOURCES})
    names = list(names)
    if len(names) > L.EXT_MAX:
        raise ValueError(f"extended resources: at most {L.EXT_MAX} per call, got {names}")
    R = max(len(names), 1)
    node_ext = np.zeros((R, len(nodes)), np.int64)
    req_ext = np.zeros((R, len(pending)), np.int64)
    by_name = {nd.name: j for j, nd in enumerate(nodes)}
    for r, name in enumerate(names):
        for j, nd in enumerate(nodes):
            if name in nd.capacity:
                node_ext[r, j] = _whole(nd.capacity[name], f"node {nd.name}, {name}")
        for pod in bound:
            j = by_name.get(pod.node_name)
            if j is not None:
                node_ext[r, j] -= sum(_whole(c.requests[name], f"pod {pod.name}, {name}")
                                      for c in pod.containers if name in c.requests)
        for i, pod in enumerate(pending):
            req_ext[r, i] = sum(_whole(c.requests[name], f"pod {pod.name}, {name}")
                                for c in pod.containers if name in c.requests)
    return names, node_ext, req_ext


def bound_constraint_columns(bound: List[Pod], pending: List[Pod], names: List[str]):
    """The two extra columns of ksched_load_bound_constrained's table from Kubernetes objects, for the bound pods in
    their order: what each holds of the extended resources `names` (ext_tables' names; its one empty column where
    there is none), and the mask of the spread groups that count it -- spread_tables' groups for the same pending
    pods, one per distinct (selector, maxSkew) in their order, bit s where the pod's labels match group s's selector.
    Returns (bound_ext int64[R, nb], bound_spread uint64[nb])."""
    bound_ext = np.zeros((max(len(names), 1), len(bound)), np.int64)
    for r, name in enumerate(names):
        for t, pod in enumerate(bound):
            bound_ext[r, t] = sum(_whole(c.requests[name], f"pod {pod.name}, {name}")
                                  for c in pod.containers if name in c.requests)
    groups: Dict[tuple, int] = {}
    for pod in pending:
        if pod.spread is not None:
            groups.setdefault((pod.spread.match_labels, pod.spread.max_skew), len(groups))
    bound_spread = np.zeros(len(bound), np.uint64)
    for (match_labels, _), s in groups.items():
        for t, pod in enumerate(bound):
            if all(pod.labels.get(k) == v for k, v in match_labels):
                bound_spread[t] |= np.uint64(1) << np.uint64(s)
    return bound_ext, bound_spread


def parse_price(s: str) -> float:
    out = C.c_float(0)
    r = L.lib().ksched_parse_price(s.encode(), C.byref(out))
    if r != L.OK:
        raise FatalParse(f"price {s!r}")
    return out.value


class FakeCluster:
    """In-memory stand-in for kube-apiserver + the reference's scheduling functions."""

    def __init__(self, nodes: List[Node], pods: List[Pod], priority: int = L.PRIORITY_RESOURCE,
                 domain: int = L.DOMAIN_ALL, use_labels: bool = False, mode: int = L.MODE_AUTO, explain_failures: bool = True,
                 **engine_kw):
        self.nodes = list(nodes)
        self.pods = list(pods)
        self.events: List[dict] = []
        self.priority, self.domain, self.use_labels = priority, domain, use_labels
        self.explain_failures = explain_failures
        self.engine = Engine(mode=mode, priority=priority, domain=domain, use_labels=use_labels, **engine_kw)
        self._sync_engine()

    # getNodes / getPods analogues
    def get_nodes(self) -> List[Node]:
        return self.nodes

    def get_pods(self) -> List[Pod]:
        return self.pods

    def _sync_engine(self):
        ac, am, ap = pack_nodes(self.nodes, [p for p in self.pods if p.node_name])
        labels = np.array([x.labels for x in self.nodes], dtype=np.uint64) if self.use_labels else None
        price = None
        if self.priority == L.PRIORITY_BEST_PRICE:
            price = np.array([parse_price(x.price) for x in self.nodes], dtype=np.float32)
        self.engine.load_nodes(ac, am, ap, labels=labels, price=price)

    @classmethod
    def from_kube_json(cls, node_list: Union[str, dict], pod_list: Union[str, dict], **kw) -> "FakeCluster":
        """A cluster from the apiserver's NodeList / PodList JSON (what getNodes/getPods decode,
        anchor/tools.go:53-108, anchor/types.go:48-123).  Node label maps become bitsets when
        use_labels is set; the best-price priority reads PRICE_ANNOTATION."""
        nl, pl = _as_obj(node_list), _as_obj(pod_list)
        nodes = [node_from_kube(x) for x in (nl.get("items") or [])]
        pods = [pod_from_kube(x) for x in (pl.get("items") or [])]
        vocab = LabelVocab()
        for nd in nodes:
            nd.labels = vocab.node_bits(nd.label_map)
        c = cls(nodes, pods, **kw)
        c.vocab = vocab
        return c

    def unscheduled_pods(self) -> List[Pod]:
        """getUnscheduledPods (anchor/schedule.go:148-183): pods with no nodeName that name this
        scheduler in their annotation, in list order."""
        return [p for p in self.pods
                if not p.node_name and p.annotations.get(SCHEDULER_ANNOTATION) == SCHEDULER_NAME]

    def selector_of(self, pod: Pod) -> int:
        vocab = getattr(self, "vocab", None)
        return vocab.selector_bits(pod.node_selector) if vocab is not None else 0

    def _node_index(self, name: str) -> int:
        for i, nd in enumerate(self.nodes):
            if nd.name == name:
                return i
        raise KeyError(f"pod bound to unknown node {name!r} (reference: nil dereference, anchor/predicate.go:94-99)")

    def _charge(self, pod: Pod, sign: int) -> None:
        rc, rm, _ = pack_pods([pod])
        i = self._node_index(pod.node_name)
        # used += (cpu, mem, 1) per bound pod (anchor/predicate.go:83-105) => allocatable -= ...
        self.engine.apply_delta([i], [-sign * int(rc[0])], [-sign * int(rm[0])], [-sign])

    def handle_event(self, event: Union[str, dict]):
        """One pod watch event (PodWatchEvent, anchor/types.go:54-57).  The reference's watch loop
        schedules every ADDED unscheduled pod (anchor/schedule.go:45-58, 91-143) and re-counts every
        bound pod on each predicate call (anchor/predicate.go:83-105); here bound pods maintain the
        device node state incrementally (ksched_apply_delta) instead.  Returns the schedule result
        (pod, node | Exception) for an ADDED pending pod, else None."""
        ev = _as_obj(event)
        typ, pod = ev.get("type"), pod_from_kube(ev.get("object") or {})
        known = {p.name: p for p in self.pods}
        if typ == "ADDED":
            if pod.name in known:
                return None
            self.pods.append(pod)
            if pod.node_name:
                self._charge(pod, +1)
                return None
            # the watch selects spec.nodeName= only, with no scheduler-name check (anchor/schedule.go:
            # 94-95, 127-129, 52-56), unlike getUnscheduledPods
            return self.schedule_pods([pod])[0]
        if typ == "MODIFIED":
            old = known.get(pod.name)
            if old is not None and not old.node_name and pod.node_name:  # bound by someone else
                old.node_name = pod.node_name
                old.containers = pod.containers
                self._charge(old, +1)
            return None
        if typ == "DELETED":
            old = known.get(pod.name)
            if old is not None:
                self.pods.remove(old)
                if old.node_name:
                    self._charge(old, -1)
            return None
        return None

    def failed_scheduling_message(self, pod: Pod, reasons) -> str:
        """The FailedScheduling event text (anchor/predicate.go:152-171): the pod line, then one
        "fit failure on node (%s): Insufficient X" line per non-fitting node in node-list order."""
        lines = [f"fit failure on node ({self.nodes[j].name}): {L.REASON_TEXT[int(r)]}"
                 for j, r in enumerate(reasons) if r != L.REASON_FIT]
        return f"pod ({pod.name}) failed to fit in any node\n" + "\n".join(lines)

    def _explain_failures(self, idx):
        """Per-node reasons of every NO_FIT pod of the call just made, each against the state it saw at
        its own turn -- reconstructed on the device from the call's placements (ksched_explain_pod),
        no host replay and no state change."""
        return {i: self.engine.explain_pod(i)[1] for i, x in enumerate(idx) if x == L.NO_FIT}

    def rank_pod(self, pod: Pod, k: int = 16, selector: Optional[int] = None):
        """The scheduler-extender filter + prioritize answer for one pod, without placing it (ksched_rank): its k
        best nodes in the scheduler's order as [(Node, score | price, reason text | None)].  The text (REASON_TEXT)
        is set only where a ranked node fails the predicate -- the all-node domain's quirk."""
        rc, rm, rp = pack_pods([pod])
        if selector is None:
            selector = self.selector_of(pod)
        sel = np.asarray([selector], dtype=np.uint64) if self.use_labels else None
        idx, score, reason, count, _ = self.engine.rank(rc, rm, rp, sel, k=k)
        return [(self.nodes[int(idx[0, r])], float(score[0, r]), L.REASON_TEXT.get(int(reason[0, r])))
                for r in range(int(count[0]))]

    def _dry_run_args(self, pod: Pod, selector: Optional[int]):
        """What rank_pod_full and explain_pod_full share: the spread, extended-resource and affinity tables reloaded
        from self.pods' bound pods with [pod] as the pending list (spread_tables, ext_tables, affinity_tables), as
        preempt_pod reloads its table.  Returns the pod's request, its selector array, the per-pod constraint arrays
        in Engine.rank_full's order and the extended resources' names."""
        bound = [p for p in self.pods if p.node_name]
        node_domain, skew, counts, group, enforce = spread_tables(self.nodes, bound, [pod])
        names, node_ext, req_ext = ext_tables(self.nodes, bound, [pod])
        t = affinity_tables(self.nodes, bound, [pod])
        self.engine.load_spread(node_domain, skew, counts)
        self.engine.load_ext(node_ext)
        self.engine.load_affinity(*t[:4])
        if selector is None:
            selector = self.selector_of(pod)
        sel = np.asarray([selector], dtype=np.uint64) if self.use_labels else None
        return pack_pods([pod]), sel, (group, enforce, req_ext) + tuple(t[4:]), names

    def rank_pod_full(self, pod: Pod, k: int = 16, selector: Optional[int] = None):
        """rank_pod under the pod's spread constraint, extended resources and affinity terms (ksched_rank_full): its k
        best nodes among those schedule_full would call eligible, as [(Node, score | price, reason text | None)].  The
        three tables are reloaded from self.pods' bound pods first; nothing is placed.  The text (REASON_TEXT_FULL, an
        extended column by its resource's name) is set only where a ranked node is not eligible -- the all-node
        domain's quirk."""
        (rc, rm, rp), sel, cons, names = self._dry_run_args(pod, selector)
        idx, score, reason, count, _, _ = self.engine.rank_full(rc, rm, rp, sel, k, *cons)
        return [(self.nodes[int(idx[0, r])], float(score[0, r]),
                 L.reason_text_full(int(reason[0, r]), names) if reason[0, r] != L.REASON_FIT else None)
                for r in range(int(count[0]))]

    def explain_pod_full(self, pod: Pod, selector: Optional[int] = None):
        """Why the pod fits where it does, constraints included (ksched_explain_full), against the current state: the
        three tables are reloaded from self.pods' bound pods first; nothing is placed and no event is posted.  Returns
        (counts int64[NUM_REASONS_FULL], message): the nodes per reason code, and the FailedScheduling text with one
        "fit failure on node (...): ..." line per node that is not eligible, in node-list order -- kube-scheduler's
        wordings (REASON_TEXT_FULL), the extended-resource lines naming the resource."""
        (rc, rm, rp), sel, cons, names = self._dry_run_args(pod, selector)
        group, enforce, req_ext, member, anti_host, anti_zone, aff_group, aff_zone = cons
        counts, reasons = self.engine.explain_full(
            int(rc[0]), int(rm[0]), int(rp[0]), 0 if sel is None else int(sel[0]), int(group[0]), bool(enforce[0]),
            req_ext[:, 0], int(member[0]), int(anti_host[0]), int(anti_zone[0]), int(aff_group[0]), bool(aff_zone[0]))
        lines = [f"fit failure on node ({self.nodes[j].name}): {L.reason_text_full(int(r), names)}"
                 for j, r in enumerate(reasons) if r != L.REASON_FIT]
        return counts, f"pod ({pod.name}) failed to fit in any node\n" + "\n".join(lines)

    def preempt_pod(self, pod: Pod, evict: bool = False, selector: Optional[int] = None):
        """kube-scheduler's default preemption for one pod that fits nowhere (ksched_preempt): the node on which the
        cheapest set of lower-priority bound pods would have to go, and those pods, most important first, as
        (Node, [victim Pods]); FitError when no node is a candidate.  The bound-pod table is reloaded from self.pods
        on every call.  evict=True also removes the victims -- through the DELETED path of handle_event, which gives
        their resources back to the node -- and appends one Preempted event per victim.  The pod is never bound: it
        is scheduled by the next schedule call, as kube-scheduler's nominated pods are."""
        bound = [p for p in self.pods if p.node_name]
        bc, bm, _ = pack_pods(bound)
        self.engine.load_bound([self._node_index(p.node_name) for p in bound], bc, bm, [p.priority for p in bound])
        rc, rm, rp = pack_pods([pod])
        if selector is None:
            selector = self.selector_of(pod)
        sel = np.asarray([selector], dtype=np.uint64) if self.use_labels else None
        node, nv, _, _, _, vic = self.engine.preempt(rc, rm, rp, sel, [pod.priority], vcap=L.BOUND_MAX_PER_NODE)
        return self._preempt_answer(pod, bound, node, nv, vic, evict)

    def preempt_pod_constrained(self, pod: Pod, evict: bool = False, selector: Optional[int] = None):
        """preempt_pod under the pod's extended-resource requests and spread constraint (ksched_preempt_constrained):
        a node counts, and a bound pod stays, only where the pod would also hold its extended requests and satisfy its
        spread constraint with the victims gone.  The spread and extended-resource tables and the bound-pod table --
        with each bound pod's extended amounts and group mask (bound_constraint_columns) -- are reloaded from self.pods
        (spread_tables, ext_tables) on every call.  Everything else is preempt_pod's: the answer, FitError, evict=True
        through the DELETED path with one Preempted event per victim, and the pod itself never bound."""
        bound = [p for p in self.pods if p.node_name]
        node_domain, skew, counts, group, enforce = spread_tables(self.nodes, bound, [pod])
        names, node_ext, req_ext = ext_tables(self.nodes, bound, [pod])
        bound_ext, bound_spread = bound_constraint_columns(bound, [pod], names)
        self.engine.load_spread(node_domain, skew, counts)
        self.engine.load_ext(node_ext)
        bc, bm, _ = pack_pods(bound)
        self.engine.load_bound_constrained([self._node_index(p.node_name) for p in bound], bc, bm,
                                           [p.priority for p in bound], bound_ext, bound_spread)
        rc, rm, rp = pack_pods([pod])
        if selector is None:
            selector = self.selector_of(pod)
        sel = np.asarray([selector], dtype=np.uint64) if self.use_labels else None
        node, nv, _, _, _, vic = self.engine.preempt_constrained(rc, rm, rp, sel, [pod.priority], group, enforce, req_ext,
                                                                 vcap=L.BOUND_MAX_PER_NODE)
        return self._preempt_answer(pod, bound, node, nv, vic, evict)

    def _preempt_answer(self, pod: Pod, bound: List[Pod], node, nv, vic, evict: bool):
        """A one-pod preemption answer as (Node, [victim Pods]), the victims evicted where asked (preempt_pod)."""
        if node[0] == L.NO_FIT:
            raise FitError(f"Unable to schedule pod ({pod.name}): no node fits it even without its lower-priority pods")
        target = self.nodes[int(node[0])]
        victims = [bound[int(t)] for t in vic[0, :int(nv[0])]]
        if evict:
            for v in victims:
                self.handle_event(dict(type="DELETED", object=dict(metadata=dict(name=v.name))))
                self.events.append(dict(reason="Preempted", type="Normal", involved=v.name,
                                        message=f"Preempted by pod ({pod.name}) on node {target.name}"))
        return target, victims

    def bind(self, pod: Pod, node: Node) -> None:
        """POST Binding + Scheduled event (anchor/schedule.go:200-261), in memory."""
        pod.node_name = node.name
        self.events.append(dict(reason="Scheduled", message=f"Successfully assigned {pod.name} to {node.name}"))

    def _resolve(self, pods, idx, why=None):
        """One engine call's per-pod results as the (pod, node | Exception) list, in order: NO_FIT posts a
        FailedScheduling event (with the per-node lines of why[k], where the call has them for pod k: its reason codes,
        or the finished text) and gives a FitError, NO_POSITIVE_SCORE a NilNodeError, any other index binds the pod to
        that node."""
        out = []
        for k, (pod, i) in enumerate(zip(pods, idx)):
            if i == L.NO_FIT:
                msg = ((why[k] if isinstance(why[k], str) else self.failed_scheduling_message(pod, why[k]))
                       if why and k in why else f"pod ({pod.name}) failed to fit in any node")
                self.events.append(dict(reason="FailedScheduling", message=msg, type="Warning",
                                        involved=pod.name))
                out.append((pod, FitError(f"Unable to schedule pod ({pod.name}) failed to fit in any node")))
            elif i == L.NO_POSITIVE_SCORE:
                out.append((pod, NilNodeError(pod.name)))
            else:
                node = self.nodes[int(i)]
                self.bind(pod, node)
                out.append((pod, node))
        return out

    def schedule_pods(self, pending: Optional[List[Pod]] = None, selectors=None):
        """schedulePods (anchor/schedule.go:185-197): one engine call resolves every pending pod in order;
        binds follow in the same order.  Returns a list of (pod, node | Exception).  By default the
        pending set is getUnscheduledPods' (unbound pods annotated for this scheduler,
        anchor/schedule.go:175-177); pass `pending` to schedule any other list (the watch path)."""
        pending = self.unscheduled_pods() if pending is None else pending
        rc, rm, rp = pack_pods(pending)
        if selectors is None and self.use_labels:
            selectors = [self.selector_of(p) for p in pending]
        sel = None if not self.use_labels else np.asarray(selectors, dtype=np.uint64)
        idx, score, feas = self.engine.schedule(rc, rm, rp, sel)
        return self._resolve(pending, idx, self._explain_failures(idx) if self.explain_failures else {})

    # the engine call of each set of constraints (gangs, spread, ext, affinity)
    _CONSTRAINED_CALLS = {(True, False, False, False): "schedule_gangs", (False, True, False, False): "schedule_spread",
                          (False, False, True, False): "schedule_ext", (False, False, False, True): "schedule_affinity",
                          (True, True, True, False): "schedule_constrained", (True, True, True, True): "schedule_full"}

    def _schedule_under(self, pending, gangs=False, spread=False, ext=False, affinity=False, why=False, node_rows=None):
        """What the constrained schedule_* methods share.  With gangs the pending pods are grouped first (group_gangs
        reorders them); the tables wanted are built for that list from self.pods' bound pods (spread_tables,
        ext_tables, affinity_tables), all of them before the first is loaded; then the one engine call those constraints
        have, with the per-pod arguments in its order, resolved through _resolve_gangs (gangs) or _resolve.  why: the
        call's _why form, with the per-node lines of the first node_rows pods that fit nowhere (None: all)."""
        pods = self.unscheduled_pods() if pending is None else pending
        off = gmin = names = None
        if gangs:
            pods, off, gmin = group_gangs(pods)
        bound = [p for p in self.pods if p.node_name]
        args, loads = ([off, gmin] if gangs else []), []
        if spread:
            node_domain, skew, counts, group, enforce = spread_tables(self.nodes, bound, pods)
            loads.append(lambda: self.engine.load_spread(node_domain, skew, counts))
            args += [group, enforce]
        if ext:
            names, node_ext, req_ext = ext_tables(self.nodes, bound, pods)
            loads.append(lambda: self.engine.load_ext(node_ext))
            args.append(req_ext)
        if affinity:
            t = affinity_tables(self.nodes, bound, pods)
            loads.append(lambda: self.engine.load_affinity(*t[:4]))
            args += t[4:]
        for load in loads:
            load()
        rc, rm, rp = pack_pods(pods)
        sel = np.asarray([self.selector_of(p) for p in pods], dtype=np.uint64) if self.use_labels else None
        call = getattr(self.engine, self._CONSTRAINED_CALLS[gangs, spread, ext, affinity] + ("_why" if why else ""))
        texts = None
        if why:
            rows = len(pods) if node_rows is None else min(int(node_rows), len(pods))
            idx, _, _, placed, (wpod, _, reasons, _) = call(rc, rm, rp, sel, *args, why_rows=rows, node_rows=rows)
            texts = {}
            for r in range(0 if reasons is None else len(reasons)):
                k = int(wpod[r])
                lines = [f"fit failure on node ({self.nodes[j].name}): {L.reason_text_full(int(c), names)}"
                         for j, c in enumerate(reasons[r]) if c != L.REASON_FIT]
                texts[k] = f"pod ({pods[k].name}) failed to fit in any node\n" + "\n".join(lines)
        else:
            idx, _, _, *placed = call(rc, rm, rp, sel, *args)
            placed = placed[0] if gangs else None
        return self._resolve_gangs(pods, off, gmin, idx, placed, texts) if gangs else self._resolve(pods, idx)

    def schedule_gangs(self, pending: Optional[List[Pod]] = None):
        """schedule_pods with pod groups (group_gangs; ksched_schedule_gangs): one engine call resolves every gang
        in order.  An accepted gang's placed members are bound in order; a rejected gang binds nothing and posts one
        FailedScheduling event per member.  Returns (pod, node | Exception) in the gangs' order -- GangRejected for
        a member that found a node in a rejected gang.  (No per-node "fit failure" lines: a rolled-back gang
        leaves no placements to rebuild a pod's state from; schedule_full_why collects them at the pod's turn.)"""
        return self._schedule_under(pending, gangs=True)

    def _resolve_gangs(self, pods, off, gmin, idx, placed, why=None):
        """A gang call's per-pod results, gang by gang, as the (pod, node | Exception) list (see schedule_gangs).  why:
        the FailedScheduling text of the NO_FIT pods the call has one for, by position in pods (schedule_full_why)."""
        out = []
        for g in range(len(gmin)):
            lo, hi = int(off[g]), int(off[g + 1])
            gname = pods[lo].annotations.get(GROUP_NAME_ANNOTATION) or pods[lo].name
            found = int(np.sum((idx[lo:hi] >= 0) | (idx[lo:hi] == L.GANG_REJECTED)))
            rejected = found < int(gmin[g])
            assert int(placed[g]) == (0 if rejected else found)
            for k, (pod, i) in enumerate(zip(pods[lo:hi], idx[lo:hi]), lo):
                if i == L.GANG_REJECTED:
                    msg = (f"pod ({pod.name}) rejected with its gang ({gname}): {found} of {hi - lo} members placed, "
                           f"{int(gmin[g])} needed")
                    self.events.append(dict(reason="FailedScheduling", message=msg, type="Warning", involved=pod.name))
                    out.append((pod, GangRejected(msg)))
                    continue
                if i == L.NO_POSITIVE_SCORE and rejected:
                    self.events.append(dict(reason="FailedScheduling", type="Warning", involved=pod.name,
                                            message=f"pod ({pod.name}) found no node with a positive score"))
                out += self._resolve([pod], [i], {0: why[k]} if why and k in why else None)
        return out

    def schedule_spread(self, pending: Optional[List[Pod]] = None):
        """schedule_pods under the pending pods' topology spread constraints (spread_tables;
        ksched_schedule_spread): the spread table is reloaded from self.pods' bound pods on every call, then one
        engine call resolves every pending pod in order and the binds follow.  Returns (pod, node | Exception); a
        pod that fits nowhere its constraint allows gets the usual FailedScheduling event (without per-node lines: the at-its-turn explain
        calls know no spread reason; explain_pod_full gives them against the current state, schedule_full_why at the
        pod's turn)."""
        return self._schedule_under(pending, spread=True)

    def schedule_affinity(self, pending: Optional[List[Pod]] = None):
        """schedule_pods under the pods' required inter-pod affinity and anti-affinity terms (affinity_tables;
        ksched_schedule_affinity): the affinity table is reloaded from self.pods' bound pods on every call, then one
        engine call resolves every pending pod in order and the binds follow.  Returns (pod, node | Exception); a pod
        that fits nowhere its terms allow gets the usual FailedScheduling event (without per-node lines: the at-its-turn
        explain calls know no affinity reason; explain_pod_full gives them against the current state, schedule_full_why
        at the pod's turn)."""
        return self._schedule_under(pending, affinity=True)

    def schedule_ext(self, pending: Optional[List[Pod]] = None):
        """schedule_pods with the pending pods' extended resources (ext_tables; ksched_schedule_ext) in the fit
        predicate: the table is reloaded from self.pods' bound pods on every call, then one engine call resolves every
        pending pod in order and the binds follow.  Returns (pod, node | Exception); a pod that fits nowhere gets the
        usual FailedScheduling event (without per-node lines: the at-its-turn explain calls know no extended-resource
        reason; explain_pod_full gives them against the current state, schedule_full_why at the pod's turn)."""
        return self._schedule_under(pending, ext=True)

    def schedule_constrained(self, pending: Optional[List[Pod]] = None):
        """schedule_gangs, schedule_spread and schedule_ext in one engine call (ksched_schedule_constrained): the
        pending pods are grouped into their gangs first (group_gangs reorders them), the spread and extended-resource
        tables are built for the reordered list (spread_tables, ext_tables) and reloaded from self.pods' bound pods,
        and one launch resolves every gang in order -- a rejected gang gives back the extended resources it took and
        the spread counts it raised.  Resolved gang by gang exactly as schedule_gangs does: binds, GangRejected and
        events."""
        return self._schedule_under(pending, gangs=True, spread=True, ext=True)

    def schedule_full(self, pending: Optional[List[Pod]] = None):
        """schedule_constrained and schedule_affinity in one engine call (ksched_schedule_full): the pending pods are
        grouped into their gangs first (group_gangs reorders them), the spread, extended-resource and affinity tables
        are built for the reordered list (spread_tables, ext_tables, affinity_tables) and reloaded from self.pods' bound
        pods, and one launch resolves every gang in order -- a rejected gang gives back the extended resources it took,
        the spread counts it raised and the affinity words it set.  Resolved gang by gang exactly as schedule_gangs
        does: binds, GangRejected and events."""
        return self._schedule_under(pending, gangs=True, spread=True, ext=True, affinity=True)

    def schedule_full_why(self, pending: Optional[List[Pod]] = None, node_rows: Optional[int] = None):
        """schedule_full whose FailedScheduling events carry the reference's per-node lines (ksched_schedule_full_why):
        for every pod that fits nowhere -- a member of a gang included, accepted or rejected -- one "fit failure on node
        (...): ..." line per node with the reason the pod saw AT ITS TURN, the tentative placements of its own gang
        included, in kube-scheduler's wordings (REASON_TEXT_FULL, an extended column by its resource's name).
        node_rows: the number of such pods that get the lines (None: all of them); the others get the plain event.
        Everything else -- tables, order, binds, GangRejected, return value -- is schedule_full's."""
        return self._schedule_under(pending, gangs=True, spread=True, ext=True, affinity=True, why=True,
                                    node_rows=node_rows)

    def schedule_pod(self, pod: Pod, selector: Optional[int] = None):
        """schedulePod (anchor/schedule.go:68-89) for a single pod."""
        if selector is None:
            selector = self.selector_of(pod)
        res = self.schedule_pods([pod], selectors=[selector] if self.use_labels else None)[0][1]
        if isinstance(res, Exception):
            raise res
        return res
