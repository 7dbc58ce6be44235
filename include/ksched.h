/*
 * ksched.h -- C ABI of the MI355X-native scheduling core (libksched.so).
 *
 * Drop-in boundary for the hot path of yinwoods/k8s-scheduler (paths relative to the reference):
 *   func predicate(pod *Pod) ([]*Node, error)              anchor/predicate.go:107-176
 *   func priorities(pod *Pod, nodes []*Node) (*Node, error) anchor/priorities.go:25-63
 *   the per-pod commit that the next pod observes           anchor/schedule.go:68-89, 185-197
 *                                                           (used += request, anchor/predicate.go:83-105)
 * The Go caller keeps getNodes/getPods (anchor/tools.go:53-108) and bind/postEvent
 * (anchor/schedule.go:200-261) unchanged; see INTEGRATION.md for the cgo shim.
 *
 * Plain C types only.  Caller-owned arrays are read (or written) during the call only and never
 * retained, so Go slices of scalars may be passed directly under the cgo pointer rules.
 * Every function returns an int status (KSCHED_OK == 0), never throws across the ABI and never
 * exits the process.  A context is not reentrant: callers serialise calls on one context exactly as
 * the reference serialises schedulePod under processorLock (anchor/schedule.go:29,55,186).
 */
#ifndef KSCHED_H
#define KSCHED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSCHED_ABI_VERSION 6

/* status codes */
#define KSCHED_OK 0
#define KSCHED_E_INVALID (-1)   /* bad argument / shape / option */
#define KSCHED_E_DEVICE (-2)    /* HIP or RCCL failure, or a device-side timeout */
#define KSCHED_E_PARSE (-3)     /* the reference's errFatal parse paths (anchor/predicate.go:15,31,39,49) */
#define KSCHED_E_STATE (-4)     /* call out of order (e.g. schedule before load_nodes) */
#define KSCHED_E_NOMEM (-5)
#define KSCHED_E_UNKNOWN_NODE (-6) /* a bound pod names a node not in the node list (reference: nil deref panic, anchor/predicate.go:94-99) */

/* per-pod outcome in out_idx[] */
#define KSCHED_NO_FIT (-1)            /* predicate found no node: reference returns "failed to fit" (anchor/schedule.go:74-76) */
#define KSCHED_NO_POSITIVE_SCORE (-2) /* no node scored > 0: reference binds a nil node and panics (anchor/priorities.go:55-62, anchor/schedule.go:208); documented divergence */
#define KSCHED_GANG_REJECTED (-3)     /* ksched_schedule_gangs only: the pod found a node, but too few members of its gang did; its commit was undone */

/* options */
#define KSCHED_MODE_EXACT 0     /* pod-by-pod: one full node scan + grid-wide arg-best per pod (persistent kernel) */
#define KSCHED_MODE_BATCHED 1   /* speculative top-K for a batch of pods + ordered commit with exact re-score */
#define KSCHED_MODE_AUTO 2

#define KSCHED_PRIORITY_RESOURCE 0    /* (balanced + least-requested) / 2, anchor/priorities.go:45-50 */
#define KSCHED_PRIORITY_BEST_PRICE 1  /* lowest node price among feasible nodes (README.md:37-64; build-defined) */

/* ordered-commit implementations (batched mode; all produce the sequential result) */
#define KSCHED_COMMIT_SEQUENTIAL 1    /* one wave re-scores the touched set per pod (batch <= 128) */
#define KSCHED_COMMIT_LANE_PER_POD 2  /* retired (round 1 variant): treated as KSCHED_COMMIT_SPECULATIVE */
#define KSCHED_COMMIT_SPECULATIVE 3   /* guess first touches, check all pods in parallel, resolve the first miss (batch <= 64) */

/* batched-mode pipelines (all produce the same results) */
#define KSCHED_PIPELINE_AUTO 0    /* the persistent kernel where the configuration fits it, else the stream pipeline */
#define KSCHED_PIPELINE_STREAM 1  /* always the stream pipeline (per-batch score / merge / commit launches) */

#define KSCHED_DOMAIN_ALL 0       /* argmax over ALL nodes, feasible or not (the reference, anchor/priorities.go:45) */
#define KSCHED_DOMAIN_FEASIBLE 1  /* argmax over feasible nodes only (build extension) */

typedef struct ksched_opts {
    int32_t struct_size; /* = sizeof(ksched_opts) */
    int32_t mode;        /* KSCHED_MODE_* */
    int32_t priority;    /* KSCHED_PRIORITY_* */
    int32_t domain;      /* KSCHED_DOMAIN_* (best-price always ranges over feasible nodes) */
    int32_t use_labels;  /* 1: feasible &= (node_labels & pod_selector) == pod_selector (build extension) */
    int32_t batch;       /* batched mode: pods per speculative batch (0 = auto) */
    int32_t topk;        /* batched mode: candidates kept per pod, one of 4, 8, 16 (0 = auto) */
    int32_t device;      /* HIP device ordinal (-1 = current) */
    /* node sharding across ranks (multi-GPU); single GPU: rank 0, nranks 1 */
    int32_t rank;
    int32_t nranks;
    int64_t node_offset;  /* global index of this rank's first node */
    int64_t nodes_global; /* total nodes across ranks (0 = local count when nranks == 1) */
    int32_t exact_wgs;    /* exact mode: workgroups (0 = auto) */
    int32_t timing;       /* 1: time kernel families with HIP events on the engine stream (sampled) */
    int32_t timing_every; /* batched mode: time one batch in every N (0 = 16) */
    int32_t chunk_topk;   /* batched mode: candidates kept per node chunk before the merge, 2/4/8/16 (0 = auto);
                             capped at topk.  The merge keeps the exact prefix. */
    int32_t commit_impl;  /* batched mode: KSCHED_COMMIT_* (0 = auto: speculative when batch <= 64) */
    int32_t pipeline;     /* batched mode: KSCHED_PIPELINE_AUTO (0) or KSCHED_PIPELINE_STREAM (ABI 4) */
    int32_t pipe_wgs;     /* persistent pipeline: at most this many workgroups, one per CU (0 = every CU).
                             The launch is always cooperative (the runtime admits the grid only if every
                             workgroup is resident at once); ranks that share ONE device are joined by
                             ksched_xchg_join_local and split its CUs in one such launch. (ABI 4) */
    int32_t reserved[1];
} ksched_opts;

typedef struct ksched_ctx ksched_ctx;

typedef struct ksched_stats {
    int64_t pods;          /* pods resolved by the last schedule call */
    int64_t placed;        /* pods bound to a node */
    int64_t batches;       /* speculative batches launched (batched mode) */
    int64_t truncations;   /* batches cut short by a candidate-list overflow */
    int64_t pair_evals;    /* pod-node pairs evaluated by the score kernels */
    double device_ms;      /* device time of the last schedule call (HIP events) */
    double kernel_ms[4];   /* timed device ms per kernel family: [0] score (or the exact kernel),
                              [1] merge, [2] commit, [3] collective (all-gather + rank merge) */
    int64_t kernel_launches[4]; /* number of timed batches (launch groups) behind kernel_ms */
    int64_t kernel_pairs[4];    /* pod-node pairs evaluated by the timed family-0 launches */
    int64_t pipeline;           /* which device pipeline ran the last call: KSCHED_PIPE_* (ABI 2) */
    int64_t rescues;            /* persistent pipeline (ABI 5): exhausted candidate lists resolved by a full scan
                                   of the untouched nodes instead of truncating their batch */
    int64_t exact_rows;         /* persistent pipeline: node rows scored exactly (f64) by the score workgroups,
                                   summed over batches -- the screened scan's survivors plus unscreened batches */
    int64_t scan_rows;          /* ... and node rows scanned (each row once per active batch) */
} ksched_stats;

enum {
    KSCHED_PIPE_NONE = 0,       /* no pods */
    KSCHED_PIPE_EXACT = 1,      /* the exact persistent kernel, one pod at a time */
    KSCHED_PIPE_STREAM = 2,     /* batched: score / merge / speculative commit kernels per batch, stream-linked */
    KSCHED_PIPE_STREAM_SEQ = 3, /* batched with the sequential one-pod-at-a-time commit kernel */
    KSCHED_PIPE_PERSISTENT = 4  /* batched: ONE persistent kernel (commit workgroup + score/merge workgroups) */
};

/* ---- lifecycle ---- */
int ksched_abi_version(void);
int ksched_default_opts(ksched_opts *opts);
int ksched_create(const ksched_opts *opts, ksched_ctx **out);
int ksched_destroy(ksched_ctx *ctx);
const char *ksched_last_error(const ksched_ctx *ctx); /* never NULL; "" when no error */

/* Multi-GPU: rank 0 creates a 128-byte RCCL unique id; every rank passes it to ksched_set_comm
 * before the first schedule call (opts.nranks > 1). */
int ksched_get_unique_id(uint8_t out_id[128]);
int ksched_set_comm(ksched_ctx *ctx, const uint8_t id[128]);

/* In-process rank group: the same node-sharded batched path with R contexts of ONE process on ONE
 * device (one host thread per context), the per-batch all-gather done by host-coordinated device
 * copies instead of RCCL (RCCL admits one rank per device).  It runs the multi-rank code on a single
 * GPU (a test vehicle, one host round trip per batch); contexts set opts.rank / nranks / node_offset /
 * nodes_global as for ksched_set_comm, call ksched_set_group instead of it, and must run the same
 * schedule calls concurrently. */
/* Device-side candidate exchange for the node-sharded batched path (one process per GPU, 2..8 ranks,
 * batch <= 64): instead of one RCCL all-gather per batch launched from the host, the persistent
 * pipeline's merger workgroups write each pod's candidate list straight into every rank's receive
 * ring over xGMI (tagged 8-byte granules in uncached device memory) and rank-merge the R lists they
 * receive -- no launch, no host round trip, no collective per batch.  Setup, on every rank:
 *   ksched_xchg_export(ctx, h)          allocates (or reuses) this rank's ring and zeroes it (a device kernel
 *                                       of system-scope stores, the granules' own path) at EVERY export;
 *                                       h = its IPC handle and the first granule tag this process has never
 *                                       used (128 bytes)
 *   (all-gather the R blobs in rank order, e.g. torch.distributed)
 *   ksched_xchg_import(ctx, handles)    maps every rank's ring (R * 128 bytes, own entry ignored); the tags
 *                                       of the setup start at the largest of the R hints, so no tag repeats
 *                                       in any process's memory
 * Batched runs then take the exchange path on every rank (an RCCL communicator is optional: it is
 * the fallback when a device timeout disables the exchange; ksched_xchg_ready reports the state).
 * Replaces the same all-gather as ksched_set_comm; the call sequence is unchanged. */
#define KSCHED_XCHG_HANDLE_BYTES 128
int ksched_xchg_export(ksched_ctx *ctx, uint8_t handle[KSCHED_XCHG_HANDLE_BYTES]);
int ksched_xchg_import(ksched_ctx *ctx, const uint8_t *handles);
int ksched_xchg_ready(const ksched_ctx *ctx);
/* Turns the exchange off on this rank (later batched calls take the RCCL path).  Every rank calls it when
 * any rank failed to import (ABI 4): the ranks must agree on the transport. */
int ksched_xchg_close(ksched_ctx *ctx);
/* Ranks as threads of ONE process on ONE device (ABI 5): joins ctxs[0..n-1] (rank r at ctxs[r], each created
 * with nranks = n, 2 <= n <= 8, batch <= 64 and the same options) into the device exchange.  Their persistent
 * pipelines then run as ONE cooperative launch -- rank r's workgroups a contiguous block range, the ranks sharing
 * the CUs equally -- so every rank's grid is resident at once by construction; separate launches (of separate
 * processes) sharing a device guarantee no such thing.  The contexts' threads call
 * ksched_run concurrently, as with ksched_set_group; destroy all of them together.  Every rank's grid must fit
 * its share of the CUs: at 8 ranks on one MI355X (31 CUs each) that needs batch <= 32.
 * ksched_xchg_join_local_ex (ABI 6) takes flags: KSCHED_XCHG_RINGS_UNCACHED allocates the rings exactly as
 * ksched_xchg_export does (hipDeviceMallocUncached, zeroed at every setup, tags from the process's next unused
 * one); KSCHED_XCHG_RINGS_IPC
 * (implies UNCACHED) also maps every peer's ring through its IPC handle, as ksched_xchg_import does -- the
 * multi-process transport's allocation, zeroing, handles and epoch rule on one device (it fails where the
 * runtime does not open a handle of the same process). */
int ksched_xchg_join_local(ksched_ctx *const *ctxs, int32_t n);
#define KSCHED_XCHG_RINGS_UNCACHED 1
#define KSCHED_XCHG_RINGS_IPC 2
int ksched_xchg_join_local_ex(ksched_ctx *const *ctxs, int32_t n, int32_t flags);

typedef struct ksched_group ksched_group;
int ksched_group_create(int32_t nranks, int32_t device, ksched_group **out);
int ksched_group_destroy(ksched_group *g); /* after every context using it is destroyed */
int ksched_set_group(ksched_ctx *ctx, ksched_group *g);

/* ---- node state (allocatable = capacity - used, anchor/predicate.go:56-67) ---- */
/* Loads this rank's n nodes (node order = nodeList.Items order).  labels / price may be NULL
 * unless the options need them.  Prices must be finite. */
int ksched_load_nodes(ksched_ctx *ctx, int64_t n, const int64_t *alloc_cpu, const int64_t *alloc_mem,
                      const int64_t *alloc_pods, const uint64_t *labels, const float *price);
/* alloc[node_idx[i]] += (d_cpu[i], d_mem[i], d_pods[i]) for binds / deletions made by others,
 * or to undo a bind that failed (anchor/schedule.go:200-237).  node_idx is local to this rank. */
int ksched_apply_delta(ksched_ctx *ctx, int64_t k, const int32_t *node_idx, const int64_t *d_cpu,
                       const int64_t *d_mem, const int64_t *d_pods);
/* FailedScheduling diagnostics (anchor/predicate.go:127-157): evaluates the predicate of ONE pod
 * against the current (local) node state and reports, per node, the first failing check in the
 * reference's order -- the "fit failure on node (%s): Insufficient CPU|Memory|Pod" lines of the
 * FailedScheduling event -- then the build-defined label check.  out_counts[KSCHED_REASON_*] counts
 * nodes per outcome (out_counts[KSCHED_REASON_FIT] == the pod's feasible count); out_reason (n_local
 * bytes, may be NULL) receives each node's code.  Multi-rank: counts cover this rank's shard. */
#define KSCHED_REASON_FIT 0
#define KSCHED_REASON_CPU 1     /* "Insufficient CPU"    anchor/predicate.go:134-138 */
#define KSCHED_REASON_MEMORY 2  /* "Insufficient Memory" anchor/predicate.go:139-143 */
#define KSCHED_REASON_POD 3     /* "Insufficient Pod"    anchor/predicate.go:144-148 */
#define KSCHED_REASON_LABELS 4  /* label selector not satisfied (build extension) */
#define KSCHED_NUM_REASONS 5
int ksched_explain(ksched_ctx *ctx, int64_t req_cpu, int64_t req_mem, int64_t req_pods, uint64_t selector,
                   int64_t out_counts[KSCHED_NUM_REASONS], uint8_t *out_reason);
/* The same diagnostics for EVERY pod of the last schedule call (ksched_schedule / ksched_run) that
 * ended KSCHED_NO_FIT, each against the node state it saw at its turn -- the state after the
 * placements of all pods before it (anchor/schedule.go:185-197 re-reads the cluster per pod) -- with
 * no host replay: out_counts[i * KSCHED_NUM_REASONS + r] for pod i (rows of the other pods are
 * zero); *out_nofit (may be NULL) = their number.  Valid only while the last call's placements are
 * the last change to the node state (KSCHED_E_STATE after load_nodes / apply_delta / restore_state /
 * upload_pods).  Multi-rank: counts cover this rank's shard (sum them over ranks). */
int ksched_explain_batch(ksched_ctx *ctx, int64_t p, int64_t *out_counts, int64_t *out_nofit);
/* Per-node reasons of pod `pod` of the last schedule call at its turn: the "fit failure on node"
 * lines of its FailedScheduling event (out_reason: n_local bytes, may be NULL). */
int ksched_explain_pod(ksched_ctx *ctx, int64_t pod, int64_t out_counts[KSCHED_NUM_REASONS], uint8_t *out_reason);
/* ---- ranked dry run (added within ABI 6: probe with dlsym(lib, "ksched_rank"), the version number did not move) ----
 * For each of m pod shapes, the k best nodes the scheduler would choose among if that pod were next, against
 * the current (local) node state: the scheduler-extender filter + prioritize verbs, "why this node and not
 * that one", capacity what-ifs.  Every pod is evaluated on its own; NOTHING is committed and nothing else a
 * context holds changes (node rows, staged pods, the last call's results, ksched_explain_batch's validity).
 * Entry r of pod i (out_*[i * k + r]) is its r-th best ELIGIBLE node in the scheduler's own order -- key
 * descending, global index ascending.  Eligible: resource priority, score > 0 (and feasible under
 * KSCHED_DOMAIN_FEASIBLE); best-price, feasible, ranked by price ascending.  So entry 0 is what ksched_schedule
 * would pick for that pod, count == 0 && feasible == 0 is KSCHED_NO_FIT and count == 0 && feasible > 0 is
 * KSCHED_NO_POSITIVE_SCORE.  Under KSCHED_DOMAIN_ALL a ranked node may fail the predicate (the reference's
 * argmax over all nodes): out_reason shows it, the first failing check in ksched_explain's order.
 *   out_idx      m*k  node index (global across ranks); -1 past out_count[i]
 *   out_score    m*k  the score (resource priority) or the price (best-price), bit for bit the scheduler's; 0 past the end
 *   out_reason   m*k  KSCHED_REASON_* of that node for that pod (KSCHED_REASON_FIT past the end)
 *   out_count    m    valid entries, <= k
 *   out_feasible m    nodes passing predicate()
 * 1 <= k <= KSCHED_RANK_MAX; m >= 0 (large m is served in chunks: the device workspace stays below 20 MiB);
 * selector may be NULL unless opts.use_labels; any output pointer may be NULL.  The call waits for the
 * context's stream first, as ksched_explain does.  Multi-rank: the lists cover this rank's shard. */
#define KSCHED_RANK_MAX 64
int ksched_rank(ksched_ctx *ctx, int64_t m, const int64_t *req_cpu, const int64_t *req_mem, const int64_t *req_pods,
                const uint64_t *selector, int32_t k, int32_t *out_idx, double *out_score, uint8_t *out_reason,
                int32_t *out_count, int32_t *out_feasible);
/* Host only (no context, no GPU; added within ABI 6 with ksched_rank): merges the lists nranks node shards
 * returned for the same m pods and k -- idx_all / score_all / reason_all [rank][m][k], count_all / feasible_all
 * [rank][m] -- into the global lists, in the same order (best-price: price ascending); out_feasible is the sum
 * over the shards.  reason_all, feasible_all and any output pointer may be NULL. */
int ksched_rank_merge(int32_t priority, int32_t nranks, int64_t m, int32_t k, const int32_t *idx_all,
                      const double *score_all, const uint8_t *reason_all, const int32_t *count_all,
                      const int32_t *feasible_all, int32_t *out_idx, double *out_score, uint8_t *out_reason,
                      int32_t *out_count, int32_t *out_feasible);
/* ---- preemption dry run (added within ABI 6: probe with dlsym(lib, "ksched_preempt"), the version number did not move) ----
 * kube-scheduler's default preemption (the PostFilter step) without PDBs and start times: for a pod that fits
 * nowhere, which lower-priority bound pods would have to go, and on which node.  A build extension: the reference
 * knows no priorities.
 *
 * ksched_load_bound: the table of bound pods, a snapshot the caller owns.  Pod t of the table (its TABLE INDEX, the
 * name every answer uses) is bound to local node node_idx[t], holds (cpu[t], mem[t]) and one pod slot there -- what
 * its commit subtracted from the node's row -- and has priority prio[t].  Call it after ksched_load_nodes.  nb == 0
 * is a valid, empty table.  KSCHED_E_INVALID: a node index outside [0, n_local), or more than
 * KSCHED_BOUND_MAX_PER_NODE pods on one node; KSCHED_E_NOMEM: the table could not be allocated (the context then
 * holds no table).  The call changes no node row and nothing else the context holds.  ksched_load_nodes
 * invalidates the table (ksched_preempt returns KSCHED_E_STATE until it is loaded again); schedule calls,
 * ksched_apply_delta and ksched_restore_state leave it alone -- they move the rows, and keeping the table in step
 * with them is the caller's business (FakeCluster.preempt_pod reloads it on every call).
 *
 * ksched_preempt: each of the m pods is evaluated on its own against the current (local) rows and the table.
 * NOTHING is committed and nothing else a context holds changes -- ksched_rank's promise.  Sums are wrapping int64;
 * fits is the scheduler's predicate, the label check included under opts.use_labels.  Per pod i and node j:
 *   1. potential victims: the table's pods on j with prio < prio[i].  Importance order: priority descending, then
 *      table index ascending (earlier = older = more important).
 *   2. free = alloc[j] + sum of (cpu, mem, 1) over the potential victims.  !fits(req[i], free): j is no candidate.
 *   3. reprieve: walk the potential victims, most important first.  fits(req[i], free - v): free -= v, v is
 *      reprieved; otherwise v is a victim.
 *   4. the node's key: (max victim prio, sum of (prio + 2^31) over the victims as int64, victim count); the max is
 *      KSCHED_PREEMPT_NO_VICTIM_PRIO without a victim (pickOneNodeForPreemption's order).
 * The chosen node is the candidate with the lexicographically smallest key, then the lowest global index: a node
 * that fits already has no victim and wins.  Outputs per pod (any pointer may be NULL):
 *   out_node       global node index, or KSCHED_NO_FIT when no node is a candidate (the next three are then 0,
 *                  KSCHED_PREEMPT_NO_VICTIM_PRIO, 0 and the pod's victim row all -1)
 *   out_nvictims   the chosen node's victim count, in full even above vcap
 *   out_max_prio, out_sum_prio   the chosen key
 *   out_candidates candidate nodes of this rank's shard
 *   out_victims    m*vcap: out_victims[i * vcap + r] = table index of the chosen node's r-th victim in step 3's order,
 *                  at most vcap of them, -1 past the end
 * 1 <= vcap <= KSCHED_BOUND_MAX_PER_NODE; m >= 0 (large m is served in chunks with a bounded device workspace);
 * selector may be NULL unless opts.use_labels.  The call waits for the context's stream first.  Multi-rank: the
 * answer covers this rank's shard (ksched.dist.merge_preempt picks among the shards' answers). */
#define KSCHED_BOUND_MAX_PER_NODE 1024
#define KSCHED_PREEMPT_NO_VICTIM_PRIO INT32_MIN
int ksched_load_bound(ksched_ctx *ctx, int64_t nb, const int32_t *node_idx, const int64_t *cpu, const int64_t *mem,
                      const int32_t *prio);
int ksched_preempt(ksched_ctx *ctx, int64_t m, const int64_t *req_cpu, const int64_t *req_mem, const int64_t *req_pods,
                   const uint64_t *selector, const int32_t *prio, int32_t vcap, int32_t *out_node, int32_t *out_nvictims,
                   int32_t *out_max_prio, int64_t *out_sum_prio, int32_t *out_candidates, int32_t *out_victims);
/* Copies the current (local) node state back to the host. */
int ksched_read_nodes(ksched_ctx *ctx, int64_t n, int64_t *alloc_cpu, int64_t *alloc_mem, int64_t *alloc_pods);
/* Device-side snapshot / restore of the node state (bench: identical start state every step). */
int ksched_save_state(ksched_ctx *ctx);
int ksched_restore_state(ksched_ctx *ctx);

/* ---- scheduling: schedulePods over p pending pods, in order (anchor/schedule.go:185-197) ----
 * req_pods is the container count (anchor/predicate.go:78); each placed pod commits
 * alloc[node] -= (req_cpu, req_mem, 1) (anchor/predicate.go:102).  Outputs per pod:
 *   out_idx      node index (global across ranks) | KSCHED_NO_FIT | KSCHED_NO_POSITIVE_SCORE
 *   out_score    winning score (resource priority) or price (best-price); 0 when not placed
 *   out_feasible number of nodes passing predicate() for that pod at its turn
 * Any output pointer may be NULL. */
int ksched_schedule(ksched_ctx *ctx, int64_t p, const int64_t *req_cpu, const int64_t *req_mem,
                    const int64_t *req_pods, const uint64_t *selector,
                    int32_t *out_idx, double *out_score, int32_t *out_feasible);

/* ---- gang scheduling (added within ABI 6: probe with dlsym(lib, "ksched_schedule_gangs"); ksched_stats did not change) ----
 * The same p pods in all-or-nothing groups (Kubernetes coscheduling, PodGroup.minMember), resolved by ONE launch of
 * the exact kernel whatever opts.mode says (stats.pipeline == KSCHED_PIPE_EXACT).  A build extension: the reference's
 * schedulePods (anchor/schedule.go:185-197) knows no groups.
 *   gang_off  n_gangs + 1 CSR offsets (the idiom of cont_off below): gang_off[0] == 0, gang_off[n_gangs] == p,
 *             strictly increasing (no empty gang); gang g is pods [gang_off[g], gang_off[g + 1]), at most
 *             KSCHED_GANG_MAX of them
 *   gang_min  n_gangs minimum members, 1 <= gang_min[g] <= size; NULL: every member is required
 * Gangs are processed in order and members in order within a gang.  Every member is evaluated exactly as
 * ksched_schedule evaluates a pod in exact mode, against the current state -- which includes the tentative
 * placements of the earlier members of its own gang -- and is tentatively committed as usual (alloc -= (req_cpu,
 * req_mem, 1), wrapping).  No member is skipped, even after an earlier member of its gang failed, so every pod's
 * out_feasible is defined.  A member counts as placed when its outcome is a node index (>= 0; under
 * KSCHED_DOMAIN_ALL that node may fail the predicate, as in the reference).  At the end of gang g:
 *   placed >= gang_min[g]: accepted.  The commits stand; members that failed keep KSCHED_NO_FIT /
 *     KSCHED_NO_POSITIVE_SCORE.
 *   placed <  gang_min[g]: rejected.  Every tentative commit of the gang is undone (a wrapping add): the node rows
 *     are bit-identical to the rows before the gang.  Members that had been placed get out_idx =
 *     KSCHED_GANG_REJECTED and out_score = 0; members that failed keep their own code -- the reason the gang
 *     failed; out_feasible keeps the count each member saw at its turn.
 *   out_gang_placed[g] (may be NULL) = members bound: 0 for a rejected gang.
 * A call whose gangs all have size 1 is ksched_schedule in exact mode.  KSCHED_E_INVALID (nothing changed): a gang
 * above KSCHED_GANG_MAX, bad offsets or minima, opts.nranks > 1.  Afterwards ksched_explain_batch /
 * ksched_explain_pod return KSCHED_E_STATE (they rebuild a pod's state from final placements, which a rolled-back
 * gang does not have: ksched_schedule_full_why below collects a pod's reasons inside the run, at its turn); after a
 * device error the node state is as unspecified as after a failed ksched_schedule. */
#define KSCHED_GANG_MAX 1024
int ksched_schedule_gangs(ksched_ctx *ctx, int64_t p, const int64_t *req_cpu, const int64_t *req_mem,
                          const int64_t *req_pods, const uint64_t *selector, int64_t n_gangs, const int64_t *gang_off,
                          const int32_t *gang_min, int32_t *out_idx, double *out_score, int32_t *out_feasible,
                          int32_t *out_gang_placed);

/* ---- topology spread (added within ABI 6: probe with dlsym(lib, "ksched_schedule_spread"); the version number did not move) ----
 * Pod topology spread constraints (topologySpreadConstraints with whenUnsatisfiable: DoNotSchedule) over ONE topology
 * key, resolved by ONE launch of the exact kernel whatever opts.mode says (stats.pipeline == KSCHED_PIPE_EXACT,
 * stats.pair_evals == p * n).  A build extension: the reference knows no constraints.
 *
 * The table (ksched_load_spread, after ksched_load_nodes): n_domains = D domains of the key and n_groups = S groups.
 *   node_domain[j] in [0, D): node j's domain (its zone; its own index for hostname spread); -1: the node does not
 *                  carry the key
 *   a group        the pods one constraint's label selector matches
 *   counts[s*D+d]  the number of such pods already bound in domain d (NULL: all zero)
 *   max_skew[s]    >= 1
 * Pods: spread_group[i] in [-1, S), -1: the pod belongs to no group.  spread_enforce[i] != 0 (NULL: every pod): the
 * pod must satisfy its group's constraint; == 0: the pod only counts -- it matches the selector but carries no
 * constraint itself.  The flag is ignored where the group is -1.
 *
 * Per pod i, in order, with s its group, e whether it enforces, and minc = min over d in [0, D) of counts[s][d]:
 *   eligible(j) = fits(j) && (!e || (node_domain[j] >= 0 && counts[s][node_domain[j]] + 1 - minc <= max_skew[s]))
 * fits is the scheduler's predicate, with the label check under opts.use_labels; this is kube-scheduler's
 * PodTopologySpread filter with selfMatch = 1.  Everything else is ksched_schedule in exact mode with eligible in the
 * place of fits: out_feasible counts eligible nodes, zero eligible nodes is KSCHED_NO_FIT, the key, the tie-break and
 * the commit alloc -= (req_cpu, req_mem, 1) are unchanged.  So the constraint joins the predicate exactly as labels
 * do: under KSCHED_DOMAIN_ALL an ineligible node can still win the argmax, as in the reference; callers who want
 * enforcement use KSCHED_DOMAIN_FEASIBLE, or best-price, which always ranges over feasible nodes.  If the pod is
 * placed on w, s >= 0 and node_domain[w] >= 0: counts[s][node_domain[w]] += 1, whether or not the pod enforces.
 *
 * State: the counts live in the context and carry over from call to call; ksched_read_spread returns them.
 * ksched_load_nodes invalidates the table (ksched_schedule_spread and ksched_read_spread return KSCHED_E_STATE until
 * it is loaded again); ksched_apply_delta and ksched_save_state / ksched_restore_state leave the counts alone --
 * keeping them in step is the caller's business, as with ksched_load_bound (FakeCluster.schedule_spread reloads the
 * table on every call).  ksched_schedule, ksched_schedule_gangs, ksched_rank, ksched_explain, ksched_explain_batch /
 * _pod and ksched_preempt neither read nor move the table; ksched_rank_full, ksched_explain_full and
 * ksched_preempt_constrained read it.  After ksched_schedule_spread, ksched_explain_batch / ksched_explain_pod return
 * KSCHED_E_STATE: they know no spread reason (KSCHED_NUM_REASONS did not change); ksched_schedule_full_why below gives
 * the reasons at a pod's turn.
 *
 * KSCHED_E_INVALID (nothing changed; a table loaded earlier survives): D or S < 1 or above the caps, S * D >
 * KSCHED_SPREAD_MAX_CELLS, a node domain outside [-1, D), a domain id in [0, D) that no node carries (the minimum
 * ranges over all D with no mask: compact the ids), max_skew < 1, a count outside [0, 2^30], spread_group[i] outside
 * [-1, S), p >= 2^30, opts.nranks > 1.
 *
 * Out of scope: ScheduleAnyway scoring; several constraints or topology keys per pod; minDomains;
 * nodeAffinityPolicy / nodeTaintsPolicy (the minimum ranges over all domains, which is k8s's Ignore); a spread reason
 * from this call itself (at a pod's turn: ksched_schedule_full_why below; against the current state:
 * ksched_explain_full); multi-rank; the batched pipeline.
 *
 * Worked example (best-price, feasible domain): nodes n0 (zone A, price 0.1), n1 (A, 0.2), n2 (B, 0.5), all with ample
 * room; one group with max_skew 1 and counts 0; four enforcing pods.  Pod 0 sees A 0, B 0: every node is eligible, the
 * cheapest is n0 (A 1, B 0).  Pod 1: a pod in A would make the skew 2, only n2 is eligible (A 1, B 1).  Pod 2: as pod
 * 0, n0 (A 2, B 1).  Pod 3: n2.  out_idx = {0, 2, 0, 2}, out_feasible = {3, 1, 3, 1}, final counts A 2, B 2.
 * ksched_schedule on the same input gives {0, 0, 0, 0}. */
#define KSCHED_SPREAD_MAX_DOMAINS 1024
#define KSCHED_SPREAD_MAX_GROUPS  64
#define KSCHED_SPREAD_MAX_CELLS   4096      /* n_groups * n_domains: the per-workgroup LDS table, 16 KiB */
int ksched_load_spread(ksched_ctx *ctx, int32_t n_domains, const int32_t *node_domain /* n_local */,
                       int32_t n_groups, const int32_t *max_skew /* n_groups */,
                       const int32_t *counts /* n_groups * n_domains, NULL = zeros */);
int ksched_read_spread(ksched_ctx *ctx, int32_t *out_counts /* n_groups * n_domains */);
int ksched_schedule_spread(ksched_ctx *ctx, int64_t p, const int64_t *req_cpu, const int64_t *req_mem,
                           const int64_t *req_pods, const uint64_t *selector, const int32_t *spread_group /* p */,
                           const uint8_t *spread_enforce /* p, NULL = all 1 */, int32_t *out_idx, double *out_score,
                           int32_t *out_feasible);

/* ---- extended resources (added within ABI 6: probe with dlsym(lib, "ksched_schedule_ext"); the version number did not move) ----
 * The scalar-resource half of kube-scheduler's NodeResourcesFit: up to KSCHED_EXT_MAX further resource columns beside
 * cpu, memory and pod slots (amd.com/gpu, nvidia.com/gpu, hugepages-2Mi, an RDMA NIC, a pre-scaled ephemeral-storage),
 * resolved by ONE launch of the exact kernel whatever opts.mode says (stats.pipeline == KSCHED_PIPE_EXACT,
 * stats.pair_evals == p * n).  A build extension: the reference knows cpu, memory and pods only.
 *
 * The table (ksched_load_ext, after ksched_load_nodes): node_ext[r * n_local + j] is node j's allocatable amount of
 * resource r -- capacity minus what bound pods already hold.  Any int64 is accepted.
 * Pods: req_ext[r * p + i] >= 0 is pod i's request for resource r (NULL: every request is zero).  A zero request is not
 * checked at all, as in kube-scheduler's fitsRequest: a node whose column is 0 or negative still takes pods that do
 * not ask for it.
 *
 * Per pod i, in order:
 *   eligible(i, j) = fits(i, j) && for every r < n_ext: req_ext[r][i] == 0 || req_ext[r][i] <= ext[r][j]
 * fits is the scheduler's predicate, with the label check under opts.use_labels.  Everything else is ksched_schedule
 * in exact mode with eligible in the place of fits: out_feasible counts eligible nodes, zero eligible nodes is
 * KSCHED_NO_FIT, the key, the tie-break and the commit alloc -= (req_cpu, req_mem, 1) are unchanged.  Scores do not
 * see the extended columns: kube-scheduler's default resource scoring covers cpu and memory only, and so does the
 * reference's.  The constraint joins the predicate exactly as labels and spread do: under KSCHED_DOMAIN_ALL an
 * ineligible node can still win the argmax; callers who want enforcement use KSCHED_DOMAIN_FEASIBLE, or best-price.
 * A pod placed on w does ext[r][w] -= req_ext[r][i] for every r; the subtraction wraps, like the commit's, so under
 * KSCHED_DOMAIN_ALL a column can go negative.
 *
 * State: the table lives in the context and carries over from call to call; ksched_read_ext returns it.
 * ksched_load_nodes invalidates it (ksched_schedule_ext and ksched_read_ext return KSCHED_E_STATE until it is loaded
 * again); ksched_apply_delta and ksched_save_state / ksched_restore_state leave it alone -- keeping it in step is the
 * caller's business (FakeCluster.schedule_ext reloads the table on every call).  ksched_schedule,
 * ksched_schedule_gangs, ksched_schedule_spread, ksched_rank, ksched_explain, ksched_explain_batch / _pod and
 * ksched_preempt neither read nor move it; ksched_rank_full, ksched_explain_full and ksched_preempt_constrained read it.  After ksched_schedule_ext, ksched_explain_batch / ksched_explain_pod return KSCHED_E_STATE: they know no
 * extended-resource reason (KSCHED_NUM_REASONS did not change); ksched_schedule_full_why below gives the reasons at a
 * pod's turn.
 *
 * KSCHED_E_INVALID (nothing changed; a table loaded earlier survives): n_ext outside [1, KSCHED_EXT_MAX], a null
 * node_ext, a negative request, p outside [0, 2^30), opts.nranks > 1.
 *
 * Out of scope: extended columns in ksched_rank, ksched_preempt and ksched_explain* (dry runs that see them:
 * ksched_rank_full, ksched_explain_full and ksched_preempt_constrained below; with gangs and spread: ksched_schedule_constrained below); the batched pipeline and multi-rank; the one-workgroup exact kernel (an ext run always takes the multi-slot one); an apply_delta for the table; init
 * containers and pod overhead; quantity suffixes (amounts are whole numbers, pre-scaled by the caller); scoring on
 * extended resources.
 *
 * Worked example (best-price, feasible domain, one resource "gpu", ample cpu and memory): nodes n0 (price 0.1, gpu 1),
 * n1 (0.2, gpu 0), n2 (0.5, gpu 2); the pods ask for gpu 1, 0, 2, 1.  Pod 0: {n0, n2} are eligible, the cheapest is n0
 * (gpu 0, 0, 2).  Pod 1 asks for nothing, so nothing is checked: all three are eligible, n0 again.  Pod 2: only n2
 * (gpu 0, 0, 0).  Pod 3: no node, KSCHED_NO_FIT.  out_idx = {0, 0, 2, -1}, out_feasible = {2, 3, 1, 0}, final gpu column
 * {0, 0, 0}.  ksched_schedule on the same input gives {0, 0, 0, 0}. */
#define KSCHED_EXT_MAX 4                     /* the exact kernel's per-workgroup LDS table: 4 * 2048 slots * 8 B = 64 KiB */
int ksched_load_ext(ksched_ctx *ctx, int32_t n_ext, const int64_t *node_ext /* n_ext * n_local, node_ext[r * n_local + j] */);
int ksched_read_ext(ksched_ctx *ctx, int64_t *out_ext /* n_ext * n_local */);
int ksched_schedule_ext(ksched_ctx *ctx, int64_t p, const int64_t *req_cpu, const int64_t *req_mem,
                        const int64_t *req_pods, const uint64_t *selector,
                        const int64_t *req_ext /* n_ext * p, req_ext[r * p + i]; NULL = all zero */,
                        int32_t *out_idx, double *out_score, int32_t *out_feasible);

/* ---- gangs, spread and extended resources together (added within ABI 6: probe with dlsym(lib, "ksched_schedule_constrained"); the version number did not move) ----
 * The three calls above in ONE launch of the exact kernel whatever opts.mode says (stats.pipeline == KSCHED_PIPE_EXACT,
 * stats.pair_evals == p * n): a distributed training job is a gang of pods that each ask for amd.com/gpu and spread over
 * zones, and a rejected gang must also give back the GPUs it took and the spread counts it raised -- which three calls
 * one after another cannot do.  The arguments are flat (no struct of pointers: the cgo rule at the top of this file).
 *
 * Each constraint is on or off for the whole call:
 *   gang_off      NULL: n_gangs must be 0, every pod is a gang of one, gang_min and out_gang_placed are ignored.
 *                 Given: ksched_schedule_gangs' rules for n_gangs, gang_off and gang_min, unchanged.
 *   spread_group  NULL: no pod is in a spread group; no spread table is needed, a loaded one is neither read nor moved.
 *                 Given: a table from ksched_load_spread must be loaded (KSCHED_E_STATE otherwise);
 *                 ksched_schedule_spread's rules for spread_group and spread_enforce.
 *   req_ext       NULL: no pod asks for an extended resource; no table is needed, a loaded one is neither read nor moved.
 *                 Given: a table from ksched_load_ext must be loaded (KSCHED_E_STATE otherwise); ksched_schedule_ext's
 *                 rules.
 *
 * Per pod i, in order:
 *   eligible(i, j) = fits(i, j) && spread_ok(i, j) && ext_ok(i, j)
 * fits is the scheduler's predicate, with the label check under opts.use_labels; spread_ok is ksched_schedule_spread's
 * clause (true for a pod that does not enforce); ext_ok is ksched_schedule_ext's (true for a pod that asks for nothing).
 * Everything else is ksched_schedule in exact mode with eligible in the place of fits, exactly as those calls word it:
 * out_feasible counts eligible nodes, zero eligible nodes is KSCHED_NO_FIT, the key and the tie-break are unchanged, and
 * under KSCHED_DOMAIN_ALL an ineligible node can still win the argmax.
 *
 * A pod placed on w commits alloc[w] -= (req_cpu, req_mem, 1); ext[r][w] -= req_ext[r][i], wrapping; and, where its
 * group s >= 0 and node_domain[w] >= 0, counts[s][node_domain[w]] += 1.  Within a gang these commits are tentative, and
 * later members of the same gang see all three.  At the end of gang g, placed >= gang_min[g] decides as in
 * ksched_schedule_gangs:
 *   accepted: all three kinds of commit stand.
 *   rejected: all three are undone -- the node rows, every ext column and every spread count (with each row's minimum)
 *     are bit-identical to their values before the gang's first member.  Out codes and out_gang_placed are
 *     ksched_schedule_gangs': KSCHED_GANG_REJECTED with score 0 for members that had found a node, the member's own code
 *     for those that had not; out_feasible is what each member saw at its turn.
 *
 * State: the spread counts and the ext table carry over from call to call, as with the single calls;
 * ksched_read_spread / ksched_read_ext return them.  Afterwards ksched_explain_batch / ksched_explain_pod return
 * KSCHED_E_STATE (the reasons at a pod's turn: ksched_schedule_full_why below).
 *
 * KSCHED_E_INVALID (nothing changed; loaded tables survive): every invalid case of the three calls, gang_off == NULL
 * with n_gangs != 0, p outside [0, 2^30), opts.nranks > 1.
 *
 * Equivalences: with all three off the call is ksched_schedule in exact mode; with exactly one on it is that
 * constraint's own call, output for output and state for state.
 *
 * Worked example (best-price, feasible domain, ample cpu and memory): nodes n0 (zone A, price 0.1, gpu 2), n1 (A, 0.2,
 * gpu 1), n2 (B, 0.5, gpu 1); one spread group with max_skew 1 and counts 0; the gangs {p0, p1, p2}, {p3, p4}, {p5},
 * every member required; p0-p4 are in the group and enforce, p5 is in no group; the gpu requests are 1, 1, 1, 0, 2, 1.
 * p0: all three nodes are eligible, the cheapest is n0 (A 1, B 0; gpu 1, 1, 1).  p1: zone A would make the skew 2, only
 * n2 (A 1, B 1; gpu 1, 1, 0).  p2: both zones are allowed and gpu >= 1 leaves n0 and n1: n0 (A 2, B 1; gpu 0, 1, 0); gang
 * 0 is accepted with 3 placed.  p3 asks for no gpu, so no column is checked; only zone B is allowed: n2, tentatively A 2,
 * B 2 -- the row's minimum rises to 2.  p4 asks for gpu 2 and no node has it: KSCHED_NO_FIT.  Gang 1 is rejected: p3
 * becomes KSCHED_GANG_REJECTED, the counts go back to A 2, B 1 (the minimum falls back to 1) and n2's row is restored.
 * p5: n1 is the only node with a gpu.  out_idx = {0, 2, 0, -3, -1, 1}, out_feasible = {3, 1, 2, 1, 0, 1},
 * out_gang_placed = {3, 0, 1}, final counts A 2, B 1, final gpu column {0, 0, 0}. */
int ksched_schedule_constrained(ksched_ctx *ctx, int64_t p,
        const int64_t *req_cpu, const int64_t *req_mem, const int64_t *req_pods, const uint64_t *selector,
        int64_t n_gangs, const int64_t *gang_off /* n_gangs + 1, or NULL */, const int32_t *gang_min /* or NULL */,
        const int32_t *spread_group /* p, or NULL */, const uint8_t *spread_enforce /* p, or NULL */,
        const int64_t *req_ext /* n_ext * p, or NULL */,
        int32_t *out_idx, double *out_score, int32_t *out_feasible, int32_t *out_gang_placed);

/* ---- inter-pod affinity and anti-affinity (added within ABI 6: probe with dlsym(lib, "ksched_schedule_affinity"); the version number did not move) ----
 * Required inter-pod affinity and anti-affinity (podAffinity / podAntiAffinity with
 * requiredDuringSchedulingIgnoredDuringExecution), resolved by ONE launch of the exact kernel whatever opts.mode says
 * (stats.pipeline == KSCHED_PIPE_EXACT, stats.pair_evals == p * n).  A build extension: the reference knows no
 * constraints.  The label bitset cannot express it -- the rule depends on where earlier pods of the same call landed --
 * and neither can spread: its rule is a skew against a minimum, its domains stop at 1024 (hostname scope needs D = n),
 * and it has no symmetric half ("an already-bound pod refuses me").
 *
 * Groups: at most KSCHED_AFF_MAX_GROUPS = 64.  A group is the set of pods that one term's label selector matches; group
 * s is bit s of a uint64_t.
 * Scopes: two.  host: every node is its own domain and always carries the key (kubernetes.io/hostname).  zone: ONE
 * topology key; node_domain[j] in [-1, D), -1: node j does not carry the key; D in [0, KSCHED_SPREAD_MAX_DOMAINS].
 * D == 0: there is no zone key -- node_domain may be NULL and every node counts as -1.  Every id in [0, D) must be
 * carried by some node, as ksched_load_spread requires.
 *
 * The table (ksched_load_affinity, after ksched_load_nodes): three mask arrays of n_local uint64_t each, NULL = all zero.
 *   node_member[j]     bit s: some pod bound on j belongs to group s
 *   node_anti_host[j]  bit s: some pod bound on j carries a required anti-affinity term of host scope against group s
 *   node_anti_zone[j]  the same for zone scope; on a node without the key the bits are kept and read back but act on
 *                      nothing
 * The library derives the rest:
 *   zone_member[d] = OR of node_member over the nodes of domain d      any_host = OR of every node_member
 *   zone_anti[d]   = OR of node_anti_zone over the nodes of domain d   any_zone = OR of every zone_member[d]
 *
 * Pods, all flat arrays (the cgo rule at the top of this file); any of them may be NULL, meaning zeros (-1 for aff_group):
 *   member[i]                   the groups the pod belongs to
 *   anti_host[i], anti_zone[i]  the groups its required anti-affinity terms name, per scope
 *   aff_group[i] in [-1, 64), aff_zone[i] (0 = host, otherwise zone)   its ONE required affinity term; -1: none
 * A pod carries at most one affinity term: kube-scheduler counts an existing pod towards affinity only if it matches ALL
 * the pod's terms, which a per-group mask cannot state; with one term the two readings coincide.  It may carry any
 * number of anti-affinity terms: kube treats those one by one.
 *
 * Per pod i, in order, with d = node_domain[j] and a the bit of aff_group[i]:
 *   eligible(i, j) = fits(i, j) && all three of
 *   1. own anti-affinity:    (node_member[j] & anti_host[i]) == 0 && (d < 0 || (zone_member[d] & anti_zone[i]) == 0)
 *                            -- a node without the key cannot violate a zone term
 *   2. bound pods' anti-affinity, the symmetric half:
 *                            (node_anti_host[j] & member[i]) == 0 && (d < 0 || (zone_anti[d] & member[i]) == 0)
 *   3. own affinity, when aff_group[i] >= 0:
 *        waived when a is not in any_host (host scope) or not in any_zone (zone scope), and a is in member[i] -- kube's
 *          first pod of a self-affine set; a waived pod passes this clause on every node
 *        host scope otherwise: a is in node_member[j]
 *        zone scope otherwise: d >= 0 and a is in zone_member[d]
 * fits is the scheduler's predicate, with the label check under opts.use_labels.  Everything else is ksched_schedule in
 * exact mode with eligible in the place of fits: out_feasible counts eligible nodes, zero eligible nodes is
 * KSCHED_NO_FIT, the key, the tie-break and the commit alloc -= (req_cpu, req_mem, 1) are unchanged.  The constraint
 * joins the predicate exactly as labels, spread and ext do: under KSCHED_DOMAIN_ALL an ineligible node can still win the
 * argmax; callers who want enforcement use KSCHED_DOMAIN_FEASIBLE, or best-price.
 *
 * Commit: a pod placed on w, with dw = node_domain[w], does the following whether or not w was eligible:
 *   node_member[w] |= member[i]; node_anti_host[w] |= anti_host[i]; node_anti_zone[w] |= anti_zone[i];
 *   any_host |= member[i];
 *   where dw >= 0: zone_member[dw] |= member[i]; zone_anti[dw] |= anti_zone[i]; any_zone |= member[i].
 * Bound pods never leave during a call, so the words only gain bits: no counts, no minima, no recount.
 *
 * State: the table lives in the context and carries over from call to call; ksched_read_affinity returns the three node
 * arrays (any pointer may be NULL).  ksched_load_nodes invalidates the table (ksched_schedule_affinity and
 * ksched_read_affinity return KSCHED_E_STATE until it is loaded again); ksched_apply_delta and ksched_save_state /
 * ksched_restore_state leave it alone, as with spread -- the caller reloads after deletions
 * (FakeCluster.schedule_affinity reloads the table on every call).  ksched_schedule_full reads and moves the table,
 * ksched_rank_full and ksched_explain_full read it; no other call does either.  After
 * ksched_schedule_affinity, ksched_explain_batch / ksched_explain_pod return KSCHED_E_STATE: they know no affinity reason
 * (KSCHED_NUM_REASONS did not change); ksched_schedule_full_why below gives the reasons at a pod's turn.
 *
 * KSCHED_E_INVALID (nothing changed; a table loaded earlier survives): D outside [0, KSCHED_SPREAD_MAX_DOMAINS], a node
 * domain outside [-1, D), a domain id in [0, D) that no node carries, node_domain == NULL with D > 0 and n > 0,
 * aff_group[i] outside [-1, 64), p outside [0, 2^30), opts.nranks > 1.
 *
 * Out of scope: affinity inside ksched_schedule_constrained (with gangs, spread and ext and the gang rollback:
 * ksched_schedule_full below); preferred (scored) terms; more than one affinity term per pod; more than one
 * zone key; namespaceSelector, matchLabelKeys; pod removal without a reload; affinity reasons from this call itself (at
 * a pod's turn: ksched_schedule_full_why below) and ksched_rank under affinity (against the current state:
 * ksched_explain_full and ksched_rank_full below); ksched_preempt
 * under affinity (under ext and spread: ksched_preempt_constrained below); the batched pipelines and multi-rank; the one-workgroup exact kernel.
 *
 * Worked example (best-price, feasible domain, ample room): nodes n0 (zone A, price 0.1), n1 (B, 0.2), n2 (A, 0.3), n3
 * (no key, 0.4); groups web = bit 0, cache = bit 1, db = bit 2; the table starts empty.  Pods: p0, p1: member web,
 * anti_host web.  p2, p3, p4: member cache, anti_zone cache, affinity web at zone scope.  p5: as p0.  p6: member web, no
 * terms.  p7: member db, affinity db at host scope.  p8: member db, affinity db at zone scope.
 *   pod  eligible  goes to  why
 *   p0   4         n0       nothing bound yet
 *   p1   3         n1       n0 is barred
 *   p2   3         n0       web is in A and B, and n3 has no key
 *   p3   1         n1       zone A now holds a cache
 *   p4   0         NO_FIT   both zones are barred
 *   p5   2         n2       eligible n2 and n3
 *   p6   1         n3       the web pods on n0-n2 refuse it: the symmetric half
 *   p7   4         n0       waived
 *   p8   2         n0       db is now in A: n0, n2
 * out_idx = {0, 1, 0, 1, -1, 2, 3, 0, 0}, out_feasible = {4, 3, 3, 1, 0, 2, 1, 4, 2}, final node_member = {7, 3, 1, 1},
 * node_anti_host = {1, 1, 1, 0}, node_anti_zone = {2, 2, 0, 0}.  ksched_schedule on the same input gives all 0. */
#define KSCHED_AFF_MAX_GROUPS 64             /* one bit of a uint64_t per group */
int ksched_load_affinity(ksched_ctx *ctx, int32_t n_domains, const int32_t *node_domain /* n_local, or NULL with n_domains 0 */,
                         const uint64_t *node_member /* n_local, NULL = zeros */,
                         const uint64_t *node_anti_host /* n_local, NULL = zeros */,
                         const uint64_t *node_anti_zone /* n_local, NULL = zeros */);
int ksched_read_affinity(ksched_ctx *ctx, uint64_t *out_member /* n_local, or NULL */,
                         uint64_t *out_anti_host /* n_local, or NULL */, uint64_t *out_anti_zone /* n_local, or NULL */);
int ksched_schedule_affinity(ksched_ctx *ctx, int64_t p, const int64_t *req_cpu, const int64_t *req_mem,
                             const int64_t *req_pods, const uint64_t *selector,
                             const uint64_t *member /* p, or NULL */, const uint64_t *anti_host /* p, or NULL */,
                             const uint64_t *anti_zone /* p, or NULL */, const int32_t *aff_group /* p, or NULL */,
                             const uint8_t *aff_zone /* p, or NULL = host */,
                             int32_t *out_idx, double *out_score, int32_t *out_feasible);

/* ---- gangs, spread, extended resources and affinity together (added within ABI 6: probe with dlsym(lib, "ksched_schedule_full"); the version number did not move) ----
 * ksched_schedule_constrained and ksched_schedule_affinity in ONE launch of the exact kernel whatever opts.mode says
 * (stats.pipeline == KSCHED_PIPE_EXACT, stats.pair_evals == p * n).  A distributed training job is a gang whose workers
 * each ask for amd.com/gpu, refuse to share a host (podAntiAffinity on hostname) and want to sit in one zone (self-affine
 * podAffinity): the two calls cannot be chained, because a gang that ksched_schedule_affinity would have refused has
 * already committed.  The arguments are flat (the cgo rule at the top of this file).
 *
 * Each constraint is on or off for the whole call:
 *   gang_off, spread_group, req_ext   exactly as in ksched_schedule_constrained.
 *   affinity      on when at least one of member, anti_host, anti_zone, aff_group, aff_zone is non-NULL; the others then
 *                 mean zeros (-1 for aff_group), as in ksched_schedule_affinity.  On: a table from ksched_load_affinity
 *                 must be loaded (KSCHED_E_STATE otherwise).  Off (all five NULL): no table is needed, a loaded one is
 *                 neither read nor moved.
 *
 * Per pod i, in order:
 *   eligible(i, j) = fits(i, j) && spread_ok(i, j) && ext_ok(i, j) && affinity_ok(i, j)
 * fits, spread_ok and ext_ok are ksched_schedule_constrained's; affinity_ok is the three clauses of
 * ksched_schedule_affinity, the waiver included (true for a pod without group or term).  Everything else is
 * ksched_schedule in exact mode with eligible in the place of fits, exactly as those calls word it: out_feasible counts
 * eligible nodes, zero eligible nodes is KSCHED_NO_FIT, the key and the tie-break are unchanged, and under
 * KSCHED_DOMAIN_ALL an ineligible node can still win the argmax.
 *
 * A pod placed on w commits the node row, the ext columns and the spread count as in ksched_schedule_constrained, and the
 * affinity words as in ksched_schedule_affinity: node_member[w], node_anti_host[w], node_anti_zone[w], any_host and,
 * where the affinity table's node_domain[w] >= 0, zone_member, zone_anti and any_zone.  Within a gang all four kinds of
 * commit are tentative, and later members of the same gang see all four.  At the end of gang g, placed >= gang_min[g]
 * decides as in ksched_schedule_gangs:
 *   accepted: all four stand.
 *   rejected: all four are undone.  Beside what ksched_schedule_constrained promises, the three node arrays that
 *     ksched_read_affinity returns are bit-identical to their values before the gang's first member, and so are the
 *     derived zone and any words the context keeps: a waiver that a rejected gang spent is available again.  Out codes and
 *     out_gang_placed are ksched_schedule_gangs'.
 *
 * Separate zone keys: the spread table's node_domain and the affinity table's node_domain are two independent arrays; the
 * keys, and the number of domains, may differ.
 *
 * State: the spread counts, the ext table and the affinity words carry over from call to call, as with the single calls;
 * ksched_read_spread / ksched_read_ext / ksched_read_affinity return them.  Afterwards ksched_explain_batch /
 * ksched_explain_pod return KSCHED_E_STATE; the same run with every NO_FIT pod's reasons at its turn is
 * ksched_schedule_full_why below.
 *
 * KSCHED_E_INVALID (nothing changed; loaded tables survive): every invalid case of the four calls -- gang_off == NULL
 * with n_gangs != 0, p outside [0, 2^30), aff_group[i] outside [-1, 64), opts.nranks > 1 among them.
 *
 * Limits: the single calls' (KSCHED_GANG_MAX, KSCHED_SPREAD_MAX_*, KSCHED_EXT_MAX, KSCHED_AFF_MAX_GROUPS), and the exact
 * kernel's geometry unchanged: up to 2048 nodes per workgroup with every table on.  A rejected gang's undo log of the
 * affinity words lives in device memory the context owns (24 KiB, and 16 KiB per workgroup).
 *
 * Equivalences: with affinity off the call is ksched_schedule_constrained, with only affinity on it is
 * ksched_schedule_affinity, output for output and state for state.
 *
 * Worked example (best-price, feasible domain, ample cpu and memory): nodes n0 (zone A, price 0.1, gpu 1), n1 (A, 0.2,
 * gpu 1), n2 (B, 0.3, gpu 1), n3 (B, 0.4, gpu 0); both tables use the same zones.  Spread: one group, max_skew 1, counts
 * 0; p0-p4 are in it and only count (enforce 0), p5 is in it and enforces.  Affinity: group train = bit 0, an empty table.
 * Gangs {p0, p1, p2}, {p3, p4}, {p5}, every member required.  p0-p4: member train, anti_host train, affinity train at zone
 * scope, gpu 1.  p5: no words, gpu 0.
 *   pod  eligible  outcome  why
 *   p0   3         n0       waived: no train anywhere
 *   p1   1         n1       train is now in zone A only, and n0 refuses it
 *   p2   0         NO_FIT   zone A's hosts are both taken
 * Gang 0 is rejected: p0 and p1 become KSCHED_GANG_REJECTED; the rows, the gpus, the counts (A 2 -> 0) and every affinity
 * word go back.
 *   p3   3         n0       waived AGAIN -- with any_zone left set it would find no node, with the node words left set
 *                           n0 and n1 would refuse it
 *   p4   1         n1       as p1
 *   p5   2         n2       zone A would make the skew 3
 * out_idx = {-3, -3, -1, 0, 1, 2}, out_feasible = {3, 1, 0, 3, 1, 2}, out_gang_placed = {0, 2, 1}, final counts A 2, B 1,
 * final gpu column {0, 0, 1, 0}, node_member = node_anti_host = {1, 1, 0, 0}, node_anti_zone all 0. */
int ksched_schedule_full(ksched_ctx *ctx, int64_t p,
        const int64_t *req_cpu, const int64_t *req_mem, const int64_t *req_pods, const uint64_t *selector,
        int64_t n_gangs, const int64_t *gang_off /* n_gangs + 1, or NULL */, const int32_t *gang_min /* or NULL */,
        const int32_t *spread_group /* p, or NULL */, const uint8_t *spread_enforce /* p, or NULL */,
        const int64_t *req_ext /* n_ext * p, or NULL */,
        const uint64_t *member /* p, or NULL */, const uint64_t *anti_host /* p, or NULL */,
        const uint64_t *anti_zone /* p, or NULL */, const int32_t *aff_group /* p, or NULL */,
        const uint8_t *aff_zone /* p, or NULL = host */,
        int32_t *out_idx, double *out_score, int32_t *out_feasible, int32_t *out_gang_placed);

/* ---- dry runs under constraints (added within ABI 6: probe with dlsym(lib, "ksched_rank_full"); the version number did not move) ----
 * ksched_rank and ksched_explain with ksched_schedule_full's eligible in the place of fits: the scheduler-extender filter
 * and prioritize verbs, and the FailedScheduling event with its per-node reasons (anchor/predicate.go:127-171), for a pod
 * that carries a spread constraint, extended-resource requests or affinity terms.  A caller whose training job came back
 * KSCHED_NO_FIT from ksched_schedule_full asks here whether it was "Insufficient amd.com/gpu", the spread skew, its own
 * anti-affinity or somebody else's.
 *
 * Both are dry runs in ksched_rank's sense.  They read the node rows and the context's spread, extended-resource and
 * affinity tables AS THEY STAND, every pod on its own; NOTHING is committed.  Afterwards the node rows, what
 * ksched_read_spread / ksched_read_ext / ksched_read_affinity return, the staged pods, the last call's results and the
 * validity and content of ksched_explain_batch are byte-identical to before.  So they describe the CURRENT state, not the
 * state a pod of an earlier call saw at its turn -- as kube-scheduler re-posts FailedScheduling at each retry against the
 * then-current state.
 *
 * Reason codes: KSCHED_REASON_FIT .. KSCHED_REASON_LABELS keep their values; the constraints add the codes below.  A
 * node's reason is the FIRST failing check in exactly this order: cpu, memory, pods, labels (under opts.use_labels), the
 * extended columns 0 .. n_ext - 1 (a zero request is skipped), the spread key, the spread skew, the pod's affinity term,
 * its own anti-affinity terms, the bound pods' anti-affinity terms.  Reason 0 is eligible(i, j) of ksched_schedule_full
 * -- the same predicate, with the same tables, not a restatement: spread_ok is ksched_schedule_spread's clause with minc
 * taken over the current counts, ext_ok ksched_schedule_ext's, and the three affinity clauses are
 * ksched_schedule_affinity's.  The waiver of clause 3 is decided per pod from the context's current any_host / any_zone,
 * as that call words it; a waived pod never gets KSCHED_REASON_AFFINITY.
 *
 * ksched_rank_full is ksched_rank with eligible in the place of fits; everything else is that call's contract word for
 * word: m pod shapes, each on its own; entry r of pod i its r-th best eligible node in the scheduler's order; count == 0
 * with feasible == 0 is KSCHED_NO_FIT and with feasible > 0 KSCHED_NO_POSITIVE_SCORE; under KSCHED_DOMAIN_ALL an
 * ineligible node can be ranked, and out_reason then carries its full code; 1 <= k <= KSCHED_RANK_MAX; large m is served
 * in chunks with a bounded device workspace (below 20 MiB); any output pointer may be NULL; the call waits for the
 * context's stream first.  Entry 0 of pod i is what ksched_schedule_full would choose if that pod were the next call's
 * only pod.  What differs:
 *   out_feasible       m     nodes with reason 0
 *   out_reason_counts  m*14  out_reason_counts[i * KSCHED_NUM_REASONS_FULL + r] = nodes whose reason is r: a row sums to
 *                            n_local, and its column 0 is out_feasible[i]
 * Each constraint is on or off for the whole call, by ksched_schedule_full's NULL rule: spread_group, req_ext, or any of
 * the five affinity pointers switches its constraint on (the other affinity arrays then mean zeros, -1 for aff_group).
 * On: its table must be loaded (KSCHED_E_STATE otherwise).  Off: no table is needed, a loaded one is not read.
 *
 * ksched_explain_full is ksched_explain for one pod with these codes: out_counts[r] counts the nodes per code
 * (out_counts[KSCHED_REASON_FIT] is the pod's feasible count), out_reason (n_local bytes, may be NULL) receives each
 * node's code.  A constraint is on where the pod uses it: spread when spread_group >= 0 (spread_enforce == 0: the pod
 * only counts, and no spread code arises), ext when req_ext != NULL, affinity when a word is non-zero or aff_group >= 0.
 * Its counts equal the pod's row of ksched_rank_full's out_reason_counts, and its codes at ranked nodes that call's
 * out_reason.
 *
 * KSCHED_E_INVALID (nothing changed): the single calls' argument rules -- spread_group outside [-1, S), a negative
 * extended-resource request, aff_group outside [-1, 64) --, k out of range, m outside [0, 2^30), a NULL request array, a
 * NULL selector under opts.use_labels, a NULL out_counts, opts.nranks > 1 (the tables are single-GPU; there is no shard
 * merge).  KSCHED_E_STATE before ksched_load_nodes.  n_local == 0 answers as ksched_rank does: empty lists, zero counts.
 *
 * Out of scope: dry runs of a gang (members see each other's tentative commits); ksched_preempt under affinity
 * (under ext and spread: ksched_preempt_constrained below); multi-rank; ScheduleAnyway and preferred terms.  The reasons a pod of a finished constrained run saw at its turn are
 * not a dry run's to give -- a rolled-back gang leaves no placements to rebuild from, and ksched_explain_batch /
 * ksched_explain_pod still return KSCHED_E_STATE after a constrained call: ksched_schedule_full_why below collects them
 * inside the run.
 *
 * Worked example, from the end state of ksched_schedule_full's own worked example (best-price, feasible domain): n0, n1
 * in zone A, n2, n3 in B; counts A 2, B 1 with max_skew 1 (minc 1: a domain may hold at most 1); gpu column {0, 0, 1, 0};
 * node_member = node_anti_host = {1, 1, 0, 0}, so zone_member = {A 1, B 0}; train = bit 0.
 *   pod                                                              reasons n0..n3   list
 *   X  member, anti_host and zone affinity train, gpu 1, group 0     5, 5, 11, 5      empty, feasible 0
 *   Y  as X, but gpu 0 and no spread group                           12, 12, 11, 11   empty
 *   Z  member train only                                             13, 13, 0, 0     n2 (0.3), n3 (0.4)
 *   W  no affinity words, gpu 0, group 0 (enforcing)                 10, 10, 0, 0     n2, n3
 * X: three nodes have no gpu, and the check comes before the affinity term that n2 fails (no train in zone B).  Y: the
 * train pods on n0 and n1 are what its own anti-affinity names.  Z carries no term, but the bound pods' terms refuse it. */
#define KSCHED_REASON_EXT0                    5   /* + r, r < KSCHED_EXT_MAX: "Insufficient <resource r>"; the lowest failing column */
#define KSCHED_REASON_SPREAD_NO_KEY           9   /* an enforcing pod, node_domain[j] < 0 */
#define KSCHED_REASON_SPREAD_SKEW            10   /* counts[s][d] + 1 - minc > max_skew[s] */
#define KSCHED_REASON_AFFINITY               11   /* ksched_schedule_affinity's clause 3, the pod's own affinity term (not waived) */
#define KSCHED_REASON_ANTI_AFFINITY          12   /* clause 1, the pod's own anti-affinity terms */
#define KSCHED_REASON_EXISTING_ANTI_AFFINITY 13   /* clause 2, bound pods' terms: the symmetric half */
#define KSCHED_NUM_REASONS_FULL              14
int ksched_rank_full(ksched_ctx *ctx, int64_t m,
        const int64_t *req_cpu, const int64_t *req_mem, const int64_t *req_pods, const uint64_t *selector,
        const int32_t *spread_group /* m, or NULL */, const uint8_t *spread_enforce /* m, or NULL = all 1 */,
        const int64_t *req_ext /* n_ext * m, req_ext[r * m + i], or NULL */,
        const uint64_t *member /* m, or NULL */, const uint64_t *anti_host /* m, or NULL */,
        const uint64_t *anti_zone /* m, or NULL */, const int32_t *aff_group /* m, or NULL */,
        const uint8_t *aff_zone /* m, or NULL = host */,
        int32_t k, int32_t *out_idx, double *out_score, uint8_t *out_reason, int32_t *out_count,
        int32_t *out_feasible, int64_t *out_reason_counts /* m * KSCHED_NUM_REASONS_FULL, or NULL */);
int ksched_explain_full(ksched_ctx *ctx, int64_t req_cpu, int64_t req_mem, int64_t req_pods, uint64_t selector,
        int32_t spread_group /* -1: none */, int32_t spread_enforce, const int64_t *req_ext /* n_ext, or NULL */,
        uint64_t member, uint64_t anti_host, uint64_t anti_zone, int32_t aff_group /* -1: none */, int32_t aff_zone,
        int64_t out_counts[KSCHED_NUM_REASONS_FULL], uint8_t *out_reason /* n_local, or NULL */);

/* ---- FailedScheduling reasons at a pod's turn (added within ABI 6: probe with dlsym(lib, "ksched_schedule_full_why"); the version number did not move) ----
 * The reference posts a FailedScheduling event at the turn of every pod that fits nowhere, with one line per node
 * (anchor/predicate.go:127-171).  ksched_explain_batch / ksched_explain_pod keep that for ksched_schedule by rebuilding a
 * pod's state from the call's placements; a constrained call cannot be rebuilt that way -- the state a member of a
 * rejected gang saw held the tentative commits of its own gang, and the rollback erased them -- and ksched_explain_full
 * answers against the state of NOW.  This call collects the reasons inside the run, at the pod's turn: the training job
 * that came back KSCHED_GANG_REJECTED learns which member failed and why ("Insufficient amd.com/gpu on 61 nodes,
 * anti-affinity on 3").
 *
 * The call IS ksched_schedule_full on the same arguments: out_idx, out_score, out_feasible and out_gang_placed are what
 * that call returns on the same input, bit for bit, and so are the node rows, the three tables, the stats
 * (stats.pipeline == KSCHED_PIPE_EXACT, stats.pair_evals == p * n), the NULL rules that switch a constraint off and the
 * state rules afterwards (ksched_explain_batch / ksched_explain_pod return KSCHED_E_STATE).  With every constraint off
 * it is therefore the at-its-turn explain of ksched_schedule in exact mode, with the codes 0-4 only.
 *
 * What it adds.  Every pod whose outcome at its turn is KSCHED_NO_FIT (zero eligible nodes) is one NO_FIT pod, in pod
 * order; *out_nofit (may be NULL) is their total number, and the first min(total, why_rows) of them are recorded, row r
 * for the r-th:
 *   out_why_pod[r]                               the pod's index
 *   out_why_counts[r * KSCHED_NUM_REASONS_FULL + c]   the number of local nodes whose reason is c
 *   out_why_reason[r * n_local + j]              node j's code, for r < node_rows (node_rows <= why_rows; NULL with 0)
 * Rows past the recorded ones: out_why_pod -1, the counts 0, the bytes 0.  why_rows == 0 is allowed: only *out_nofit is
 * produced.
 *
 * The codes are ksched_rank_full's fourteen in its order -- the first failing check -- evaluated against the rows and
 * tables AS THE POD SAW THEM AT ITS TURN: all commits of the earlier pods of the call; the tentative commits of the
 * earlier members of its own gang, whether that gang is later accepted or rejected; the spread minimum of that moment;
 * and the waiver of the affinity term decided from the any_host / any_zone of that moment (a waived pod never gets
 * KSCHED_REASON_AFFINITY).  Consequences: a recorded row has column 0 equal to 0 and sums to n_local; a NO_FIT member
 * of a rejected gang keeps its row -- the reason the gang failed; members that found a node have no row, and neither
 * have KSCHED_NO_POSITIVE_SCORE pods (they had eligible nodes).
 *
 * KSCHED_E_INVALID (nothing changed; loaded tables survive): every case of ksched_schedule_full, in its order; then
 * why_rows or node_rows negative, node_rows > why_rows, why_rows >= 2^30; a NULL out_why_pod or out_why_counts with
 * why_rows > 0; a NULL out_why_reason with node_rows > 0; node_rows * n_local above KSCHED_WHY_MAX_NODE_BYTES.  The rows
 * live in a device buffer the context owns, why_rows * (4 + 8 * KSCHED_NUM_REASONS_FULL) bytes and the node bytes;
 * KSCHED_E_NOMEM when it cannot be had, with everything unchanged.
 *
 * Worked example: ksched_schedule_full's own.  p2 is the only NO_FIT pod (*out_nofit == 1, out_why_pod[0] == 2).  At its
 * turn n0 and n1 hold p0 and p1 -- tentatively: their gang is rejected afterwards -- and the gpu column is {0, 0, 1, 0}.
 * Its codes n0..n3 are 5, 5, 11, 5: three nodes without a gpu (the check comes before n0's and n1's anti-affinity), and
 * zone B without a train pod; the counts row has 3 in column 5 and 1 in column 11.  Asked of ksched_explain_full after
 * the call, the same pod is judged against a state where gang 0 has gone and gang 1 sits on n0 and n1 instead: this
 * input gives the same four codes there, but in general they differ (in the tests' generated inputs, for between one half
 * and all of a call's NO_FIT pods).
 *
 * Out of scope: the batched pipelines and multi-rank (opts.nranks > 1 is KSCHED_E_INVALID, as for ksched_schedule_full);
 * per-node bytes for pods that were placed or had no positive score; a reason for KSCHED_GANG_REJECTED members beyond
 * their gang's NO_FIT rows; the Go shim. */
#define KSCHED_WHY_MAX_NODE_BYTES (1 << 28)  /* node_rows * n_local: the per-node bytes of one call */
int ksched_schedule_full_why(ksched_ctx *ctx, int64_t p,
        const int64_t *req_cpu, const int64_t *req_mem, const int64_t *req_pods, const uint64_t *selector,
        int64_t n_gangs, const int64_t *gang_off /* n_gangs + 1, or NULL */, const int32_t *gang_min /* or NULL */,
        const int32_t *spread_group /* p, or NULL */, const uint8_t *spread_enforce /* p, or NULL */,
        const int64_t *req_ext /* n_ext * p, or NULL */,
        const uint64_t *member /* p, or NULL */, const uint64_t *anti_host /* p, or NULL */,
        const uint64_t *anti_zone /* p, or NULL */, const int32_t *aff_group /* p, or NULL */,
        const uint8_t *aff_zone /* p, or NULL = host */,
        int32_t *out_idx, double *out_score, int32_t *out_feasible, int32_t *out_gang_placed,
        int64_t why_rows, int32_t *out_why_pod /* why_rows */,
        int64_t *out_why_counts /* why_rows * KSCHED_NUM_REASONS_FULL */,
        int64_t node_rows, uint8_t *out_why_reason /* node_rows * n_local, or NULL with node_rows 0 */,
        int64_t *out_nofit /* or NULL */);

/* ---- preemption under the extended columns and the spread table (added within ABI 6: probe with dlsym(lib, "ksched_preempt_constrained"); the version number did not move) ----
 * ksched_preempt knows cpu, memory and pod slots.  A pod that came back KSCHED_NO_FIT from ksched_schedule_full with
 * "Insufficient amd.com/gpu" on every node gets from it a node where cpu can be freed but no gpu can, or a victim set
 * that reprieves the one pod holding the gpu.  kube-scheduler's default preemption removes the lower-priority pods from
 * every filter plugin's view of the node (RemovePod), re-runs the filters, and reprieves under the same filters.  Two of
 * the constraints here are counted, so a removal is an exact subtraction: the extended columns, as amounts, and the
 * spread table, as counts per (group, domain).  These two calls are preemption under those two --
 * ksched_schedule_constrained's node-level constraints.
 *
 * ksched_load_bound_constrained loads the one bound-pod table ksched_load_bound loads, under its rules (after
 * ksched_load_nodes; it replaces the table held; ksched_load_nodes invalidates it; a refused load leaves the earlier
 * table in place; KSCHED_BOUND_MAX_PER_NODE), with two more columns per pod:
 *   bound_ext[r * nb + t] >= 0   what table pod t holds of extended resource r: what its commit subtracted from
 *                                ext[r][node].  NULL if and only if n_ext == 0
 *   bound_spread[t]              bit s set: pod t is counted in counts[s][.] of the spread table -- it matches group s's
 *                                selector.  A mask, not an index: a bound pod can match several groups' selectors.  NULL:
 *                                zeros
 * KSCHED_E_INVALID: ksched_load_bound's cases; n_ext outside [0, KSCHED_EXT_MAX]; a NULL bound_ext with n_ext > 0 or a
 * non-NULL one with n_ext == 0; a negative amount.  A table loaded by ksched_load_bound is the table with n_ext == 0 and
 * every mask zero.  ksched_preempt ignores the extra columns: its outputs after this call are byte-equal to those after
 * ksched_load_bound with the first four arrays.
 *
 * ksched_preempt_constrained is ksched_preempt word for word -- a dry run, each pod on its own, nothing committed; the
 * outputs, the key, the choice, vcap, the chunks, the wait for the stream, selector under opts.use_labels -- except for
 * the eligibility of a node.  Each constraint is on or off for the whole call by ksched_schedule_full's NULL rule
 * (spread_group, req_ext).  Per pod i and node j, with d = the spread table's node_domain[j]; s = spread_group[i] where it
 * is >= 0 and the pod enforces, none otherwise; C = counts[s][d] as loaded; mo = the minimum of counts[s][d'] over
 * d' != d (absent with one domain: the minimum below is then c alone):
 *   1. potential victims: the table's pods on j with prio < prio[i]; ksched_preempt's importance order.
 *   2. with all of them gone: free = alloc[j] + sum of (cpu, mem, 1); fext[r] = ext[r][j] + sum of bound_ext[r][v]
 *      (wrapping int64); rem = the potential victims with bit s in their mask.
 *        elig(free, fext, rem) = fits(req[i], free)
 *                                && for every r: req_ext[r][i] == 0 || req_ext[r][i] <= fext[r]
 *                                && (s none || (d >= 0 && c + 1 - min(mo, c) <= max_skew[s])),  c = C - rem in int64
 *      !elig: j is no candidate.
 *   3. reprieve, most important first: elig(free - v, fext - v's amounts, rem - [v has bit s]) holds: those become the
 *      state and v is reprieved; otherwise v is a victim.
 *   4. the node's key, the choice (smallest key, then lowest global index) and every output column: ksched_preempt's.
 * The preemptor's own + 1 is in the formula only: no count moves.  A pod that only counts (spread_enforce == 0) or has
 * group -1 reads no count.  A zero extended request checks nothing, so a zero or negative column does not bar the node.
 * elig is monotone -- more free resource and fewer counted pods never make it false -- so with its victims gone the pod
 * is eligible on the chosen node, and with the last victim left in place it is not.  Keeping the counts and the masks
 * consistent is the caller's business, as with every table here (FakeCluster.preempt_pod_constrained derives both from
 * the same pods).
 *
 * Errors, in this order.  KSCHED_E_INVALID (nothing changed): ksched_preempt's argument rules; m outside [0, 2^30);
 * opts.nranks > 1 (the tables are single-GPU: there is no shard merge for this call); ksched_schedule_spread's and
 * ksched_schedule_ext's rules for the pod arrays (a group outside [-1, S), a negative request; against a table that is
 * loaded -- without one there is no S and no array length, and the call ends in the next code).  KSCHED_E_STATE: before
 * ksched_load_nodes; no bound-pod table; a constraint on without its table; req_ext given and the bound table's n_ext
 * not the ext table's; spread on and a mask bit at or above the spread table's S.
 *
 * The call leaves byte-identical: the node rows, what ksched_read_spread and ksched_read_ext return, the staged pods, the
 * last call's results, and the validity and content of ksched_explain_batch.  With both constraints off its outputs are
 * byte-equal to ksched_preempt's on the same table (from kernels of its own).  With every prio[i] at or below the
 * table's lowest priority nobody may go: out_candidates[i] is then ksched_explain_full's out_counts[0] for that pod
 * (affinity off, the same spread and ext arguments), and out_node[i] the lowest node whose code there is 0, or
 * KSCHED_NO_FIT.
 *
 * Out of scope: affinity under preemption (the affinity table keeps ORs of group bits per node and zone, and a removal
 * cannot be taken out of an OR: it needs per-(node, group) counts first); gangs of preemptors; PDBs and start times;
 * multi-rank; the batched pipelines; reasons for the nodes that are no candidates.
 *
 * Worked example.  ksched_preempt's hand cluster (tests/test_preempt_host.py; 1 MiB and 10 slots free everywhere) with
 * one gpu column and one spread group of max_skew 1, loaded counts A 3, B 2 (one counted pod in A is not in the table):
 *   node  alloc cpu  zone  free gpu      table pod  node  cpu  prio  gpu  in group
 *   n0    400        A     0             0          n2    500  100   1    yes
 *   n1    0          B     0             1          n0    600  200   1    no
 *   n2    400        A     1             2          n1    500  200   0    yes
 *                                        3          n0    500  100   1    yes
 *                                        4          n1    500  50    1    yes
 *                                        5          n2    600  200   0    no
 * Pods: A cpu 1000, prio 1000, gpu 2, no group; B as A with prio 150 and gpu 0; C cpu 400, prio 1000, gpu 0, group 0,
 * enforcing; D as C, counting only.
 *   A on n0: free cpu 1500, gpu 2.  Pod 1: 900 < 1000, a victim.  Pod 3: cpu fits, but gpu 2 - 1 < 2, a victim.  Key
 *     (200, 300 + 2^32, 2), victims [1, 3].  n1: gpu 1 < 2, no candidate.  n2: n0's key, victims [5, 0], loses the tie
 *     on the index.  Answer: n0, 2 victims, 2 candidates (ksched_preempt: n0, victims [1], 3 candidates -- a gpu short).
 *   B: no candidate.
 *   C on n0: rem 1, c = 2, skew 1: a candidate.  Pod 1: reprieved.  Pod 3: c = 3, 3 + 1 - 2 = 2 > 1, a victim by the
 *     spread rule alone.  Key (100, ...).  n1: rem 2, c = 0.  Pod 2: reprieved (cpu 500 >= 400, c = 1).  Pod 4: cpu 0 <
 *     400, a victim.  Key (50, 50 + 2^31, 1).  n2: as n0, victim [0].  Answer: n1, victims [4], 3 candidates
 *     (ksched_preempt: n0, no victim).
 *   D: n0, no victim, 3 candidates.
 * At vcap 2: out_node {0, -1, 1, 0}, out_nvictims {2, 0, 1, 0}, out_max_prio {200, INT32_MIN, 50, INT32_MIN},
 * out_sum_prio {4294967596, 0, 2147483698, 0}, out_candidates {2, 0, 3, 3}, out_victims {[1, 3], [-1, -1], [4, -1],
 * [-1, -1]}. */
int ksched_load_bound_constrained(ksched_ctx *ctx, int64_t nb, const int32_t *node_idx, const int64_t *cpu,
        const int64_t *mem, const int32_t *prio,
        int32_t n_ext, const int64_t *bound_ext /* n_ext * nb, bound_ext[r * nb + t]; NULL iff n_ext == 0 */,
        const uint64_t *bound_spread /* nb, or NULL = zeros */);
int ksched_preempt_constrained(ksched_ctx *ctx, int64_t m,
        const int64_t *req_cpu, const int64_t *req_mem, const int64_t *req_pods, const uint64_t *selector,
        const int32_t *prio,
        const int32_t *spread_group /* m, or NULL */, const uint8_t *spread_enforce /* m, or NULL = all 1 */,
        const int64_t *req_ext /* n_ext * m, req_ext[r * m + i], or NULL */,
        int32_t vcap, int32_t *out_node, int32_t *out_nvictims, int32_t *out_max_prio, int64_t *out_sum_prio,
        int32_t *out_candidates, int32_t *out_victims);

/* Same, in two halves, with the pods staged in HBM: upload once, run many times (bench). */
int ksched_upload_pods(ksched_ctx *ctx, int64_t p, const int64_t *req_cpu, const int64_t *req_mem,
                       const int64_t *req_pods, const uint64_t *selector);
int ksched_run(ksched_ctx *ctx);                 /* schedules the staged pods; results stay on device */
/* Bound of every device-side wait of the persistent pipeline, in ms (default 10000, or the
 * KSCHED_PERSIST_TIMEOUT_MS environment variable at create).  A wait that exceeds it ends the call with
 * KSCHED_E_DEVICE naming the wait and where every workgroup stood (ABI 4). */
int ksched_set_timeout(ksched_ctx *ctx, int32_t persist_ms);
int ksched_sync(ksched_ctx *ctx);                /* waits for the run; fills stats */
int ksched_download_results(ksched_ctx *ctx, int64_t p, int32_t *out_idx, double *out_score, int32_t *out_feasible);
int ksched_get_stats(const ksched_ctx *ctx, ksched_stats *out);
/* Diagnostics (added within ABI 6: probe with dlsym(lib, "ksched_get_commit_stamps")): the first n <= 48 words of the
 * persistent commit's KSCHED_COMMIT_STAMPS sums of the last synced run -- zeros unless the context was created with
 * that variable set (n <= 32 up to the library that added the fold masks: a larger n is KSCHED_E_INVALID there, and
 * words 0-31 keep their meaning).  [12] rounds, [13] failed guesses, [14] batches, [15] batches whose early read of
 * the merge count sufficed, [29] batches whose inherited keys were loaded before the merges' wait, [30] batches that
 * tried (those with an older export to inherit, voided ones included); the others of 0-31 are cycle sums and the
 * touched-node screen's column counts (ksched_diag.hip's print_persist_trace prints them, the fold masks' line too,
 * with the KSCHED_PERSIST_TRACE summary; print_commit_stamps is the stream pipeline's).  The two commit workgroups add
 * to the same words: the resource-priority (screened) kernels add the counts [5], [8], [12]-[14], [31] and [32]-[37]
 * atomically, so they are exact; the best-price kernels keep plain adds for [5], [8], [12]-[14] and [31], which can
 * lose a few per call (the cycle sums are plain adds in every kernel).  The screened commit's fold masks
 * (KSCHED_NO_FOLD_MASK=1 turns them off): [32] rounds whose check read no wave's partial bests, [33] partial rows read
 * over all checks (masks off: waves x rounds), [34] batches whose wave-0 state read none, [35] columns the confirm
 * folds visited, [36] columns they skipped, [37] batches with a check that read none after an earlier one that read
 * some; [38]-[47] are reserved (zero). */
int ksched_get_commit_stamps(const ksched_ctx *ctx, int32_t n, int64_t *out);
/* Diagnostics (added within ABI 6: probe with dlsym): the seeded score scan's counters of the last synced persistent
 * run, summed over the score workgroups, into out[5]: [0] (workgroup, batch) scans whose bound was seeded from the
 * previous batch's needed rows, [1] seed rows, [2] scans whose bound was 0 (everything passes) for some active pod,
 * [3] scans seeded from all rows because the batch before ran unscreened (it left no masks), [4] ... because its
 * needed rows passed the cap.  (A call's first scans and KSCHED_NO_SEED runs seed from all rows too.) */
int ksched_get_seed_stats(const ksched_ctx *ctx, int64_t *out);
/* Turns the sampled per-kernel HIP-event timing (opts.timing / opts.timing_every) on or off for the
 * following calls (every = 0: keep the current sampling period). */
int ksched_set_timing(ksched_ctx *ctx, int32_t timing, int32_t every);

/* Diagnostics: out_native[i] = a[i] / b[i] (hipcc's f64 division) and out_fast[i] = the engine's
 * hoisted-reciprocal division of the same operands, both computed on the device (bit-exactness
 * check of the division used by every score kernel). */
int ksched_selftest_fastdiv(ksched_ctx *ctx, int64_t n, const double *a, const double *b, double *out_native,
                            double *out_fast);
/* Diagnostics (added within ABI 6: probe with dlsym): the device's own score, screen, record and wave primitives,
 * run in isolation on arrays of operands.  They prove the primitives' source semantics under the library's
 * compile flags, not the instruction stream of the kernels that inline them.  Arrays are structure-of-arrays:
 * "[k][n]" is k rows of n elements.  req / alloc: [3][n] (cpu, memory, pods).
 *   score:     out_score [3][n] resource_score, resource_score_fast<false>, <true>; out_upper [2][n]
 *              resource_score_upper<false>, <true>; out_recip [3][n] recip((double)alloc); out_flags [n]: bit 0 / 1
 *              near1 of the two upper bounds, bit 2 / 3 eligible (resource priority) in the all-node / feasible
 *              domain, bit 4 the fit predicate.
 *   price_key: out_key[i] = the best-price key of price[i].
 *   screen:    out_f32 [13][n] screen_req x3, screen_recip x3, screen_y x3, screen_pair from screen_recip, from
 *              screen_y, screen_fast's v and mx; out_u32 [8][n] lo_ok of the two screen_pair, amb, rf, pass 1's
 *              record: all-node domain by screen_rec / screen_rec_nf, by the packed conversion, feasible domain
 *              likewise (no labels).
 *   rec_w:     out [4][n] screen_rec_w(w), screen_rec_w(w2), low and high half of the packed conversion of (w, w2).
 *   threshold: out [4][n] screen_rec_threshold(L), screen_rec_threshold_nf(L), screen_rec_needed(rec, those two),
 *              screen_rec_needed(rec, -1, -1).
 *   wave:      ncases cases of 64 lanes.  sort_code / sort_idx [6][64 ncases]: the pairs in aligned sorted runs of
 *              1, 2, 4, 8, 16, 32; key / idx / aux [64 ncases]; cut / nv [ncases].  out_u64 [12][64 ncases]: the six
 *              sorted codes, wave_max_u64 and wave_sum_i64 of arrangement 0's codes, the key bits of wave_argbest and
 *              wave_argbest_fast, key_code(key), wave_or_u64 of arrangement 0's codes.  out_i32 [13][64 ncases]: the
 *              six sorted idx, wave_rank of the lane's own pair and wave_min_i32(idx) (arrangement 0), the two
 *              arg-bests' idx, their aux, list_thr_bits(cut, lanes < nv, key_code(key)).
 *   list:      key / idx [steps][n]: one sequence per element (idx 0x7fffffff: skipped) through
 *              list_insert_ordered<2, 4, 8, 16>; out_key / out_idx [30][n]: the four lists one after the other.
 *   slots:     x [2][steps][4][n]: two sets of steps of four lower bounds per element through bound_slots<KC> into
 *              KC slots, sort_desc_u32 of each set, topk_merge_u32 of the two.  out [60][n]: for KC = 4 (bound_slots'
 *              maximum form; 20 rows) then KC = 8 (its insertion form; 40 rows) the raw slots of set 0, of set 1, the
 *              sorted slots of set 0, of set 1, the merged list. */
int ksched_selftest_score(ksched_ctx *ctx, int64_t n, const int64_t *req, const int64_t *alloc, double *out_score,
                          double *out_upper, double *out_recip, int32_t *out_flags);
int ksched_selftest_price_key(ksched_ctx *ctx, int64_t n, const float *price, double *out_key);
int ksched_selftest_screen(ksched_ctx *ctx, int64_t n, const int64_t *req, const int64_t *alloc, float *out_f32,
                           uint32_t *out_u32);
int ksched_selftest_rec_w(ksched_ctx *ctx, int64_t n, const float *w, const float *w2, uint32_t *out);
int ksched_selftest_threshold(ksched_ctx *ctx, int64_t n, const float *L, const uint32_t *rec, int32_t *out);
/* seed (added within ABI 6): flags bit 0 amb, bit 1 el; x [6][n] lower bounds.  out [5][n]: screen_need(v, amb, el, L),
 * then the sorted top-4 list after six bound_insert<4>. */
int ksched_selftest_seed(ksched_ctx *ctx, int64_t n, const float *v, const float *L, const uint32_t *flags,
                         const uint32_t *x, uint32_t *out);
/* touch_screen (added within ABI 6): the persistent commit's touched-node column, element = one (pod, column) pair:
 * req the pod's request, alloc the column's node state, thr the pod's list threshold, active != 0: the pod may use the
 * column.  out_f32 [4][n]: the column's staged f32 reciprocals x3 (touch_stage), the pod's screen value; out_u32 [2][n]:
 * the pod needs the exact key (touch_need), some element of its wave -- 64 consecutive elements -- does; out_key [n]:
 * touch_column's key (resource priority, all-node domain): exact where the wave needs it (-inf: not eligible), the
 * skip NaN 0x7ff8000000000bad otherwise. */
int ksched_selftest_touch_screen(ksched_ctx *ctx, int64_t n, const int64_t *req, const int64_t *alloc, const float *thr,
                                 const uint32_t *active, float *out_f32, uint32_t *out_u32, double *out_key);
int ksched_selftest_wave(ksched_ctx *ctx, int64_t ncases, const uint64_t *sort_code, const int32_t *sort_idx,
                         const double *key, const int32_t *idx, const int32_t *aux, const int32_t *cut,
                         const int32_t *nv, uint64_t *out_u64, int32_t *out_i32);
int ksched_selftest_list(ksched_ctx *ctx, int64_t n, int32_t steps, const double *key, const int32_t *idx,
                         double *out_key, int32_t *out_idx);
int ksched_selftest_slots(ksched_ctx *ctx, int64_t n, int32_t steps, const uint32_t *x, uint32_t *out);
/* Diagnostics (added within ABI 6: probe with dlsym): the stream pipeline's list-consuming stages, each as ONE launch
 * of the engine's own kernel on lists the caller built.  Neither reads node rows: a context without loaded nodes works.
 * A list entry ("Rec", 56 bytes) is {f64 key; i32 idx; i32 valid; i64 a[3]; u64 labels; f32 price; i32 pad}; a pod's
 * list is K entries, best first, the invalid ones last; entry 0's pad is the list's cut flag (candidates exist that
 * the list does not hold, all ranking below its last valid entry).  An export is a 16-byte header {i32 count; 12
 * bytes 0} and count records ("XRec", 80 bytes) {i32 idx; i32 0; i64 cur[3]; i64 sb[3]; u64 labels; f32 price; 12
 * bytes 0}.  Results nobody wrote keep the byte 0xa5.
 *   rank_merge: blocks is R rank blocks in the all-gather layout, each {Rec [nb][K]; i64 fc [nb]}; one launch of
 *               the rank merge at cursor 0 over nb pods.  out_rec [nb][K], out_fc [nb].  K in {4, 8, 16},
 *               1 <= R <= 64, 1 <= nb <= 1024, else KSCHED_E_INVALID.
 *   commit:     ONE commit, by the kernel impl names (KSCHED_COMMIT_SEQUENTIAL or KSCHED_COMMIT_SPECULATIVE), of
 *               batch 0 of a call of nb pods at batch size B: requests rc / rm / rp / sel [nb] (sel may be NULL
 *               without labels), lists Rec [nb][K], fc0 [nb] the lists' feasible counts, xin the export the batch
 *               inherits.  out_idx / out_score / out_feas [nb] (pods at or past the new cursor are unspecified);
 *               out_x: this batch's export, room for 16 + 160 B bytes; out_ctl [5]: the cursor, the batches
 *               committed, truncated, the pods placed, and the plan of batch 2.  KSCHED_E_INVALID without a launch,
 *               as the engine would refuse: K outside {4, 8, 16}, nb outside [1, B], B over 128 (speculative: 64),
 *               xin's count over 64 (speculative, whatever B: the kernel's inherited slots) or over B (sequential:
 *               its table holds 2 B nodes), a (B, K) over the sequential commit's LDS (none within these limits). */
int ksched_selftest_rank_merge(ksched_ctx *ctx, int32_t K, int32_t R, int32_t nb, const void *blocks, void *out_rec,
                               int64_t *out_fc);
int ksched_selftest_commit(ksched_ctx *ctx, int32_t impl, int32_t K, int32_t B, int32_t priority, int32_t domain,
                           int32_t use_labels, int32_t fast53, int32_t nb, const int64_t *rc, const int64_t *rm,
                           const int64_t *rp, const uint64_t *sel, const void *lists, const int64_t *fc0,
                           const void *xin, int32_t *out_idx, double *out_score, int32_t *out_feas, void *out_x,
                           int64_t *out_ctl);

/* ---- host packer: Go-exact Kubernetes quantity parsing ----
 * s == NULL means the key is absent from the ResourceList.  KSCHED_E_PARSE on the reference's
 * errFatal paths; otherwise KSCHED_OK with the reference's value (0 for unparseable floats and for
 * memory suffixes other than Ki/Mi). */
int ksched_parse_cpu(const char *s, int64_t *out);    /* parseCpu, anchor/predicate.go:10-24 */
int ksched_parse_memory(const char *s, int64_t *out); /* parseMemory, anchor/predicate.go:26-44 */
int ksched_parse_pods(const char *s, int64_t *out);   /* parsePod, anchor/predicate.go:46-53 */
int ksched_parse_price(const char *s, float *out);    /* node price annotation (README.md:43-48), f32 */

/* Packs a Kubernetes-shaped cluster into the SoA inputs above.
 *   nodes: n names + capacity strings (cpu/mem/pods, NULL = absent)       anchor/predicate.go:56-67
 *   bound pods: nb pods with node name, container range [cont_off[i], cont_off[i+1]) into the
 *     container request arrays (cpu/mem strings, NULL = absent)          anchor/predicate.go:83-105
 * Writes alloc_* (n).  KSCHED_E_UNKNOWN_NODE if a bound pod names an unknown node. */
int ksched_pack_nodes(int64_t n, const char *const *names, const char *const *cap_cpu,
                      const char *const *cap_mem, const char *const *cap_pods,
                      int64_t nb, const char *const *bound_node, const int64_t *cont_off,
                      const char *const *cont_cpu, const char *const *cont_mem,
                      int64_t *alloc_cpu, int64_t *alloc_mem, int64_t *alloc_pods);
/* requestedResource (anchor/predicate.go:69-81) for p pending pods (container ranges as above). */
int ksched_pack_pods(int64_t p, const int64_t *cont_off, const char *const *cont_cpu,
                     const char *const *cont_mem, int64_t *req_cpu, int64_t *req_mem, int64_t *req_pods);

#ifdef __cplusplus
}
#endif
#endif /* KSCHED_H */
