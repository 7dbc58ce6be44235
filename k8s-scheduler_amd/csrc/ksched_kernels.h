// ksched_kernels.h -- what more than one kernel family of the scheduling core (gfx950 / CDNA4) shares.  The families
// have interfaces of their own: exact mode ksched_exact.h, batched mode's stream pipeline ksched_stream.h and its
// persistent pipeline ksched_pipe.h, the ranked dry run ksched_rank.h, the preemption dry run ksched_preempt.h.
// Here: the wire types of both batched pipelines (the export records XRec / XBuf, the control block Ctl, MergeArgs
// for ksched_merge.h, CommitArgs for k_commit and ksched_commit.h's commit_spc_batch, the commit's publish / plan
// steps), the device error codes, explain (ksched_explain.hip), the utility launchers (ksched_kernels.hip) and
// KSCHED_DISPATCH, the (priority, domain, labels, fast53) -> instantiation ladder of every dispatched kernel.
#pragma once

#include "ksched_device.h"

namespace ksched {

// Nodes committed by one batch, handed to the next batch's commit (which scored against a snapshot
// one batch older) and to the apply kernel that writes them into the node rows (the stream pipeline's layout;
// the persistent pipeline stores them as tagged 16-byte chunks, ksched_pipe.h).
struct alignas(16) XRec {
    int32_t idx;
    int32_t pad;
    int64_t cur[3];   // state after the batch
    int64_t sb[3];    // state before the batch (= the next batch's snapshot state)
    uint64_t labels;
    float price;
    int32_t pad2;
    int64_t pad3;
};
static_assert(sizeof(XRec) == 80, "XRec layout");

template <bool COH>
__device__ __forceinline__ void add_i64(int64_t *p, int64_t v) {
    if (COH) st_coh(p, (uint64_t)((int64_t)ld_coh(p) + v)); else *p += v;
}

struct alignas(16) XBuf {
    int32_t count;
    int32_t pad;      // the persistent pipeline's batch tag
    int64_t pad2;
    XRec e[1];        // [2 * B] follow
};

// Device-side pipeline control (one per context).  plan[] holds each in-flight batch's first pod
// (ring of kPlanRing; -1 = nothing to do), written by k_ctl_init and by the commits (plan_after_commit).
constexpr int kPlanRing = 8;
// The persistent pipeline's lag: batch b is scored against the node state after commit(b - kPipeLag),
// and commit(b) inherits the nodes the kPipeLag - 1 batches before it committed.
// The stream pipeline runs at lag 2.
constexpr int kPipeLag = 3;
// The persistent pipeline's commit workgroups: they alternate batches (ksched_pipe.hip commit_role)
constexpr int kCommitWGs = 2;
constexpr int kCtlReplicas = 8;
struct alignas(128) CtlLine {
    unsigned long long v;
    unsigned long long pad[15];
};
struct alignas(128) Ctl {
    int64_t cursor;     // first unresolved pod
    int64_t spec_next;  // next speculative batch start
    int64_t resync;     // 1: a batch truncated; the next plan restarts at cursor
    int64_t stats[5];   // batches committed, truncated, placed, skipped, pairs scored
    int64_t plan[kPlanRing];
    unsigned long long scored;     // score workgroups finished this call (device hand-off to the merge)
    unsigned long long committed;  // batches committed this call: commit(b) publishes b + 1 (release)
    int64_t cursor_at[kPlanRing];  // cursor right after commit(b), slot b % kPlanRing
    int64_t nact;                  // persistent pipeline: active batches of the call (merger 0)
    unsigned long long polls_rmw;  // persistent waits that only the periodic atomic read satisfied
    // persistent pipeline (ksched_pipe.hip).  Every polled or atomically counted word has a 128-byte line
    // of its own: one line shared by the commit's flag, 248 pollers and two families of atomic counters
    // starved single workgroups of their poll loads for seconds on MI355X.
    // per active batch a (counted identically by every workgroup), slot a % 4 -- a workgroup can run one
    // batch ahead of the slowest, so one shared counter would mix batches; four slots cannot (batch
    // a + 4 waits for commit(a + 2), which waited for every merge of a + 2)
    CtlLine arrive[4];             // score workgroups done with active batch a: G per use of the slot
    CtlLine merged[4];             // merger workgroups done with active batch a: B per use of the slot
    CtlLine committed_x[kCtlReplicas];  // Ctl::committed, one replica per XCD: workgroup w polls w % 8
    // the rescue of an exhausted candidate list (persistent pipeline, one rank): the commit publishes request
    // number q in rescue_req, each of the B merger slots scans its share of the nodes and counts its result in
    // rescue_done (B per request)
    CtlLine rescue_req;
    CtlLine rescue_done;
    // the persistent pipeline's hand-off between its two commit workgroups: commit(b) leaves two 16-byte sc1
    // granules, each tagged b + 1: {tag, export count, cursor} and {tag, rescue requests, plan of b + 3}; commit(b + 1)
    // polls them instead of Ctl::committed and a second round of loads
    CtlLine hrec;
    // merger slots done with their inherit_x2_keys stores of active batch a: counted like merged (slot a % 4, B per
    // use), so commit(a) can load the key columns before its merges' wait instead of after it
    CtlLine inh_done[4];
};

struct MergeArgs {
    const void *in;         // Cand [B][C_in][K]  or, for the rank merge, C_in rank blocks of rank_stride bytes,
                            // each {Rec [B][K]; int64 fc[B]} (the RCCL all-gather layout)
    const int64_t *in_cnt;  // [B][C_in] (Cand input only)
    int64_t rank_stride;    // bytes per rank block (rank merge)
    int32_t C_in;
    int32_t C_out;          // ceil(C_in / 64)
    int32_t chunk_input;    // 1: inputs are score-kernel chunk lists (cut when full)
    int64_t *dbg;           // diagnostics only (KSCHED_MERGE_STAMPS): per-phase cycle sums, else null
    Cand *out;              // [B][C_out][K] (non-final)
    int64_t *out_cnt;       // [B][C_out]
    Rec *out_rec;           // [B][K]  (final)
    int64_t *out_fc;        // [B]
    const NodeRec *nodes;   // Cand input: gather node snapshot state
    int64_t node_offset;
    const int64_t *cursor;
    int64_t P;
    int32_t B;
    int32_t p0_known;   // 1: p0v is this batch's first pod (the persistent score grid read it already)
    int64_t p0v;
    int32_t *err;                        // device error word
    uint32_t *lds_msg;                   // non-null: the final list goes to LDS as a pod message (msg_words(K))
    uint32_t tag;                        // persistent pipeline: the batch's 16-bit record tag (score_role)
};

// One pod's merged candidate list as 32-bit words, the unit the ranks exchange in the persistent
// multi-rank pipeline: K Rec rows (14 words each, the Rec layout) then the feasible count (2 words).
constexpr int kRecWords = (int)(sizeof(Rec) / 4);
constexpr int msg_words(int K) { return K * kRecWords + 2; }

struct PersistArgs;   // ksched_pipe.h
struct PersistLocal;  // ksched_pipe.h
struct CommitArgs {
    const Rec *lists;       // [B][K]
    const int64_t *fc0;     // [B]
    PodArgs pods;
    const int64_t *plan;    // this batch's plan slot
    const int64_t *plan1;   // the next batch's plan slot (already set)
    int64_t *plan2;         // the slot of the batch after next: written by this commit
    Ctl *ctl;
    int32_t B;
    const XBuf *xin;        // nodes committed by the previous batch (relative to this batch's snapshot)
    const XBuf *xin2;       // persistent pipeline (lag 3): nodes committed two batches earlier; else null
    XBuf *xout;             // nodes committed by this batch
    OutArgs out;
    int64_t *dbg;           // diagnostics only (KSCHED_COMMIT_STAMPS): per-phase cycle sums, else null
    int64_t batch;          // this batch's index in the call (published to Ctl::committed when done)
    int64_t *cursor_at;     // persistent pipeline: &Ctl::cursor_at[batch % kPlanRing] (else null)
    PersistLocal *loc;      // persistent pipeline (COH): the commit workgroup's LDS control state
    int32_t release;        // COH: also write back the XCD's L2 (agent release) before Ctl::committed
    char *rescue;           // persistent pipeline: the rescue request / results (else null: truncate)
    int32_t rescue_n;       // merger slots serving a rescue (= B)
    int32_t rescue_max;     // rescues per batch; the next exhausted list truncates the batch
    int32_t rescue_cap;     // persistent: the rescue bucket's capacity, in rescues
    int32_t rescue_low;     // persistent: rescues per batch while the bucket is below half full
    int32_t rescue_look;    // persistent: skip a rescue when the batch's exhausted lists already overrun the credit
    int32_t rescue_rate;    // persistent: the bucket's refill per batch of this workgroup, in quarter rescues (a batch
                            // spends at most min(rescue_max, credit) rescues; rate >= 4 * rescue_max: a fixed budget)
    int32_t touch_screen;   // persistent commit: the touched-node screen on (KSCHED_NO_TOUCH_SCREEN=1 turns it off)
    uint32_t fold_all;      // screened commit: ~0u folds every wave's partials and every guessed column (KSCHED_NO_FOLD_MASK=1),
                            // 0 only those its fold masks name (ksched_commit.h kFoldMaskBytes)
    const char *inh;        // persistent commit: the mergers' keys of the older export (inherit_x2_keys), else null
    int64_t timeout_ticks;  // bound of the rescue wait
    int32_t *err;           // device error word (kErrWaitRescue)
    uint64_t *trace_row;    // KSCHED_PERSIST_TRACE: this batch's trace row (else null)
    const PersistArgs *xp;  // persistent pipeline: its arguments (R > 1: the rescue's rank fold through the rings)
    int64_t dbg_act;        // diagnostics (KSCHED_XCHG_DUMP): this batch's active-batch index
};
// CommitArgs::dbg, in 8-byte words (ksched_get_commit_stamps; include/ksched.h names the words)
constexpr int kCommitDbgWords = 48;
// k_commit_spc's workgroup (wave 0 guesses and checks, 8 waves evaluate); commit_spc_batch's default size in k_pipe too
constexpr int kSpcThreads = 512;

// Commit(b) -> score(b + lag) hand-off on the device (lag 2 on the stream pipeline, kPipeLag in k_pipe): the
// committing wave drains its stores, writes back the XCD L2 (agent release) and publishes
// Ctl::committed = b + 1; the later score polls it instead of waiting
// on a cross-queue stream event (~12 us per hand-off).  Call from ONE wave that
// made every global store of the commit (the others made none).
// COH (persistent pipeline): every handed-off store was an sc1 store, so no L2 write-back is needed.
// COH (persistent pipeline): the caller stored Ctl::cursor_at (store_cursor_at) before the drain in front of its
// hand-off record, so every store a reader of Ctl::committed needs has landed: no store and no drain here (the
// hand-off record itself is read only by the next commit, which polls it).
template <bool COH = false>
__device__ __forceinline__ void publish_committed(const CommitArgs &A) {
    if (!COH) {
        if ((threadIdx.x & 63) == 0 && A.cursor_at) st_coh(A.cursor_at, ld_coh(&A.ctl->cursor));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if ((threadIdx.x & 63) == 0) {
        if (!COH || A.release) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (COH)  // two commit workgroups: a maximum, so the count never steps back
            __hip_atomic_fetch_max(&A.ctl->committed, (unsigned long long)A.batch + 1ull, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        else
            __hip_atomic_store(&A.ctl->committed, (unsigned long long)A.batch + 1ull, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    // persistent pipeline: the per-XCD replicas (lanes 0..7 of the publishing wave, one each)
    if (COH && (threadIdx.x & 63) < kCtlReplicas)
        __hip_atomic_fetch_max(&A.ctl->committed_x[threadIdx.x & 63].v, (unsigned long long)A.batch + 1ull,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Speculative planning, done by the commit of batch k for batch k+2 (stream order makes plan(k+2)
// visible to score(k+2), which waits for commit(k)): after a truncation restart at the committed
// frontier, otherwise continue one batch after plan(k+1).  -1 = past the last pod.
template <bool COH = false>
__device__ __forceinline__ void plan_after_commit(const CommitArgs &A, bool truncated, int64_t cursor) {
    const int64_t n1 = load_i64<COH>(A.plan1);
    int64_t nx = truncated ? cursor : (n1 < 0 ? -1 : n1 + A.B);
    if (nx >= A.pods.p) nx = -1;
    store_i64<COH>(A.plan2, nx);
}

// the device error word (the `err` of every kernel argument struct, all families): a call's first error,
// decoded by the host at sync (decode_device_error, ksched_diag.hip, has each code's meaning)
enum : int32_t { kErrExactExchange = 1, kErrStreamMergeWait = 2, kErrStreamScoreWait = 4,
                 // the persistent pipeline's waits
                 kErrWaitMerged = 5, kErrWaitCommit = 6, kErrWaitArrive = 7, kErrScorePlan = 8, kErrCommitPlan = 9,
                 kErrWaitPeerLists = 10, kErrRankBarrier = 11, kErrWaitRescue = 12,
                 kErrBadIndex = 14, kErrLdsCanary = 15 };

// FailedScheduling diagnostics of a whole schedule call (ksched_explain.hip).
struct ExplainArgs {
    const int32_t *idx;           // the call's results (global node index | NO_FIT | NO_POSITIVE_SCORE)
    int64_t p;
    const int64_t *rc, *rm, *rp;  // the call's pods
    const uint64_t *sel;
    const NodeRec *nodes;         // this rank's node rows after the call
    int64_t n_local, node_lo;
    bool use_labels;
    int32_t *fpod_out;            // explain_batch: the NO_FIT pods, in pod order (device, >= p entries)
    int64_t *n_nofit;             // explain_batch: their number (host)
    int64_t q_rc, q_rm, q_rp;     // explain_pod_at: that pod's request
    uint64_t q_sel;
};
// counts[f][kNumReasons] (zeroed by the caller) for the f-th NO_FIT pod; ws is a growable workspace.
hipError_t explain_batch(const ExplainArgs &a, void **ws, size_t *ws_bytes, unsigned long long *counts, hipStream_t s);
// per-node reasons + counts of ONE pod against the state it saw at its turn (state: 3 * n_local int64)
hipError_t explain_pod_at(const ExplainArgs &a, int64_t pod, int64_t *state, uint8_t *reason,
                          unsigned long long *counts, hipStream_t s);

// the utility launchers (ksched_kernels.hip)
hipError_t launch_prep_nodes(NodeRec *nodes, int64_t n, hipStream_t s);
constexpr int kNumReasons = 5;  // fit, Insufficient CPU, Insufficient Memory, Insufficient Pod, labels
hipError_t launch_explain(const NodeRec *nodes, int64_t n, int64_t rc, int64_t rm, int64_t rp, uint64_t sel,
                          bool use_labels, uint8_t *reason, unsigned long long *counts, hipStream_t s);
hipError_t launch_apply_delta(NodeRec *nodes, int64_t n, int64_t k, const int32_t *idx, const int64_t *d,
                              hipStream_t s);
hipError_t launch_ctl_init(Ctl *ctl, int B, int64_t P, int lag, hipStream_t s);
// zero `bytes` (a multiple of 8) at p with system-scope 8-byte stores: the path the exchange's granules take
// (a hipMemset of an uncached ring was not what a later kernel's system-scope loads read: DESIGN.md section 6.1)
hipError_t launch_zero_sys(void *p, size_t bytes, hipStream_t s);
// diagnostics: qdiv(a, b, recip(b)) against the native a / b, bit for bit
hipError_t launch_selftest_div(int64_t n, const double *a, const double *b, double *native, double *fast,
                               hipStream_t s);
// diagnostics: the score, screen, record and wave primitives on arrays of operands (ksched_selftest.hip; device
// pointers, layouts at each kernel there)
struct WaveTestArgs {
    int64_t ncases;           // one 64-lane workgroup each; per-lane arrays hold ncases * 64 elements
    const uint64_t *scode;    // [6][lanes] (code, idx) pairs in sorted runs of 1, 2, 4, 8, 16, 32
    const int32_t *sidx;
    const double *key;        // [lanes] the arg-bests' (key, idx, aux)
    const int32_t *kidx, *aux;
    const int32_t *cut, *nv;  // [ncases] list_thr_bits: the list is cut; its valid entries are lanes < nv
    uint64_t *ocode;          // [6][lanes] wave_sort_desc<RUN>
    int32_t *oidx;
    int32_t *rank;            // [lanes] wave_rank of the lane's own pair (arrangement 0)
    uint64_t *red_max;        // [lanes] wave_max_u64(code), wave_sum_i64(code), wave_min_i32(idx) (arrangement 0)
    int64_t *red_sum;
    int32_t *red_min;
    uint64_t *red_or;         // [lanes] wave_or_u64(code) (arrangement 0)
    uint64_t *ab_key;         // [2][lanes] wave_argbest, wave_argbest_fast
    int32_t *ab_idx, *ab_aux;
    uint64_t *kcode;          // [lanes] key_code(key)
    int32_t *thr;             // [lanes] list_thr_bits
};
hipError_t launch_selftest_score(int64_t n, const int64_t *req, const int64_t *alloc, double *score, double *upper,
                                 double *rcp, int32_t *flags, hipStream_t s);
hipError_t launch_selftest_price(int64_t n, const float *price, double *key, hipStream_t s);
hipError_t launch_selftest_screen(int64_t n, const int64_t *req, const int64_t *alloc, float *f, uint32_t *u,
                                  hipStream_t s);
hipError_t launch_selftest_rec_w(int64_t n, const float *w, const float *w2, uint32_t *out, hipStream_t s);
hipError_t launch_selftest_threshold(int64_t n, const float *L, const uint32_t *rec, int32_t *out, hipStream_t s);
hipError_t launch_selftest_seed(int64_t n, const float *v, const float *L, const uint32_t *flags, const uint32_t *x,
                                uint32_t *out, hipStream_t s);
hipError_t launch_selftest_touch_screen(int64_t n, const int64_t *req, const int64_t *alloc, const float *thr,
                                        const uint32_t *active, float *f, uint32_t *u, double *key, hipStream_t s);
hipError_t launch_selftest_wave(const WaveTestArgs &a, hipStream_t s);
hipError_t launch_selftest_list(int64_t n, int S, const double *key, const int32_t *idx, double *okey, int32_t *oidx,
                                hipStream_t s);
hipError_t launch_selftest_slots(int64_t n, int steps, const uint32_t *x, uint32_t *out, hipStream_t s);

// (priority, domain, labels, fast53) -> instantiation.  Best-price always ranges over feasible nodes
// and never divides (fast53 irrelevant).
#define KSCHED_DISPATCH(prio, dom, lab, f53, CALL)                                              \
    do {                                                                                        \
        if ((prio) == kPrioPrice) {                                                             \
            constexpr int P_ = kPrioPrice, D_ = kDomFeasible; constexpr bool F_ = false;        \
            if (lab) { constexpr bool L_ = true; return CALL; }                                 \
            else { constexpr bool L_ = false; return CALL; }                                    \
        }                                                                                       \
        constexpr int P_ = kPrioResource;                                                       \
        if ((dom) == kDomFeasible) {                                                            \
            constexpr int D_ = kDomFeasible;                                                    \
            if (lab) { constexpr bool L_ = true;                                                \
                if (f53) { constexpr bool F_ = true; return CALL; } else { constexpr bool F_ = false; return CALL; } } \
            else { constexpr bool L_ = false;                                                   \
                if (f53) { constexpr bool F_ = true; return CALL; } else { constexpr bool F_ = false; return CALL; } } \
        } else {                                                                                \
            constexpr int D_ = kDomAll;                                                         \
            if (lab) { constexpr bool L_ = true;                                                \
                if (f53) { constexpr bool F_ = true; return CALL; } else { constexpr bool F_ = false; return CALL; } } \
            else { constexpr bool L_ = false;                                                   \
                if (f53) { constexpr bool F_ = true; return CALL; } else { constexpr bool F_ = false; return CALL; } } \
        }                                                                                       \
    } while (0)

}  // namespace ksched
