// ksched_ctx.h -- the context behind the C-ABI (include/ksched.h) and what the host units share: ksched_engine.hip
// (lifecycle, run / sync, the enqueue paths), ksched_data.hip (node / pod data calls), ksched_constraints.hip (the
// gang / spread / extended-resource / affinity calls of exact mode), ksched_xchg.hip (ranks meeting) and ksched_diag.hip
// (environment, traces, dumps, device error decoding).  Internal: not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "ksched.h"
#include "ksched_exact.h"
#include "ksched_kernels.h"
#include "ksched_pipe.h"
#include "ksched_stream.h"

// In-process rank group (include/ksched.h).  The all-gather is host-coordinated and synchronous:
// every rank waits for its own send block, the ranks meet, each copies every rank's block into its
// receive buffer (device-to-device on the shared device) and waits for the copies, and the ranks meet
// again before any send block can be rewritten.  No kernel ever waits on another rank's work, so the
// ranks' streams may share hardware queues (GPU_MAX_HW_QUEUES) without deadlock.  Slower than RCCL by
// a host round trip per batch: a test vehicle for the multi-rank code, not a bench path.
struct ksched_group {
    int nranks = 0, dev = 0;
    int64_t block_bytes = 0;
    std::vector<const char *> send;  // each rank's send block of the current exchange
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0, acc = 0, result = 0;
    uint64_t gen = 0;
};

// Ranks of ONE process sharing ONE device, joined by ksched_xchg_join_local: the device exchange of the
// node-sharded persistent pipeline without IPC, and their persistent kernels as ONE cooperative launch
// (k_pipe over a PipeLaunch of every rank's arguments), so every rank's grid is resident at once by
// construction.  Per call the ranks meet twice on the host: to agree on FAST53, and to launch -- the last
// rank to arrive issues the launch on its stream behind every rank's pre-launch work (events) and the others'
// streams wait for it.
struct ksched_lgroup {
    int R = 0, dev = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    bool broken = false;        // a rank never arrived: the group is unusable
    int acc = 0, result = 0;    // FAST53 agreement
    ksched::PipeLaunch L{};     // the staged launch (rank r's arguments in L.P[r])
    hipStream_t stream[ksched::kMaxLocalRanks] = {};
    hipEvent_t ready[ksched::kMaxLocalRanks] = {};
    hipEvent_t done = nullptr;
    int kc = 0, k = 0, prio = 0, dom = 0;
    bool lab = false, f53 = false;
    hipError_t launch_err = hipSuccess;
    ~ksched_lgroup() {
        hipSetDevice(dev);
        for (int r = 0; r < ksched::kMaxLocalRanks; ++r)
            if (ready[r]) hipEventDestroy(ready[r]);
        if (done) hipEventDestroy(done);
    }
};

// One device buffer and its owner: grown on demand, never shrunk, freed with its owner.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;  // the size asked for (what reserve compares against)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    // at least `need` bytes (an allocation even for 0: kernels never see a null buffer); the contents do not survive
    // a growth; on failure the buffer is empty
    hipError_t reserve(size_t need) {
        if (p && bytes >= need) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void **)&p, std::max<size_t>(need, 1));
        if (e == hipSuccess) bytes = need; else p = nullptr;
        return e;
    }
    void release() { if (p) hipFree(p); p = nullptr; bytes = 0; }
    operator T *() const { return p; }
};

// Every hipMalloc'd buffer of a context (ksched_ctx::d).  The receive ring is not here: it has its own allocator
// and rule (rx_prepare / rx_free, ksched_xchg.hip).
struct ksched_bufs {
    DevBuf<ksched::NodeRec> nodes, snap;  // the node rows; the save_state snapshot
    DevBuf<int64_t> rc, rm, rp;           // pending pods (SoA)
    DevBuf<uint64_t> sel;
    DevBuf<int32_t> oidx, ofeas;          // per-pod results
    DevBuf<double> osc;
    DevBuf<void> ws;                      // stream pipeline: part lists, exchange blocks, rank-merged lists
    DevBuf<void> xring, lring;            // stream pipeline: the commits' export ring, the merged lists' ring
    DevBuf<int64_t> cursor;               // the Ctl block ([0] cursor, [1..3] stats, ...)
    DevBuf<int32_t> err;                  // the device error word (kErr*), read by every sync
    DevBuf<int64_t> dbg, mdbg;            // KSCHED_COMMIT_STAMPS / KSCHED_MERGE_STAMPS cycle sums
    DevBuf<uint64_t> slots;               // exact mode: the cross-workgroup exchange granules
    DevBuf<int32_t> perm;                 // exact mode on one workgroup, best-price: nodes by (price asc, index asc)
    DevBuf<int32_t> gend, gplaced;        // ksched_schedule_gangs: ExactArgs::gang_end per pod, members bound per gang
    DevBuf<int32_t> sdom, scnt, sskew;    // ksched_load_spread: node -> domain, the S x D counts, the groups' skews
    DevBuf<int32_t> sword;                // ksched_schedule_spread: ExactArgs::sp_word per pod
    DevBuf<int64_t> etab, ereq;           // ksched_load_ext: the R x n table; ksched_schedule_ext: ExactArgs::ext_req
    DevBuf<int32_t> eword;                // ksched_schedule_ext: ExactArgs::ext_word per pod
    DevBuf<int32_t> adom;                 // ksched_load_affinity: node -> zone domain (-1 everywhere without a zone key)
    DevBuf<uint64_t> amem, aanti_h, aanti_z;  // ... node_member, node_anti_host, node_anti_zone
    DevBuf<uint64_t> azone, aany;         // ... {zone_member, zone_anti} per domain; the run's final {any_host, any_zone}
    DevBuf<int32_t> aword;                // ksched_schedule_affinity: ExactArgs::af_word per pod
    DevBuf<uint64_t> apod;                // ... ExactArgs::af_pod, kAffWords per pod
    DevBuf<uint64_t> aundo;               // ksched_schedule_full: a rejected gang's undo log of the affinity words,
                                          // ExactArgs::af_undo_slot [kGangMax][3], then af_undo_zone [G][kGangMax][2]
    DevBuf<void> why;                     // ksched_schedule_full_why: the NO_FIT pods' rows (WhyLayout, ksched_why.h)
    DevBuf<void> xws, xbuf;               // explain: workspace; counts + NO_FIT pod list, or one pod's state + counts
    DevBuf<void> rws;                     // ksched_rank: one chunk's pods, span lists and outputs (rank_geometry's bound)
    DevBuf<void> dws;                     // ksched_rank_full / ksched_explain_full: the groups' minima, one chunk's pods,
                                          // span lists, histograms and outputs (dry_geometry's bound)
    DevBuf<int64_t> bcpu, bmem, boff;     // ksched_load_bound: the bound-pod table (BoundTable, ksched_preempt.h)
    DevBuf<int32_t> bprio, btidx, bdepth, bseg;
    DevBuf<void> vws;                     // ksched_preempt: one chunk's pods, span parts and outputs
    DevBuf<int64_t> bext;                 // ksched_load_bound_constrained: the table's extended amounts, [bound_R][entries]
    DevBuf<uint64_t> bmask;               // ... and group masks, [entries] (zeros behind ksched_load_bound, filled on first use)
    DevBuf<void> cws;                     // ksched_preempt_constrained: the groups' minima, one chunk's pods, span parts and outputs
    DevBuf<void> pws;                     // persistent pipeline: part lists, list / export rings, progress words, ...
    DevBuf<uint64_t> trace;               // KSCHED_PERSIST_TRACE: per-batch wall-clock stamps [rows][kTraceCols]
    DevBuf<uint64_t> trace_wg;            // KSCHED_TRACE_WG: per batch and score workgroup {start, arrival}
    DevBuf<uint64_t> xdbg;                // KSCHED_XCHG_DUMP: the exchange's message hashes (PersistArgs::xdbg)
    DevBuf<int32_t> xmin;                 // k_xchg_min result
};

// Diagnostics and A/B switches, read from the environment ONCE, at ksched_create (read_env, ksched_diag.hip); never
// a tuning switch of the product.  Flags are on when the variable is a non-zero integer.
//   variable                     default  effect
//   KSCHED_PERSIST_TRACE         0        per-batch phase stamps of the persistent pipeline, summary to stderr at sync
//   KSCHED_TRACE_DUMP=<path>     unset    with PERSIST_TRACE: the raw stamps ([rows][kTraceCols] u64, 100 MHz) to <path>
//   KSCHED_TRACE_WG=<path>       unset    raw per-workgroup stamps ([batches][G] u64: scan start | arrival << 32) to <path>
//   KSCHED_XCHG_DUMP=<path>      unset    the exchange's message hashes to <path>.r<rank>.c<call> ([cap][B][R + 1] u64)
//   KSCHED_COMMIT_STAMPS / KSCHED_MERGE_STAMPS   0, 0   the commit's / the merge's phase cycle sums to stderr
//   KSCHED_DEBUG                 0        launch decisions to stderr
//   KSCHED_NO_SCREEN             0        the exact scan everywhere (A/B of the screened scan)
//   KSCHED_NO_PAIRS              0        the screened scan's exact phase by rows (A/B of the pair lists)
//   KSCHED_NO_SEED               0        the seeded scan's bound from all rows in every batch (A/B of the seed masks)
//   KSCHED_NO_TOUCH_SCREEN       0        the commit keys every touched node exactly
//   KSCHED_NO_FOLD_MASK          0        the screened commit folds every wave's partial bests and every guessed column
//   KSCHED_NO_EARLY_INH          0        the commit loads the mergers' inherited keys only after its merges' wait
//   KSCHED_POISON                0        workspace and LDS filled with 0xff before every persistent run
//   KSCHED_LDS_FILL=<u32>        unset    (without POISON) LDS only, filled with this pattern before every persistent run
//   KSCHED_LDS_ROLE / _LO / _HI  7, 0, LDS size  ... in these roles (bit mask), from / up to this byte of the dynamic LDS
//   KSCHED_JITTER=<seed>         0        random delays at the persistent pipeline's protocol points
//   KSCHED_PLAIN_LAUNCH          0        the persistent kernels without the cooperative launch API (same residency
//                                         check; profiled runs: DESIGN.md section 6.1)
//   KSCHED_EXACT1_BS             1024     the one-workgroup exact kernel's block (1024, 512, 256; A/B)
//   KSCHED_XCHG_DIAG             0        section 6.1's experiment: 1 ring zeroed by hipMemsetAsync, 2 local tags from 1
//   KSCHED_XCHG_EPOCH_BASE       0        tests: a setup's granule tags start at least here (near 2^15: wrap)
//   KSCHED_PERSIST_TIMEOUT_MS    10000    bound of every persistent-pipeline wait (tests force timeouts with 0)
//   KSCHED_EXCHANGE_TIMEOUT_MS   2000     bound of the exact kernel's cross-workgroup exchange
//   KSCHED_RESCUE_MAX / _RATE / _CAP / _LOW / _LOOK   4, 4, 16, 2, 0   the rescue policy, at its fields below
struct ksched_diag {
    bool trace = false;           // KSCHED_PERSIST_TRACE
    std::string trace_dump;       // KSCHED_TRACE_DUMP (empty: none)
    std::string trace_wg;         // KSCHED_TRACE_WG (empty: none)
    std::string xchg_dump;        // KSCHED_XCHG_DUMP (empty: none)
    bool commit_stamps = false;   // KSCHED_COMMIT_STAMPS
    bool merge_stamps = false;    // KSCHED_MERGE_STAMPS
    bool debug = false;           // KSCHED_DEBUG
    bool no_screen = false;       // KSCHED_NO_SCREEN
    bool no_pairs = false;        // KSCHED_NO_PAIRS
    bool no_seed = false;         // KSCHED_NO_SEED
    bool touch_screen = true;     // off with KSCHED_NO_TOUCH_SCREEN
    bool no_fold_mask = false;    // KSCHED_NO_FOLD_MASK
    bool early_inh = true;        // off with KSCHED_NO_EARLY_INH
    bool poison = false;          // KSCHED_POISON
    std::optional<uint32_t> lds_fill;  // KSCHED_LDS_FILL (unset: no fill)
    int lds_role = 7;             // KSCHED_LDS_ROLE
    int lds_lo = 0;               // KSCHED_LDS_LO
    std::optional<int> lds_hi;    // KSCHED_LDS_HI (unset: the kernel's dynamic LDS size, known at launch)
    uint32_t jitter = 0;          // KSCHED_JITTER
    bool plain_launch = false;    // KSCHED_PLAIN_LAUNCH
    int exact1_bs = 1024;         // KSCHED_EXACT1_BS
    int xchg_diag = 0;            // KSCHED_XCHG_DIAG
    int64_t epoch_base = 0;       // KSCHED_XCHG_EPOCH_BASE
    int64_t persist_timeout_ms = 10000;  // KSCHED_PERSIST_TIMEOUT_MS (also ksched_set_timeout)
    int64_t exchange_timeout_ms = 2000;  // KSCHED_EXCHANGE_TIMEOUT_MS
    // the rescue policy (the rescue table).  A rescue costs ~20 us of the commit's loop,
    // a truncation ~2 voided batches, so rescues pay where exhausted lists are rare and lose where they cluster
    // (the rescues of a batch that truncates anyway are wasted).  Each commit workgroup keeps a bucket of
    // credit: rescue_rate quarter rescues per batch of its own, at most rescue_cap rescues; a batch spends at
    // most rescue_max while the bucket is at least half full and rescue_low below that
    int rescue_max = 4;           // KSCHED_RESCUE_MAX (0: exhausted lists always truncate)
    int rescue_rate = 4;          // KSCHED_RESCUE_RATE, quarter rescues per batch of the workgroup
    int rescue_cap = 16;          // KSCHED_RESCUE_CAP
    int rescue_low = 2;           // KSCHED_RESCUE_LOW
    int rescue_look = 0;          // KSCHED_RESCUE_LOOK=1: also truncate when the batch's other exhausted lists would
                                  // overrun the allowance (helps a fixed budget, loses with the bucket)
};

struct ksched_ctx {
    ksched_opts o{};
    int dev = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    std::string err;
    std::optional<ksched_bufs> d{std::in_place};  // freed as a whole, at its place in ksched_destroy's order
    // nodes
    int64_t n_local = -1;
    int64_t n_global = 0;
    uint64_t max_abs_alloc = 0;  // saturating bound on |allocatable| (fast53 check)
    uint64_t sum_abs_req = 0;    // saturating sum of |request| over the staged pods
    uint64_t snap_max_abs_alloc = 0;  // max_abs_alloc of the save_state snapshot
    int64_t perm_n = -1;         // the node count d->perm was built for (-1: none; k_exact1 needs perm_n == n_local)
    bool bound_valid = false;    // ksched_load_bound's table describes the loaded nodes (every load_nodes clears it)
    int32_t bound_R = 0;         // ... its extended columns (ksched_load_bound_constrained's n_ext; ksched_load_bound: 0)
    uint64_t bound_mask_or = 0;  // ... every group mask of it ORed (ksched_load_bound: 0)
    int64_t bound_entries = 0;   // ... its entries (64 * the sum of the blocks' depths)
    bool bound_mask_dev = false; // ... d->bmask holds its masks
    int32_t spread_D = 0, spread_S = 0;  // ksched_load_spread's table; 0: none (every load_nodes clears it)
    int32_t ext_R = 0;           // ksched_load_ext's table: its resource columns; 0: none (every load_nodes clears it)
    bool aff_valid = false;      // ksched_load_affinity's table describes the loaded nodes (every load_nodes clears it)
    int32_t aff_D = 0;           // ... its zone domains (0: no zone key)
    uint64_t aff_any[2] = {};    // ... any_host, any_zone: into every affinity run by value, back from d->aany behind it
    // every constrained schedule call, for its run: the tables the launch is given, of those its kind carries (a single
    // kind's: always)
    bool run_spread = false, run_ext = false, run_aff = false;
    int64_t why_rows = 0, why_node_rows = 0;  // ksched_schedule_full_why: the rows its kRunFullWhy launch may fill in d->why
    // pods
    int64_t p = 0;
    // batched workspace
    int K = 16, KC = 4, B = 128;
    int64_t *h_cursor = nullptr;  // pinned copy of the Ctl block
    uint32_t jitter_calls = 0;    // KSCHED_JITTER: calls so far (the seed changes per call)
    hipStream_t stream2 = nullptr;  // merge + commit stream of the batched pipeline
    hipEvent_t ev_commit[4] = {}, ev_scored[4] = {}, ev_pipe[3] = {};
    // multi-GPU
    ncclComm_t comm = nullptr;
    ksched_group *group = nullptr;  // in-process rank group (instead of comm)
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool running = false;
    bool fast53 = false;
    std::vector<hipEvent_t> ev_pool;  // sampled per-family event pairs (opts.timing)
    struct Timed { int fam; int e0, e1; int64_t pairs; };
    std::vector<Timed> timed;
    size_t ev_used = 0;
    ksched_stats st{};
    // batch FailedScheduling diagnostics (ksched_explain_batch / ksched_explain_pod)
    bool explain_valid = false;  // the last state change was the last schedule call's placements
    // persistent pipeline (ksched_pipe.hip)
    uint64_t *d_prog = nullptr;   // per-workgroup progress words (in d->pws)
    int prog_G = 0, prog_B = 0, prog_rows = 0;
    int64_t xdbg_calls = 0;       // KSCHED_XCHG_DUMP: dumps written so far
    bool persist_stats = false;  // stats come from the Ctl copy queued behind the run
    int64_t commit_dbg[ksched::kCommitDbgWords] = {};  // KSCHED_COMMIT_STAMPS: the last persistent run's words (ksched_get_commit_stamps)
    int64_t persist_B = 0;
    bool seed_counted = false;    // the last persistent launch ran a kernel that writes the seeded scan's counters
    int64_t seed_stats[5] = {};   // the last persistent run's seeded-scan counters (ksched_get_seed_stats)
    // device-side candidate exchange of the node-sharded persistent pipeline (ksched_xchg_*)
    void *d_rx = nullptr;          // this rank's receive ring (rx_prepare)
    size_t rx_bytes = 0;
    bool rx_uncached = false;      // d_rx is hipDeviceMallocUncached memory (xchg_export's kind)
    char *rx_peer[ksched::kMaxXchgRanks] = {};  // every rank's ring as mapped here (own = d_rx)
    bool rx_ipc[ksched::kMaxXchgRanks] = {};    // rx_peer[r] was opened by hipIpcOpenMemHandle (closed by rx_unmap_peers)
    bool xchg_ready = false;       // rings imported: batched runs take the persistent multi-rank path
    bool xchg_run = false;         // the current run uses the exchange
    uint32_t xchg_epoch = 1;       // granule tag base of the next call (identical on every rank)
    std::shared_ptr<ksched_lgroup> lg;  // ranks of this process on this device (ksched_xchg_join_local)
    ksched_diag diag;

    int64_t trace_rows() const { return (int64_t)(d->trace.bytes / (ksched::kTraceCols * 8)); }
    int64_t trace_wg_elems() const { return (int64_t)(d->trace_wg.bytes / 8); }
};

namespace ksched {

inline int fail(ksched_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? UINT64_MAX : a + b; }

#define HIPCHK(c, expr)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (void)hipGetLastError(); /* reported here: not again by a later launch's check */   \
            return fail((c), KSCHED_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
        }                                                                                      \
    } while (0)

#define NCCLCHK(c, expr)                                                                       \
    do {                                                                                       \
        ncclResult_t r_ = (expr);                                                              \
        if (r_ != ncclSuccess)                                                                 \
            return fail((c), KSCHED_E_DEVICE, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

// The R ranks of a local group meet: `mine` runs under the lock on arrival, `last` on the last arrival
// (before anyone is released).  false: a peer never arrived within 60 s (the group is then broken).
// (A template over the callers' lambdas, so here and not in ksched_xchg.hip.)
template <class Mine, class Last>
bool lg_meet(ksched_lgroup *g, Mine mine, Last last) {
    std::unique_lock<std::mutex> lk(g->mu);
    if (g->broken) return false;
    const uint64_t gen = g->gen;
    mine();
    if (++g->arrived == g->R) {
        last();
        g->arrived = 0;
        ++g->gen;
        g->cv.notify_all();
        return true;
    }
    if (!g->cv.wait_for(lk, std::chrono::seconds(60), [&] { return g->gen != gen; })) {
        g->broken = true;
        return false;
    }
    return true;
}

// ksched_engine.hip
int run_impl(ksched_ctx *c, ExactRun run);  // ksched_run (kRunPlain), or the exact kernel over what a constraint call staged

// ksched_xchg.hip
bool group_min(ksched_group *g, int v, int *out);  // all ranks meet; the minimum of their values (false: a rank never arrived)
void fill_xchg_args(const ksched_ctx *c, ksched::PersistArgs *a);  // the exchange fields of PersistArgs
int decide_fast53(ksched_ctx *c);        // fast53 for this call, agreed by every rank over the call's transport
void xchg_end_call(ksched_ctx *c, bool failed);  // at sync: move the epoch past the call's tags
void rx_unmap_peers(ksched_ctx *c);      // forget every peer ring this context mapped
void rx_free(ksched_ctx *c);             // give the receive ring back (uncached rings: to the pool)

// ksched_diag.hip
void read_env(ksched_diag *d);           // every KSCHED_* variable, once (ksched_create)
void print_persist_trace(ksched_ctx *c);
void print_wg_busy(ksched_ctx *c);
int print_merge_stamps(ksched_ctx *c);                              // stream pipeline, KSCHED_MERGE_STAMPS
int print_commit_stamps(ksched_ctx *c, bool spc, int64_t skipped);  // stream pipeline, KSCHED_COMMIT_STAMPS
void dump_xchg(ksched_ctx *c);           // KSCHED_XCHG_DUMP
void dump_trace_wg(ksched_ctx *c);       // KSCHED_TRACE_WG
int decode_device_error(ksched_ctx *c, int32_t e);  // the device error word (kErr*) as the call's error

}  // namespace ksched
