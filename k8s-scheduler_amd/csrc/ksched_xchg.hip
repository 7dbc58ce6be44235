// ksched_xchg.hip -- libksched: ranks meeting.  A multi-rank call's transports (RCCL communicator, in-process rank
// group, device-side exchange), the receive rings and their epoch rule, the per-call agreement on FAST53.
#include <atomic>
#include <cstring>
#include <tuple>

#include "ksched_ctx.h"

namespace ksched {

// all R ranks meet; returns the minimum of their values (false: a rank never arrived)
bool group_min(ksched_group *g, int v, int *out) {
    std::unique_lock<std::mutex> lk(g->mu);
    const uint64_t gen = g->gen;
    g->acc = g->arrived == 0 ? v : std::min(g->acc, v);
    if (++g->arrived == g->nranks) {
        g->result = g->acc;
        g->arrived = 0;
        ++g->gen;
        g->cv.notify_all();
    } else if (!g->cv.wait_for(lk, std::chrono::seconds(30), [&] { return g->gen != gen; })) {
        return false;
    }
    *out = g->result;
    return true;
}

// The exchange fields of PersistArgs (node-sharded persistent pipeline; R > 1).
void fill_xchg_args(const ksched_ctx *c, PersistArgs *a) {
    a->B = c->B;
    a->node_offset = c->o.node_offset;
    a->R = c->xchg_run ? c->o.nranks : 1;
    a->rank = c->xchg_run ? c->o.rank : 0;
    a->epoch0 = c->xchg_epoch;
    a->xchg_stride = (int64_t)xchg_stride_bytes(c->K);
    for (int r = 0; r < kMaxXchgRanks; ++r) a->rx_peer[r] = c->rx_peer[r];
}

// The receive ring of a node-sharded rank, for every way an exchange is set up (ksched_xchg_export,
// ksched_xchg_join_local_ex): (re)allocated when its size or memory kind changes, and ZEROED AT EVERY SETUP, in
// this context's stream order and finished, before any peer can learn where it is.  So a ring never holds a
// granule of an earlier setup, and every setup's epochs start at 1 (tag 0 is never live) -- the one epoch rule
// of both paths.  Uncached (hipDeviceMallocUncached): a peer GPU's xGMI stores and this GPU's polls meet in
// memory, never in a stale L2 line.
// Uncached rings are never given back to the allocator: a page the allocator hands out uncached and later cached
// again (or the reverse) was read stale by the cached side -- L2 lines of its earlier cached use survive the uncached
// stores, and a later buffer on those pages (a group's node rows) read them back: the round-4 exchange failure
// (DESIGN.md section 6.1).  A process-wide pool per device keeps every uncached page uncached for good.
struct UcPool {
    std::mutex mu;
    std::vector<std::tuple<int, void *, size_t>> free;  // (device, block, bytes)
};
static UcPool &uc_pool() {
    static UcPool *p = new UcPool();  // never destroyed: its blocks outlive every context
    return *p;
}
static hipError_t uc_alloc(int dev, size_t bytes, void **out, size_t *got) {
    UcPool &P = uc_pool();
    {
        std::lock_guard<std::mutex> lk(P.mu);
        size_t best = SIZE_MAX;
        int bi = -1;
        for (int i = 0; i < (int)P.free.size(); ++i) {
            const auto &[d, q, n] = P.free[(size_t)i];
            if (d == dev && n >= bytes && n < best) { best = n; bi = i; }
        }
        if (bi >= 0) {
            *out = std::get<1>(P.free[(size_t)bi]);
            *got = best;
            P.free.erase(P.free.begin() + bi);
            return hipSuccess;
        }
    }
    *got = bytes;
    return hipExtMallocWithFlags(out, bytes, hipDeviceMallocUncached);
}
static void uc_release(int dev, void *p, size_t bytes) {
    UcPool &P = uc_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    P.free.emplace_back(dev, p, bytes);
}
void rx_free(ksched_ctx *c) {
    if (c->d_rx) {
        if (c->rx_uncached) uc_release(c->dev, c->d_rx, c->rx_bytes);
        else hipFree(c->d_rx);
    }
    c->d_rx = nullptr;
    c->rx_bytes = 0;
}

static int rx_prepare(ksched_ctx *c, size_t bytes, bool uncached) {
    if (c->d_rx && (c->rx_bytes < bytes || c->rx_uncached != uncached)) rx_free(c);
    if (!c->d_rx) {
        size_t got = bytes;
        if (uncached) HIPCHK(c, uc_alloc(c->dev, bytes, &c->d_rx, &got));
        else HIPCHK(c, hipMalloc(&c->d_rx, bytes));
        c->rx_bytes = got;
        c->rx_uncached = uncached;
    }
    // zeroed by system-scope stores, the granules' own path (a hipMemsetAsync of an uncached ring was not what the
    // persistent kernel's system-scope loads read afterwards: the round-4 failure)
    if (c->diag.xchg_diag & 1) HIPCHK(c, hipMemsetAsync(c->d_rx, 0, c->rx_bytes, c->stream));  // round 4's way
    else HIPCHK(c, launch_zero_sys(c->d_rx, c->rx_bytes, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSCHED_OK;
}

// The first granule tag no ring of this process has used yet.  Every setup starts its tags at (at least) this
// value on every rank, and every call moves it past the tags it used, so a tag never repeats in this process's
// memory: a granule left in memory that a new ring reuses can never carry a tag the new setup waits for, even
// where zeroing the ring did not reach what its loads read.
static std::atomic<uint32_t> g_epoch_next{1};
static void epoch_used_below(uint32_t e) {
    uint32_t cur = g_epoch_next.load();
    while (cur < e && !g_epoch_next.compare_exchange_weak(cur, e)) {}
}

// forget every peer ring this context mapped (IPC maps are closed; a local group's peers are plain pointers)
void rx_unmap_peers(ksched_ctx *c) {
    for (int r = 0; r < kMaxXchgRanks; ++r) {
        if (c->rx_ipc[r] && c->rx_peer[r]) hipIpcCloseMemHandle(c->rx_peer[r]);
        c->rx_peer[r] = nullptr;
        c->rx_ipc[r] = false;
    }
}

// rank r's ring as this context maps it from its IPC handle (ksched_xchg_import, and the local group's IPC mode)
static int rx_map_peer(ksched_ctx *c, int r, const uint8_t *handle) {
    hipIpcMemHandle_t h;
    static_assert(sizeof(hipIpcMemHandle_t) + 8 <= KSCHED_XCHG_HANDLE_BYTES, "ipc handle + epoch hint");
    std::memcpy(&h, handle, sizeof(h));
    void *p = nullptr;
    HIPCHK(c, hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    c->rx_peer[r] = static_cast<char *>(p);
    c->rx_ipc[r] = true;
    return KSCHED_OK;
}

// Before every call's rank barrier each rank zeroes its own ring's message and rescue areas (not the barrier
// granules the barrier itself uses): granule tags keep 15 bits (gran_tag), so a region a call does not rewrite --
// the rescue area when no rescue happens, the message slots of a call with fewer than four active batches -- could
// otherwise hold, calls later, a granule whose tag matches a wait modulo 2^15.  A peer writes into this
// ring only after it has seen this rank at the barrier, which this rank reaches after the zeroing kernel finished
// (stream order), so no granule of the call is lost.  Within a call a region is rewritten every 4 active batches
// (messages) or every 2 rescues, and both are zeroed again by the next call.
static int rx_zero_regions(ksched_ctx *c) {
    const int R = c->o.nranks;
    const size_t stride = xchg_stride_bytes(c->K);
    const size_t msg = (size_t)4 * R * c->B * stride;
    const size_t resc = xchg_rescue_off(R, c->B, stride);
    if (!c->d_rx || c->rx_bytes < xchg_ring_bytes(R, c->B, c->K)) return fail(c, KSCHED_E_STATE, "exchange ring missing");
    HIPCHK(c, launch_zero_sys(c->d_rx, msg, c->stream));
    HIPCHK(c, launch_zero_sys(static_cast<char *>(c->d_rx) + resc, 2 * (size_t)R * kXchgRescueRec, c->stream));
    return KSCHED_OK;
}

// fast53 for this call: every |alloc| + sum of |requests| < 2^52, on every rank.
int decide_fast53(ksched_ctx *c) {
    int flag = sat_add(c->max_abs_alloc, c->sum_abs_req) < (1ull << 52) ? 1 : 0;
    if (c->group) {
        int mn = flag;
        if (!group_min(c->group, flag, &mn)) return fail(c, KSCHED_E_DEVICE, "rank group: a peer never called run");
        flag = mn;
    } else if (c->xchg_run && c->lg) {
        ksched_lgroup *g = c->lg.get();
        int mn = flag;
        if (int rc = rx_zero_regions(c); rc != KSCHED_OK) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));  // finished before any rank of the group can launch
        if (!lg_meet(g, [&] { g->acc = g->arrived == 0 ? flag : std::min(g->acc, flag); }, [&] { g->result = g->acc; }))
            return fail(c, KSCHED_E_DEVICE, "local rank group: a peer never called run");
        mn = g->result;
        flag = mn;
    } else if (c->xchg_run) {
        // the ranks meet on the device through their rings (no collective launch)
        PersistArgs a{};
        fill_xchg_args(c, &a);
        a.err = c->d->err;
        a.timeout_ticks = c->diag.persist_timeout_ms * 100000;
        int32_t mn = -1;
        if (int rc = rx_zero_regions(c); rc != KSCHED_OK) return rc;  // stream-ordered before the barrier
        HIPCHK(c, launch_xchg_min(a, flag, c->d->xmin, c->stream));
        HIPCHK(c, hipMemcpyAsync(&mn, c->d->xmin, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (mn < 0) {
            c->xchg_ready = false;
            (void)hipMemsetAsync(c->d->err, 0, sizeof(int32_t), c->stream);
            return fail(c, KSCHED_E_DEVICE, "node-sharded exchange: a peer rank never met this one (device barrier timed out)");
        }
        flag = mn;
    } else if (c->comm) {
        int32_t *d = c->d->err;  // scratch word (zeroed again before use by exact mode)
        HIPCHK(c, hipMemcpyAsync(d, &flag, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        NCCLCHK(c, ncclAllReduce(d, d, 1, ncclInt32, ncclMin, c->comm, c->stream));
        HIPCHK(c, hipMemcpyAsync(&flag, d, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemsetAsync(d, 0, sizeof(int32_t), c->stream));
    }
    c->fast53 = flag != 0;
    return KSCHED_OK;
}

// At sync, after a call that used the exchange.  Every rank counted the same active batches and rescues (batch
// tags epoch0 + a, rescue tags epoch0 + q): the next call's tags start past this call's, and this process never
// uses them again.
void xchg_end_call(ksched_ctx *c, bool failed) {
    const Ctl *h = reinterpret_cast<const Ctl *>(c->h_cursor);
    // (a step of a multiple of 2^15 would give the next call's barrier granules the tag of this call's:
    // gran_tag keeps 15 bits -- skip one more)
    const uint32_t step = (uint32_t)h->nact + (uint32_t)h->stats[4] + 2u;
    c->xchg_epoch += step + ((step & 0x7fffu) == 0 ? 1u : 0u);
    epoch_used_below(c->xchg_epoch);
    if (failed) c->xchg_ready = false;  // the rings' state is unknown: later calls take the RCCL path
    c->xchg_run = false;
}

// The settings every rank of a node-sharded group must share, because every rank replays the same commit and takes
// the same rescue-or-truncate decisions (the rescue policy) or lays out the same messages: carried in the handle
// blob after the IPC handle and the epoch hint, checked by every importer (a rank with other
// KSCHED_RESCUE_* settings would wait for rescue records no peer sends).
constexpr int kPolicyWords = 8;
constexpr size_t kPolicyOff = 72;
static_assert(sizeof(hipIpcMemHandle_t) + 4 <= kPolicyOff && kPolicyOff + 4 * kPolicyWords <= KSCHED_XCHG_HANDLE_BYTES,
              "handle blob layout");
static void policy_words(const ksched_ctx *c, uint32_t *w) {
    w[0] = 0x4b534331u;  // "KSC1": a blob of this layout
    w[1] = (uint32_t)c->diag.rescue_max;
    w[2] = (uint32_t)c->diag.rescue_rate;
    w[3] = (uint32_t)c->diag.rescue_cap;
    w[4] = (uint32_t)c->diag.rescue_low;
    w[5] = (uint32_t)c->diag.rescue_look;
    w[6] = (uint32_t)c->B | (uint32_t)c->K << 16;
    w[7] = (uint32_t)c->KC | (uint32_t)c->o.priority << 8 | (uint32_t)c->o.domain << 16 | (uint32_t)(c->o.use_labels != 0) << 24;
}

}  // namespace ksched

using namespace ksched;

extern "C" {

int ksched_get_unique_id(uint8_t out_id[128]) {
    if (!out_id) return KSCHED_E_INVALID;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return KSCHED_E_DEVICE;
    static_assert(sizeof(ncclUniqueId) == 128, "nccl id size");
    std::memcpy(out_id, &id, 128);
    return KSCHED_OK;
}

int ksched_set_comm(ksched_ctx *c, const uint8_t id[128]) {
    if (!c || !id) return KSCHED_E_INVALID;
    HIPCHK(c, hipSetDevice(c->dev));
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
    NCCLCHK(c, ncclCommInitRank(&c->comm, c->o.nranks, uid, c->o.rank));
    return KSCHED_OK;
}

int ksched_group_create(int32_t nranks, int32_t device, ksched_group **out) {
    if (!out || nranks < 1 || nranks > 1024) return KSCHED_E_INVALID;
    *out = nullptr;
    ksched_group *g = new (std::nothrow) ksched_group();
    if (!g) return KSCHED_E_NOMEM;
    g->nranks = nranks;
    g->send.assign((size_t)nranks, nullptr);
    if (device >= 0) {
        if (hipSetDevice(device) != hipSuccess) { delete g; return KSCHED_E_DEVICE; }
        g->dev = device;
    } else if (hipGetDevice(&g->dev) != hipSuccess) {
        delete g;
        return KSCHED_E_DEVICE;
    }
    *out = g;
    return KSCHED_OK;
}

int ksched_group_destroy(ksched_group *g) {
    delete g;
    return KSCHED_OK;
}

int ksched_set_group(ksched_ctx *c, ksched_group *g) {
    if (!c || !g) return KSCHED_E_INVALID;
    if (g->nranks != c->o.nranks) return fail(c, KSCHED_E_INVALID, "set_group: group size != opts.nranks");
    if (c->dev != g->dev) return fail(c, KSCHED_E_INVALID, "set_group: the group's contexts must share its device");
    if (c->comm) return fail(c, KSCHED_E_STATE, "set_group: context already has an RCCL communicator");
    const int64_t bytes = (int64_t)c->B * c->K * (int64_t)sizeof(Rec) + (int64_t)c->B * (int64_t)sizeof(int64_t);
    {
        std::lock_guard<std::mutex> lk(g->mu);
        if (g->block_bytes == 0) g->block_bytes = bytes;
        else if (g->block_bytes != bytes) return fail(c, KSCHED_E_INVALID, "set_group: ranks disagree on batch / topk");
    }
    c->group = g;
    return KSCHED_OK;
}

int ksched_xchg_export(ksched_ctx *c, uint8_t handle[KSCHED_XCHG_HANDLE_BYTES]) {
    if (!c || !handle) return KSCHED_E_INVALID;
    const int R = c->o.nranks;
    if (R < 2 || R > kMaxXchgRanks) return fail(c, KSCHED_E_INVALID, "xchg_export: 2 <= nranks <= 8");
    if (c->B > 64) return fail(c, KSCHED_E_INVALID, "xchg_export: the persistent pipeline needs batch <= 64");
    if (c->group) return fail(c, KSCHED_E_STATE, "xchg_export: context uses an in-process rank group");
    if (c->lg) return fail(c, KSCHED_E_STATE, "xchg_export: context is in a local rank group (xchg_join_local)");
    HIPCHK(c, hipSetDevice(c->dev));
    // a re-export (a second setup_exchange) drops this rank's maps of the old peers before its ring is zeroed
    rx_unmap_peers(c);
    c->xchg_ready = false;
    if (int rc = rx_prepare(c, xchg_ring_bytes(R, c->B, c->K), true); rc != KSCHED_OK) return rc;
    HIPCHK(c, c->d->xmin.reserve(sizeof(int32_t)));
    hipIpcMemHandle_t h;
    HIPCHK(c, hipIpcGetMemHandle(&h, c->d_rx));
    // the blob: the IPC handle, then this process's first unused granule tag (the setup's tags start at the
    // largest hint of all ranks)
    std::memset(handle, 0, KSCHED_XCHG_HANDLE_BYTES);
    std::memcpy(handle, &h, sizeof(h));
    const uint32_t hint = g_epoch_next.load();
    std::memcpy(handle + sizeof(h), &hint, sizeof(hint));
    uint32_t pol[kPolicyWords];
    policy_words(c, pol);
    std::memcpy(handle + kPolicyOff, pol, sizeof(pol));
    return KSCHED_OK;
}

int ksched_xchg_import(ksched_ctx *c, const uint8_t *handles) {
    if (!c || !handles) return KSCHED_E_INVALID;
    if (!c->d_rx) return fail(c, KSCHED_E_STATE, "xchg_import before xchg_export");
    if (c->lg) return fail(c, KSCHED_E_STATE, "xchg_import: context is in a local rank group (xchg_join_local)");
    HIPCHK(c, hipSetDevice(c->dev));
    const int R = c->o.nranks;
    rx_unmap_peers(c);
    c->xchg_ready = false;
    {
        uint32_t mine[kPolicyWords];
        policy_words(c, mine);
        for (int r = 0; r < R; ++r)
            if (std::memcmp(handles + (size_t)r * KSCHED_XCHG_HANDLE_BYTES + kPolicyOff, mine, sizeof(mine)) != 0)
                return fail(c, KSCHED_E_INVALID, "xchg_import: rank " + std::to_string(r) +
                                                     " has other settings (batch, topk, priority, domain, labels or the "
                                                     "KSCHED_RESCUE_* policy): every rank must share them");
    }
    for (int r = 0; r < R; ++r) {
        if (r == c->o.rank) { c->rx_peer[r] = static_cast<char *>(c->d_rx); continue; }
        if (int rc = rx_map_peer(c, r, handles + (size_t)r * KSCHED_XCHG_HANDLE_BYTES); rc != KSCHED_OK) {
            rx_unmap_peers(c);
            return rc;
        }
    }
    // every ring was zeroed by its rank's export of this setup, before its handle left (rx_prepare), AND the tags
    // start at the largest hint of all ranks: beyond any tag any of their processes used, so no granule left in
    // reused memory can match (the same R blobs on every rank: the same epoch on every rank)
    uint32_t e0 = std::max<uint32_t>(1u, (uint32_t)c->diag.epoch_base);
    for (int r = 0; r < R; ++r) {
        uint32_t hint = 0;
        std::memcpy(&hint, handles + (size_t)r * KSCHED_XCHG_HANDLE_BYTES + sizeof(hipIpcMemHandle_t), sizeof(hint));
        e0 = std::max(e0, hint);
    }
    epoch_used_below(e0 + 1);
    c->xchg_ready = true;
    c->xchg_epoch = e0;
    return KSCHED_OK;
}

int ksched_xchg_ready(const ksched_ctx *c) { return c && c->xchg_ready ? 1 : 0; }

int ksched_xchg_join_local(ksched_ctx *const *ctxs, int32_t n) { return ksched_xchg_join_local_ex(ctxs, n, 0); }

int ksched_xchg_join_local_ex(ksched_ctx *const *ctxs, int32_t n, int32_t flags) {
    if (!ctxs || n < 2 || n > kMaxLocalRanks) return KSCHED_E_INVALID;
    if (flags & ~(KSCHED_XCHG_RINGS_UNCACHED | KSCHED_XCHG_RINGS_IPC)) return KSCHED_E_INVALID;
    for (int r = 0; r < n; ++r)
        if (!ctxs[r]) return KSCHED_E_INVALID;
    const bool ipc = (flags & KSCHED_XCHG_RINGS_IPC) != 0;
    const bool uncached = ipc || (flags & KSCHED_XCHG_RINGS_UNCACHED) != 0;
    ksched_ctx *c0 = ctxs[0];
    for (int r = 0; r < n; ++r) {
        ksched_ctx *c = ctxs[r];
        if (c->o.nranks != n || c->o.rank != r)
            return fail(c, KSCHED_E_INVALID, "xchg_join_local: ctxs[r] must be rank r of nranks = n");
        if (c->dev != c0->dev) return fail(c, KSCHED_E_INVALID, "xchg_join_local: the ranks must share one device");
        if (c->B > 64) return fail(c, KSCHED_E_INVALID, "xchg_join_local: the persistent pipeline needs batch <= 64");
        if (c->group) return fail(c, KSCHED_E_STATE, "xchg_join_local: context uses an in-process rank group");
        uint32_t pc[kPolicyWords], p0[kPolicyWords];
        policy_words(c, pc);
        policy_words(c0, p0);
        if (std::memcmp(pc, p0, sizeof(pc)) != 0)
            return fail(c, KSCHED_E_INVALID, "xchg_join_local: the ranks' options or rescue policies differ");
    }
    auto g = std::make_shared<ksched_lgroup>();
    g->R = n;
    g->dev = c0->dev;
    HIPCHK(c0, hipSetDevice(c0->dev));
    for (int r = 0; r < n; ++r) HIPCHK(c0, hipEventCreateWithFlags(&g->ready[r], hipEventDisableTiming));
    HIPCHK(c0, hipEventCreateWithFlags(&g->done, hipEventDisableTiming));
    // every ring through rx_prepare, as xchg_export's: (re)allocated, zeroed at this setup and finished before
    // any rank of the group can see it.  Plain device memory by default (one device, one kernel: the granules
    // are sc1 traffic inside one device's memory, like the score -> merge records); uncached as export's on request
    for (int r = 0; r < n; ++r) {
        ksched_ctx *c = ctxs[r];
        rx_unmap_peers(c);
        c->lg.reset();
        c->xchg_ready = false;
        if (int rc = rx_prepare(c, xchg_ring_bytes(n, c0->B, c0->K), uncached); rc != KSCHED_OK) return rc;
    }
    std::vector<uint8_t> handles;
    if (ipc) {  // the multi-process path's handles: each ring exported, every peer's opened from its handle
        handles.resize((size_t)n * KSCHED_XCHG_HANDLE_BYTES);
        for (int r = 0; r < n; ++r) {
            hipIpcMemHandle_t h;
            HIPCHK(ctxs[r], hipIpcGetMemHandle(&h, ctxs[r]->d_rx));
            std::memcpy(handles.data() + (size_t)r * KSCHED_XCHG_HANDLE_BYTES, &h, sizeof(h));
        }
    }
    for (int r = 0; r < n; ++r) {
        ksched_ctx *c = ctxs[r];
        for (int q = 0; q < n; ++q) {
            if (q == r || !ipc) {
                c->rx_peer[q] = static_cast<char *>(ctxs[q]->d_rx);
            } else if (int rc = rx_map_peer(c, q, handles.data() + (size_t)q * KSCHED_XCHG_HANDLE_BYTES); rc != KSCHED_OK) {
                for (int u = 0; u <= r; ++u) rx_unmap_peers(ctxs[u]);
                return rc;
            }
        }
    }
    // the same epoch rule as xchg_import: the process's first unused tag (one process: one hint)
    const uint32_t e0 = (c0->diag.xchg_diag & 2) ? 1u : std::max<uint32_t>({1u, g_epoch_next.load(), (uint32_t)c0->diag.epoch_base});
    epoch_used_below(e0 + 1);
    for (int r = 0; r < n; ++r) {
        ksched_ctx *c = ctxs[r];
        c->lg = g;
        c->xchg_ready = true;
        c->xchg_epoch = e0;
    }
    return KSCHED_OK;
}

int ksched_xchg_close(ksched_ctx *c) {
    if (!c) return KSCHED_E_INVALID;
    c->xchg_ready = false;
    c->xchg_run = false;
    rx_unmap_peers(c);  // the peers' rings are no longer used (IPC maps closed); the own ring stays allocated
    return KSCHED_OK;
}

}  // extern "C"
