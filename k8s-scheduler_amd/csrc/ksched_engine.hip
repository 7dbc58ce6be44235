// ksched_engine.hip -- libksched: the C-ABI (include/ksched.h) over the HIP kernels.
//
// Device residency: node state (64-B NodeRec rows), pending pods (SoA), outputs and all batch
// workspaces live in HBM for the life of the context; a schedule call moves only the pods in and the
// per-pod results out.  The batched loop keeps its cursor (first unresolved pod) on the device, so
// batches are enqueued back to back with no host round trip; the host only polls the cursor every
// few dozen batches to know when to stop.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "ksched_ctx.h"
#include "ksched_why.h"

using namespace ksched;

namespace {

// Sampled kernel timing: a (start, stop) event pair around one kernel family of one batch.
hipError_t ev_take(ksched_ctx *c, int *idx) {
    if (c->ev_used >= c->ev_pool.size()) {
        hipEvent_t e;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        c->ev_pool.push_back(e);
    }
    *idx = (int)c->ev_used++;
    return hipSuccess;
}

hipError_t ev_begin(ksched_ctx *c, bool on, int *e0, hipStream_t s) {
    if (!on) return hipSuccess;
    hipError_t r = ev_take(c, e0);
    if (r != hipSuccess) return r;
    return hipEventRecord(c->ev_pool[(size_t)*e0], s);
}

hipError_t ev_end(ksched_ctx *c, bool on, int fam, int e0, int64_t pairs, hipStream_t s) {
    if (!on) return hipSuccess;
    int e1;
    hipError_t r = ev_take(c, &e1);
    if (r != hipSuccess) return r;
    r = hipEventRecord(c->ev_pool[(size_t)e1], s);
    if (r == hipSuccess) c->timed.push_back({fam, e0, e1, pairs});
    return r;
}

// Batched-mode geometry for one schedule call.
struct BatchPlan {
    int K, KC, B, pod_groups;
    int S, n_chunks;       // score kernel: nodes per chunk, chunks
    int G;                 // score workgroups = lists per pod entering the merge
    size_t off_part, off_pcnt, off_send, off_recv, off_glists, off_gfc;
    size_t send_bytes, total;
};

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

BatchPlan plan_batch(const ksched_ctx *c) {
    BatchPlan pl{};
    pl.K = c->K;
    pl.KC = c->KC;
    pl.B = c->B;
    pl.pod_groups = (pl.B + 63) / 64;
    const int64_t n = std::max<int64_t>(c->n_local, 1);
    // NSC sub-chunks (one wave each) in workgroups of kScoreWaves: 8 waves per CU at full size,
    // >= 16 nodes per wave, <= kMergeThreads workgroups (one merge lane per list)
    const int target_waves = c->cus * 8;
    int64_t nsc = std::max<int64_t>(1, target_waves / pl.pod_groups);
    const int min_s = 16;
    nsc = std::min<int64_t>(nsc, (n + min_s - 1) / min_s);
    nsc = std::min<int64_t>(nsc, (int64_t)kMergeThreads * kScoreWaves);
    nsc = std::max<int64_t>(kScoreWaves, nsc / kScoreWaves * kScoreWaves);
    pl.n_chunks = (int)nsc;
    pl.S = (int)((n + nsc - 1) / nsc);
    const int G = pl.G = (int)(nsc / kScoreWaves);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    pl.off_part = take((size_t)2 * pl.B * G * pl.KC * sizeof(Cand));  // ring of 2: score(b+1) || merge(b)
    pl.off_pcnt = take((size_t)2 * pl.B * G * sizeof(int64_t));
    pl.send_bytes = (size_t)pl.B * pl.K * sizeof(Rec) + (size_t)pl.B * sizeof(int64_t);
    pl.off_send = take(pl.send_bytes);  // local lists + fc (also the single-GPU final lists)
    const int R = std::max(1, c->o.nranks);
    pl.off_recv = take(pl.send_bytes * R);
    pl.off_glists = take((size_t)2 * pl.B * pl.K * sizeof(Rec));  // ring of 2 (rank-merged lists)
    pl.off_gfc = take((size_t)2 * pl.B * sizeof(int64_t));
    pl.total = off;
    return pl;
}

// Batched mode, software-pipelined over two streams:
//   stream S: score(b)                     polls Ctl::committed >= b - 1 (commit(b-2) done) on the device,
//                                          then overlays / writes back b-2's commits as it scans
//   stream C: merge(b) [-> all-gather -> rank merge] -> commit(b)  (+ plan of batch b+2, publish)
// score(b) runs on every CU while commit(b-1) runs on one; commit(b) inherits the nodes committed by
// batch b-1 (its score snapshot is one batch older).  Each batch's start is planned speculatively
// (previous start + B) by the commit two batches back; a truncated batch invalidates the in-flight
// speculation, which commit skips, and plans its restart at the committed frontier.
// The commit(b-2) -> score(b) edge is a device-side flag (score(b) is already resident when it is
// released: ~2 us) instead of a cross-queue stream event (~13 us per batch measured on MI355X, even
// when the event has completed: profiles/r02_*) wherever the commit provably fits beside a resident
// score workgroup; score(b) -> merge(b) is a stream event.
int enqueue_batched(ksched_ctx *c) {
    const BatchPlan pl = plan_batch(c);
    HIPCHK(c, c->d->ws.reserve(pl.total));
    const int64_t lds = (int64_t)commit_lds_bytes(pl.B, pl.K);
    if (lds > 160 * 1024 - 4096 || pl.B > 128)
        return fail(c, KSCHED_E_INVALID, "batched mode: batch <= 128 and B*(328+48K) <= ~150 KB of LDS");
    char *ws = static_cast<char *>(c->d->ws.p);
    const int prio = c->o.priority, dom = c->o.domain;
    const bool lab = c->o.use_labels != 0;
    const int R = std::max(1, c->o.nranks);
    PodArgs pods{c->d->rc, c->d->rm, c->d->rp, c->d->sel, c->p};
    const bool f53 = c->fast53;
    // commit implementation: speculative-parallel (B <= 64, default) or the single-wave sequencer (B <= 128)
    int impl = c->o.commit_impl ? c->o.commit_impl : KSCHED_COMMIT_SPECULATIVE;
    if (impl != KSCHED_COMMIT_SEQUENTIAL && pl.B > 64) impl = KSCHED_COMMIT_SEQUENTIAL;
    const bool spc_commit = impl != KSCHED_COMMIT_SEQUENTIAL;
    hipStream_t sS = c->stream, sC = c->stream2;
    // device-side score wait only where the commit provably fits beside a resident score workgroup
    const bool score_poll = commit_fits_beside_score(pl.KC, pl.K, pl.B, spc_commit, prio, dom, lab, f53);
    constexpr int kRing = 4;  // lists / X buffers / events in flight
    const size_t xb = xbuf_bytes(pl.B);
    HIPCHK(c, c->d->xring.reserve(xb * (kRing + 1)));
    HIPCHK(c, c->d->lring.reserve(pl.send_bytes * kRing));
    auto xbuf = [&](int64_t b) -> XBuf * {  // b = -1 -> the permanently empty buffer
        const int64_t slot = b < 0 ? kRing : (b % kRing);
        return reinterpret_cast<XBuf *>(static_cast<char *>(c->d->xring.p) + (size_t)slot * xb);
    };
    Ctl *ctl = reinterpret_cast<Ctl *>(c->d->cursor.p);
    HIPCHK(c, launch_ctl_init(ctl, pl.B, c->p, 2, sS));
    for (int r = 0; r <= kRing; ++r) HIPCHK(c, hipMemsetAsync(xbuf(r == kRing ? -1 : r), 0, 8, sS));
    if (c->diag.commit_stamps) HIPCHK(c, c->d->dbg.reserve(kCommitDbgWords * sizeof(int64_t)));
    if (c->d->dbg) HIPCHK(c, hipMemsetAsync(c->d->dbg, 0, kCommitDbgWords * sizeof(int64_t), sS));
    if (c->diag.merge_stamps) HIPCHK(c, c->d->mdbg.reserve(8 * sizeof(int64_t)));
    if (c->d->mdbg) HIPCHK(c, hipMemsetAsync(c->d->mdbg, 0, 8 * sizeof(int64_t), sS));
    HIPCHK(c, hipEventRecord(c->ev_pipe[0], sS));  // stream C starts after the initialisation above
    HIPCHK(c, hipStreamWaitEvent(sC, c->ev_pipe[0], 0));
    int64_t resolved = 0, b = 0;
    double avg_progress = std::max(1.0, pl.B * 0.75);
    while (resolved < c->p) {
        int64_t m = (int64_t)std::ceil((double)(c->p - resolved) / avg_progress) + 2;
        m = std::max<int64_t>(2, std::min<int64_t>(m, 256));
        const int64_t b_end = b + m;
        for (; b < b_end; ++b) {
            const bool tm = c->o.timing && (b % (c->o.timing_every > 0 ? c->o.timing_every : 16) == 0);
            int e0 = -1;
            const int slot = (int)(b % kPlanRing);
            const int64_t *plan = &ctl->plan[slot];
            char *lists_base = static_cast<char *>(c->d->lring.p) + (size_t)(b % kRing) * pl.send_bytes;
            // S: score b once commit(b-2) is done (its plan for b and its committed nodes, which score(b)
            // overlays on the rows it reads and writes back)
            ScoreArgs sa{};
            if (b >= 2) {
                if (score_poll) { sa.wait_committed = &ctl->committed; sa.wait_target = (unsigned long long)(b - 1); }
                else HIPCHK(c, hipStreamWaitEvent(sS, c->ev_commit[(b - 2) % kRing], 0));
            }
            sa.err = c->d->err;
            sa.nodes = c->d->nodes; sa.n_local = c->n_local; sa.node_offset = c->o.node_offset;
            sa.S = pl.S; sa.n_chunks = pl.n_chunks; sa.pods = pods; sa.cursor = plan; sa.B = pl.B;
            const size_t part_elems = (size_t)pl.B * pl.G;
            sa.part = reinterpret_cast<Cand *>(ws + pl.off_part) + (size_t)(b % 2) * part_elems * pl.KC;
            sa.part_cnt = reinterpret_cast<int64_t *>(ws + pl.off_pcnt) + (size_t)(b % 2) * part_elems;
            sa.patch = xbuf(b - 2);
            MergeArgs ma{};
            ma.in = sa.part; ma.in_cnt = sa.part_cnt; ma.C_in = pl.G; ma.C_out = 1; ma.chunk_input = 1;
            ma.cursor = plan; ma.P = c->p; ma.B = pl.B;
            ma.nodes = c->d->nodes; ma.node_offset = c->o.node_offset;
            ma.dbg = c->d->mdbg;
            ma.err = c->d->err;
            ma.out_rec = reinterpret_cast<Rec *>(lists_base);
            ma.out_fc = reinterpret_cast<int64_t *>(lists_base + (size_t)pl.B * pl.K * sizeof(Rec));
            HIPCHK(c, ev_begin(c, tm, &e0, sS));
            HIPCHK(c, launch_score_topk(pl.KC, prio, dom, lab, f53, sa, pl.pod_groups, sS));
            HIPCHK(c, ev_end(c, tm, 0, e0, (int64_t)pl.B * c->n_local, sS));
            // C: merge b while stream S scores b+1 (the lists' part buffers alternate)
            HIPCHK(c, hipEventRecord(c->ev_scored[b % kRing], sS));
            HIPCHK(c, hipStreamWaitEvent(sC, c->ev_scored[b % kRing], 0));
            HIPCHK(c, ev_begin(c, tm, &e0, sC));
            HIPCHK(c, launch_merge_pod(pl.KC, pl.K, ma, sC));
            HIPCHK(c, ev_end(c, tm, 1, e0, 0, sC));
            const Rec *lists = reinterpret_cast<const Rec *>(lists_base);
            const int64_t *fc0 = reinterpret_cast<const int64_t *>(lists_base + (size_t)pl.B * pl.K * sizeof(Rec));
            if (c->comm || c->group) {  // node-sharded: exchange the local lists (a 1-rank communicator also takes this path)
                HIPCHK(c, ev_begin(c, tm, &e0, sC));
                if (c->comm) {
                    NCCLCHK(c, ncclAllGather(lists_base, ws + pl.off_recv, pl.send_bytes, ncclUint8, c->comm, sC));
                } else {
                    ksched_group *g = c->group;
                    int dummy;
                    HIPCHK(c, hipEventRecord(c->ev_pipe[0], sC));
                    HIPCHK(c, hipEventSynchronize(c->ev_pipe[0]));  // my block is final
                    g->send[(size_t)c->o.rank] = lists_base;
                    if (!group_min(g, 0, &dummy)) return fail(c, KSCHED_E_DEVICE, "rank group: a peer stopped exchanging");
                    for (int q = 0; q < R; ++q)
                        HIPCHK(c, hipMemcpyAsync(ws + pl.off_recv + (size_t)q * pl.send_bytes, g->send[(size_t)q],
                                                 pl.send_bytes, hipMemcpyDeviceToDevice, sC));
                    HIPCHK(c, hipStreamSynchronize(sC));
                    if (!group_min(g, 0, &dummy)) return fail(c, KSCHED_E_DEVICE, "rank group: a peer stopped exchanging");
                }
                MergeArgs mr{};
                mr.in = ws + pl.off_recv; mr.rank_stride = (int64_t)pl.send_bytes; mr.C_in = R; mr.C_out = 1;
                mr.cursor = plan; mr.P = c->p; mr.B = pl.B;
                mr.out_rec = reinterpret_cast<Rec *>(ws + pl.off_glists) + (size_t)(b % 2) * pl.B * pl.K;
                mr.out_fc = reinterpret_cast<int64_t *>(ws + pl.off_gfc) + (size_t)(b % 2) * pl.B;
                HIPCHK(c, launch_rank_merge(pl.K, mr, sC));
                lists = mr.out_rec;
                fc0 = mr.out_fc;
                HIPCHK(c, ev_end(c, tm, 3, e0, 0, sC));
            }
            // C: ordered commit of batch b
            CommitArgs ca{};
            ca.lists = lists; ca.fc0 = fc0; ca.pods = pods; ca.plan = plan; ca.ctl = ctl; ca.B = pl.B;
            ca.plan1 = &ctl->plan[(b + 1) % kPlanRing];
            ca.plan2 = &ctl->plan[(b + 2) % kPlanRing];
            ca.xin = xbuf(b - 1); ca.xout = xbuf(b);
            ca.out = OutArgs{c->d->oidx, c->d->osc, c->d->ofeas};
            ca.dbg = c->d->dbg;
            ca.batch = b;
            HIPCHK(c, ev_begin(c, tm, &e0, sC));
            if (spc_commit) HIPCHK(c, launch_commit_spc(pl.K, prio, dom, lab, f53, ca, sC));
            else HIPCHK(c, launch_commit(pl.K, prio, dom, lab, f53, ca, (size_t)lds, sC));
            HIPCHK(c, ev_end(c, tm, 2, e0, 0, sC));
            HIPCHK(c, hipEventRecord(c->ev_commit[b % kRing], sC));
        }
        HIPCHK(c, hipMemcpyAsync(c->h_cursor, ctl, sizeof(Ctl), hipMemcpyDeviceToHost, sC));
        HIPCHK(c, hipStreamSynchronize(sC));
        const Ctl *h = reinterpret_cast<const Ctl *>(c->h_cursor);
        if (h->cursor <= resolved) return fail(c, KSCHED_E_DEVICE, "batched mode made no progress");
        resolved = h->cursor;
        if (h->stats[0] > 0) avg_progress = std::max(1.0, (double)resolved / (double)(b));
    }
    // drain: write back the last two batches' commits (the others were applied in the pipeline)
    for (int64_t bb = std::max<int64_t>(0, b - 2); bb < b; ++bb) {
        HIPCHK(c, hipStreamWaitEvent(sS, c->ev_commit[bb % kRing], 0));
        HIPCHK(c, launch_apply_batch(xbuf(bb), c->d->nodes, c->o.node_offset, c->n_local, sS));
    }
    // the run's end event is recorded on stream S: make it cover stream C
    HIPCHK(c, hipEventRecord(c->ev_pipe[1], sC));
    HIPCHK(c, hipStreamWaitEvent(sS, c->ev_pipe[1], 0));
    if (c->d->mdbg)
        if (int rc = print_merge_stamps(c); rc != KSCHED_OK) return rc;
    const Ctl *h = reinterpret_cast<const Ctl *>(c->h_cursor);
    c->st.batches = h->stats[0];
    c->st.truncations = h->stats[1];
    c->st.placed = h->stats[2];
    c->st.pair_evals = (h->stats[0] + h->stats[3]) * (int64_t)pl.B * c->n_local;
    if (c->d->dbg) return print_commit_stamps(c, spc_commit, h->stats[3]);
    return KSCHED_OK;
}

constexpr int kXcds = 8;  // MI355X: 8 XCDs x 32 CUs

// Batched mode as ONE persistent kernel (ksched_pipe.hip): no per-batch launches, no stream events,
// node rows in LDS.  Returns 1 (not taken) when the configuration does not fit it -- the stream pipeline
// was asked for, multi-rank without the device exchange, a sequential commit (batch > 64), chunk lists
// other than 4 / 8, more lists than merge threads, or rows that do not fit in LDS -- and the stream
// pipeline runs instead.
int enqueue_persistent(ksched_ctx *c) {
    if (c->o.pipeline == KSCHED_PIPELINE_STREAM) return 1;
    // single rank, or node-sharded with the device-side exchange (the RCCL / in-process group paths
    // run the stream pipeline)
    if (!c->xchg_run && (c->comm || c->group || c->o.nranks > 1 || c->o.node_offset != 0)) return 1;
    const int K = c->K, KC = c->KC, B = c->B;
    if (B > 64 || (KC != 4 && KC != 8) || (c->o.commit_impl == KSCHED_COMMIT_SEQUENTIAL)) return 1;
    const int64_t n = c->n_local;
    // node-sharded: every rank sizes its grid for the largest shard, so all ranks take the same path
    const int64_t n_geom = c->xchg_run ? std::max<int64_t>(n, (c->n_global + c->o.nranks - 1) / c->o.nranks) : n;
    // one workgroup per CU: the commit + G score workgroups.  At least ~96 rows per workgroup: a smaller
    // grid costs scan time but every list fewer shortens the merge (one rank's share of an 8-GPU c4,
    // 12.5k nodes: G = 128 -> 22.8 us per batch, 240 -> 23.8, 64 -> 24.6; round 2)
    // Ranks of a local group share the device in ONE cooperative launch: each takes an equal share of the
    // CUs (one workgroup per CU: k_pipe's LDS admits one, checked against the occupancy query below), whole
    // XCDs' worth (multiples of 8), one CU per XCD left over as a margin
    const ksched_lgroup *lgp = c->xchg_run ? c->lg.get() : nullptr;
    // (up to 4 ranks whole XCDs each; 5..8 ranks (31 CUs each on MI355X) are not rounded: whole XCDs would leave
    // 24 CUs per rank, too few for a batch of 32's merger workgroups beside the score workgroups)
    int share = c->cus;
    if (lgp) {
        share = (c->cus - kXcds) / lgp->R;
        if (lgp->R <= 4) share = share / kXcds * kXcds;
    }
    const int wgs = std::min(share, c->o.pipe_wgs > 0 ? c->o.pipe_wgs : c->cus);
    // merger workgroups: kPipeMergeSlots pods each, one slot per pod of a batch
    const int M = (B + kPipeMergeSlots - 1) / kPipeMergeSlots;
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)wgs - kCommitWGs - M, (int64_t)kPipeMergeThreads,
                                                               (n_geom + 95) / 96}));
    if (wgs < kCommitWGs + 1 + M) return 1;
    const int R = (int)((n_geom + G - 1) / G);
    PipeLaunch L{};
    PersistArgs &a = L.P[0];
    a.rows_per_wg = R;
    a.G = G;
    a.M = M;
    a.B = B;
    L.R = 1;
    L.base[1] = kCommitWGs + G + M;
    PipeInfo info{};
    const bool f53 = c->fast53, lab = c->o.use_labels != 0;
    hipError_t e = launch_pipe(KC, K, c->o.priority, c->o.domain, lab, f53, L, 0, &info, c->stream);
    if (e == hipErrorNotSupported) return 1;
    HIPCHK(c, e);
    if (c->diag.debug)
        fprintf(stderr, "[ksched pipe] G=%d rows/wg=%d LDS %zu+%zu B, %d VGPRs, %zu B scratch, %d WG/CU\n", G, R,
                info.lds, info.static_lds, info.vgprs, info.spill, info.occ);
    if (info.lds + info.static_lds > 160 * 1024) return 1;  // the rows do not fit: the stream pipeline
    if (lgp && (info.occ < 1 || (int64_t)lgp->R * (kCommitWGs + G + M) > (int64_t)(c->cus - kXcds) * info.occ))
        return fail(c, KSCHED_E_INVALID, "local rank group: the ranks' grids do not fit the device together");
    // KSCHED_PLAIN_LAUNCH (profiled runs) has no runtime residency check: the same one made here
    if (!lgp && c->diag.plain_launch && (info.occ < 1 || (int64_t)(kCommitWGs + G + M) > (int64_t)c->cus * info.occ))
        return 1;
    // workspace: part lists [kPipeLag][B][G][KC] with the counts in entry 0's pad (score(b + kPipeLag) reuses
    // batch b's), list ring 4 x (B*K Rec + B fc), XBuf ring
    const size_t part_b = align_up((size_t)kPipeLag * B * G * KC * sizeof(Cand), 256);
    const size_t lists_b = align_up((size_t)B * K * sizeof(Rec) + (size_t)B * sizeof(int64_t), 256);
    const size_t xb = align_up(xbuf_bytes_pipe(B), 256);
    const size_t prog_b = align_up((prog_seed_off(G, B, kCommitWGs) + (size_t)G * kSeedWords) * 8, 256);
    const size_t resc_b = align_up(rescue_bytes(B), 256);
    const size_t inh_b = align_up(inh_bytes(B), 256);
    const size_t need = part_b + 4 * lists_b + 5 * xb + prog_b + resc_b + inh_b;
    if (c->d->pws.bytes < need) c->d_prog = nullptr;  // it points into the block that goes
    HIPCHK(c, c->d->pws.reserve(need));
    char *w = static_cast<char *>(c->d->pws.p);
    a.nodes = c->d->nodes; a.n_local = n;
    a.pods = PodArgs{c->d->rc, c->d->rm, c->d->rp, c->d->sel, c->p};
    a.ctl = reinterpret_cast<Ctl *>(c->d->cursor.p);
    a.part = reinterpret_cast<Cand *>(w);
    a.lring = w + part_b;
    a.lists_bytes = (int64_t)lists_b;
    a.xring = a.lring + 4 * lists_b;
    a.xbuf_bytes = (int64_t)xb;
    a.prog = reinterpret_cast<uint64_t *>(a.xring + 5 * xb);
    // the rescue of exhausted lists: each rank's merger slots scan its own shard, node-sharded ranks fold their
    // results through the rings (ksched_commit.h rescue_rank_fold)
    a.rescue = c->diag.rescue_max <= 0 ? nullptr : reinterpret_cast<char *>(a.prog) + prog_b;
    a.rescue_max = c->diag.rescue_max;
    a.rescue_rate = c->diag.rescue_rate;
    a.rescue_look = c->diag.rescue_look;
    a.rescue_cap = c->diag.rescue_cap;
    a.rescue_low = c->diag.rescue_low;
    a.touch_screen = c->diag.touch_screen ? 1 : 0;
    a.early_inh = c->diag.early_inh ? 1 : 0;
    a.no_fold_mask = c->diag.no_fold_mask ? 1 : 0;
    if (c->diag.jitter) a.jitter = c->diag.jitter * 2654435761u + (uint32_t)(++c->jitter_calls) * 40503u + 1u;
    a.inh = reinterpret_cast<char *>(a.prog) + prog_b + resc_b;
    c->d_prog = a.prog;
    c->prog_G = G;
    c->prog_rows = R;
    c->prog_B = B;
    a.out = OutArgs{c->d->oidx, c->d->osc, c->d->ofeas};
    fill_xchg_args(c, &a);
    a.err = c->d->err;
    // every wait is bounded: 10 s of the 100 MHz wall clock by default (a profiler that suspends the
    // queues for a while must not turn into a spurious timeout)
    a.timeout_ticks = c->diag.persist_timeout_ms * 100000;
    a.no_screen = c->diag.no_screen ? 1 : 0;
    a.no_pairs = c->diag.no_pairs ? 1 : 0;
    a.no_seed = c->diag.no_seed ? 1 : 0;
    if (c->diag.trace) {
        const int64_t cap = 4 * (c->p / B) + 64;
        HIPCHK(c, c->d->trace.reserve((size_t)cap * kTraceCols * 8));
        HIPCHK(c, hipMemsetAsync(c->d->trace, 0, c->d->trace.bytes, c->stream));
        a.trace = c->d->trace;
        a.trace_cap = c->trace_rows();
    }
    if (!c->diag.trace_wg.empty()) {
        const int64_t elems = (4 * (c->p / B) + 64) * (int64_t)G;
        HIPCHK(c, c->d->trace_wg.reserve((size_t)elems * 8));
        HIPCHK(c, hipMemsetAsync(c->d->trace_wg, 0, c->d->trace_wg.bytes, c->stream));
        a.trace_wg = c->d->trace_wg;
        a.trace_cap = c->trace_wg_elems() / G;
    }
    if (!c->diag.xchg_dump.empty() && c->xchg_run) {
        const int64_t cap = 4 * (c->p / B) + 64;
        const int64_t elems = (int64_t)xdbg_commit_off(cap, B, c->o.nranks, c->K) + cap * 16;
        HIPCHK(c, c->d->xdbg.reserve((size_t)elems * 8));
        HIPCHK(c, hipMemsetAsync(c->d->xdbg, 0, (size_t)elems * 8, c->stream));
        a.xdbg = c->d->xdbg;
        a.xdbg_cap = cap;
    }
    if (c->diag.commit_stamps) HIPCHK(c, c->d->dbg.reserve(kCommitDbgWords * sizeof(int64_t)));
    if (c->d->dbg) {
        HIPCHK(c, hipMemsetAsync(c->d->dbg, 0, kCommitDbgWords * sizeof(int64_t), c->stream));
        a.cdbg = c->d->dbg;
    }
    if (c->diag.merge_stamps) HIPCHK(c, c->d->mdbg.reserve(8 * sizeof(int64_t)));
    if (c->d->mdbg) {
        HIPCHK(c, hipMemsetAsync(c->d->mdbg, 0, 8 * sizeof(int64_t), c->stream));
        a.mdbg = c->d->mdbg;
    }
    hipStream_t sS = c->stream;
    if (c->diag.poison) {  // read-before-write hunting: stale workspace and LDS become 0xff everywhere
        HIPCHK(c, hipMemsetAsync(c->d->pws, 0xff, need, sS));
        a.poison_lds = (int32_t)info.lds;
        a.lds_fill = ~0u; a.lds_fill_role = 7; a.lds_fill_lo = 0; a.lds_fill_hi = (int32_t)info.lds;
    } else if (c->diag.lds_fill) {  // LDS only, a chosen pattern and range
        a.poison_lds = (int32_t)info.lds;
        a.lds_fill = *c->diag.lds_fill;
        a.lds_fill_role = c->diag.lds_role;
        a.lds_fill_lo = c->diag.lds_lo;
        a.lds_fill_hi = c->diag.lds_hi.value_or((int)info.lds);
    }
    HIPCHK(c, launch_ctl_init(a.ctl, B, c->p, kPipeLag, sS));
    // the export ring whole: its records carry batch tags (store_xrec), which an earlier call's must never match
    HIPCHK(c, hipMemsetAsync(a.xring, 0, 5 * xb, sS));
    // (the seeded scan's counters behind them: only the screened KC <= 4 kernels write and the sync then reads them)
    c->seed_counted = c->o.priority == KSCHED_PRIORITY_RESOURCE && f53 && KC <= 4;
    HIPCHK(c, hipMemsetAsync(a.prog, 0, (prog_seed_off(G, B, kCommitWGs) + (c->seed_counted ? (size_t)G * kSeedWords : 0)) * 8, sS));
    // score -> merge records carry 16-bit batch tags (1 + batch): no record of an earlier call may look current
    HIPCHK(c, hipMemsetAsync(a.part, 0, part_b, sS));
    // timing: the kernel (family 0) is bracketed by events on its stream -- one launch per call, so the
    // events cost nothing per batch and may stay on inside a timed region
    int e0 = -1;
    HIPCHK(c, ev_begin(c, c->o.timing != 0, &e0, sS));
    // cooperative launch: the runtime checks the grid against the occupancy query, so every workgroup is
    // resident at once.  A local group's ranks stage their arguments and the last to arrive launches all
    // of them as one grid on its stream, behind every rank's pre-launch work; the others' streams wait for it.
    if (lgp) {
        ksched_lgroup *g = c->lg.get();
        const int me = c->o.rank;
        HIPCHK(c, hipEventRecord(g->ready[me], sS));
        const bool met = lg_meet(
            g,
            [&] {
                g->L.P[me] = a;
                g->stream[me] = sS;
                if (g->arrived == 0) {
                    g->kc = KC; g->k = K; g->prio = c->o.priority; g->dom = c->o.domain; g->lab = lab; g->f53 = f53;
                    g->launch_err = hipSuccess;
                } else if (g->kc != KC || g->k != K || g->prio != c->o.priority || g->dom != c->o.domain ||
                           g->lab != lab || g->f53 != f53) {
                    g->launch_err = hipErrorInvalidValue;  // the ranks disagree on the kernel
                }
            },
            [&] {
                if (g->launch_err != hipSuccess) return;
                g->L.R = g->R;
                g->L.base[0] = 0;
                for (int r = 0; r < g->R; ++r) g->L.base[r + 1] = g->L.base[r] + kCommitWGs + g->L.P[r].G + g->L.P[r].M;
                hipError_t le = hipSuccess;
                for (int r = 0; r < g->R && le == hipSuccess; ++r)
                    if (r != me) le = hipStreamWaitEvent(sS, g->ready[r], 0);
                if (le == hipSuccess) le = launch_pipe(g->kc, g->k, g->prio, g->dom, g->lab, g->f53, g->L, c->diag.plain_launch ? 2 : 1,
                                                             nullptr, sS);
                if (le == hipSuccess) le = hipEventRecord(g->done, sS);
                g->launch_err = le;
            });
        if (!met) return fail(c, KSCHED_E_DEVICE, "local rank group: a peer never launched");
        if (g->launch_err != hipSuccess)
            return fail(c, KSCHED_E_DEVICE, std::string("local rank group launch: ") + hipGetErrorString(g->launch_err));
        HIPCHK(c, hipStreamWaitEvent(sS, g->done, 0));  // (a no-op on the launching rank's own stream)
        e = hipSuccess;
    } else {
        e = launch_pipe(KC, K, c->o.priority, c->o.domain, lab, f53, L, c->diag.plain_launch ? 2 : 1, nullptr, sS);
    }
    if (e == hipErrorCooperativeLaunchTooLarge && !c->xchg_run) {  // the stream pipeline runs instead
        if (c->diag.debug) fprintf(stderr, "[ksched pipe] cooperative launch too large: stream pipeline\n");
        (void)hipGetLastError();
        c->timed.clear();
        c->ev_used = 0;
        return 1;
    }
    if (e != hipSuccess) return fail(c, KSCHED_E_DEVICE, std::string("launch_pipe: ") + hipGetErrorString(e));
    HIPCHK(c, ev_end(c, c->o.timing != 0, 0, e0, c->p * n, sS));
    HIPCHK(c, hipMemcpyAsync(c->h_cursor, a.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, sS));
    c->persist_stats = true;
    c->persist_B = B;
    return KSCHED_OK;
}

// A constraint's fields of ExactArgs from the context: the per-pod words its call staged, and its table where the call
// has the constraint on (run_spread / run_ext / run_aff; off: the zeroed fields say "no table").
void args_gang(const ksched_ctx *c, ExactArgs *a) { a->gang_end = c->d->gend; a->gang_placed = c->d->gplaced; }
void args_spread(const ksched_ctx *c, ExactArgs *a) {
    a->sp_word = c->d->sword;
    if (!c->run_spread) return;
    a->sp_dom = c->d->sdom; a->sp_counts = c->d->scnt; a->sp_skew = c->d->sskew;
    a->sp_D = c->spread_D; a->sp_S = c->spread_S;
}
void args_ext(const ksched_ctx *c, ExactArgs *a) {
    a->ext_word = c->d->eword;
    if (c->run_ext) { a->ext = c->d->etab; a->ext_req = c->d->ereq; a->n_ext = c->ext_R; }
}
void args_aff(const ksched_ctx *c, ExactArgs *a) {
    a->af_word = c->d->aword; a->af_pod = c->d->apod;
    if (!c->run_aff) return;
    a->af_dom = c->d->adom; a->af_member = c->d->amem; a->af_anti_host = c->d->aanti_h;
    a->af_anti_zone = c->d->aanti_z; a->af_zone = c->d->azone; a->af_any = c->d->aany;
    a->af_any_host = c->aff_any[0]; a->af_any_zone = c->aff_any[1]; a->af_D = c->aff_D;
}
// the rows of d->why, which ksched_schedule_full_why reserved and cleared (ksched_why.h); false: it did not
bool args_why(const ksched_ctx *c, ExactArgs *a) {
    const WhyLayout l = why_layout(c->why_rows, c->why_node_rows, c->n_local);
    char *w = static_cast<char *>(c->d->why.p);
    if (!w || c->d->why.bytes < l.total) return false;
    a->why_counts = reinterpret_cast<unsigned long long *>(w + l.o_counts);
    a->why_nofit = reinterpret_cast<int64_t *>(w + l.o_nofit);
    a->why_pod = reinterpret_cast<int32_t *>(w + l.o_pod);
    a->why_reason = reinterpret_cast<uint8_t *>(w + l.o_reason);
    a->why_rows = c->why_rows; a->why_node_rows = c->why_node_rows;
    return true;
}

// A plain exact run, or the run of a constrained schedule call over what it staged (ksched_constraints.hip) -- always
// k_exact, the multi-slot kernel, under the same geometry and launch rule as a plain run.  What the kind carries:
// exact_kind (ksched_exact.h).
int enqueue_exact(ksched_ctx *c, ExactRun run) {
    if (c->o.nranks > 1) return fail(c, KSCHED_E_INVALID, "exact mode is single-GPU; use batched mode across ranks");
    const ExactKind kind = exact_kind(run);
    const int64_t n = c->n_local;
    // the whole node set in ONE workgroup's registers (k_exact1): no cross-workgroup exchange per pod
    const bool price = c->o.priority == KSCHED_PRIORITY_BEST_PRICE;
    const int max1 = price ? 16 : 4;
    ExactArgs a{};
    a.nodes = c->d->nodes; a.n = n;
    a.pods = PodArgs{c->d->rc, c->d->rm, c->d->rp, c->d->sel, c->p};
    a.out = OutArgs{c->d->oidx, c->d->osc, c->d->ofeas};
    a.err = c->d->err;
    if (run == kRunPlain && c->o.exact_wgs <= 1 && n > 0 && n <= (int64_t)kExact1Block * max1 && (!price || c->perm_n == n)) {
        int bs = kExact1Block;
        if (price && c->diag.exact1_bs == 512 && n <= 5120) bs = 512;
        if (price && c->diag.exact1_bs == 256 && n <= 5120) bs = 256;
        int npt = bs == 512 ? 10 : bs == 256 ? 20 : 1;
        while ((int64_t)bs * npt < n) npt = npt < 4 ? npt + 1 : (npt < 6 && price ? npt + 1 : (npt < 8 ? 8 : (npt < 12 ? 12 : 16)));
        HIPCHK(c, hipMemsetAsync(c->d->err, 0, sizeof(int32_t), c->stream));
        a.G = 1; a.per_wg = (int32_t)n;
        a.perm = price ? c->d->perm.p : nullptr;
        int e0 = -1;
        HIPCHK(c, ev_begin(c, c->o.timing != 0, &e0, c->stream));
        HIPCHK(c, launch_exact1(npt, bs, c->o.priority, c->o.domain, c->o.use_labels != 0, c->fast53, a, c->stream));
        HIPCHK(c, ev_end(c, c->o.timing != 0, 0, e0, c->p * n, c->stream));
        c->st.pair_evals = c->p * n;
        return KSCHED_OK;
    }
    int G = c->o.exact_wgs;
    int npt;
    if (G <= 0) {
        // resource scores are ~150 FP64 ops per pair: spread nodes thin; best-price is a compare: pack
        const int per_thread = c->o.priority == KSCHED_PRIORITY_BEST_PRICE ? 8 : 1;
        npt = 1;
        while (npt < 8 && (int64_t)kExactBlock * npt < (n + c->cus - 1) / c->cus) npt *= 2;
        while (npt < per_thread && npt < 8) npt *= 2;
        G = (int)std::max<int64_t>(1, (n + (int64_t)kExactBlock * npt - 1) / ((int64_t)kExactBlock * npt));
    } else {
        npt = 1;
        while (npt < 8 && (int64_t)G * kExactBlock * npt < n) npt *= 2;
    }
    const int64_t per_wg = (n + G - 1) / G;
    if (per_wg > (int64_t)kExactBlock * npt)
        return fail(c, KSCHED_E_INVALID, "exact mode: too many nodes per workgroup (raise exact_wgs)");
    if (G > c->cus) return fail(c, KSCHED_E_INVALID, "exact mode: more workgroups than CUs");
    HIPCHK(c, c->d->slots.reserve((size_t)2 * G * 4 * sizeof(uint64_t)));
    // a rejected gang's undo log of the affinity words -- one slot record per member, one zone record per workgroup and
    // member (written before it is read: not cleared); reserved here, before the timed span begins
    const size_t undo_slot_words = (size_t)kGangMax * 3;
    if (kind.undo) HIPCHK(c, c->d->aundo.reserve((undo_slot_words + (size_t)G * kGangMax * 2) * sizeof(uint64_t)));
    HIPCHK(c, hipMemsetAsync(c->d->slots, 0, (size_t)2 * G * 4 * sizeof(uint64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d->err, 0, sizeof(int32_t), c->stream));
    a.G = G; a.per_wg = (int32_t)per_wg; a.slots = c->d->slots;
    a.timeout_ticks = c->diag.exchange_timeout_ms * 100000;  // 100 MHz wall clock
    int e0 = -1;
    HIPCHK(c, ev_begin(c, c->o.timing != 0, &e0, c->stream));
    // the fields of every constraint the kind carries: the words its call staged, and the table where the call has it on
    if (kind.gang) args_gang(c, &a);
    if (kind.spread) args_spread(c, &a);
    if (kind.ext) args_ext(c, &a);
    if (kind.aff) args_aff(c, &a);
    if (kind.undo) { a.af_undo_slot = c->d->aundo; a.af_undo_zone = c->d->aundo.p + undo_slot_words; }
    if (kind.why && !args_why(c, &a)) return fail(c, KSCHED_E_STATE, "exact mode: the why rows are not reserved");
    HIPCHK(c, launch_exact(run, npt, c->o.priority, c->o.domain, c->o.use_labels != 0, c->fast53, a, kExactBlock,
                           G > 1 && !c->diag.plain_launch, c->stream));
    HIPCHK(c, ev_end(c, c->o.timing != 0, 0, e0, c->p * n, c->stream));
    c->st.pair_evals = c->p * n;
    return KSCHED_OK;
}

}  // namespace

// ksched_run (kRunPlain), or the run of a constrained schedule call: the exact kernel over what it staged, whatever opts.mode
int ksched::run_impl(ksched_ctx *c, ExactRun run) {
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "run before load_nodes");
    if (c->o.nranks > 1 && !c->comm && !c->group && !c->xchg_ready)
        return fail(c, KSCHED_E_STATE, "run: multi-rank context without ksched_set_comm / ksched_set_group / "
                                       "ksched_xchg_import");
    HIPCHK(c, hipSetDevice(c->dev));
    c->err.clear();
    c->st = ksched_stats{};
    c->timed.clear();
    c->ev_used = 0;
    c->st.pods = c->p;
    int mode = c->o.mode;
    if (mode == KSCHED_MODE_AUTO) mode = c->o.nranks > 1 ? KSCHED_MODE_BATCHED : KSCHED_MODE_EXACT;
    if (run != kRunPlain) mode = KSCHED_MODE_EXACT;
    c->xchg_run = c->xchg_ready && mode == KSCHED_MODE_BATCHED && c->p > 0;
    // a multi-rank batched call needs a transport: the device exchange, an RCCL communicator or a rank group
    // (never a rank committing from its own shard alone)
    if (c->o.nranks > 1 && mode == KSCHED_MODE_BATCHED && c->p > 0 && !c->xchg_run && !c->comm && !c->group)
        return fail(c, KSCHED_E_STATE, "run: multi-rank context without an exchange transport");
    if (int rr = decide_fast53(c)) return rr;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    int r = KSCHED_OK;
    if (c->p > 0) {
        c->persist_stats = false;
        if (mode == KSCHED_MODE_EXACT) {
            r = enqueue_exact(c, run);
            c->st.pipeline = KSCHED_PIPE_EXACT;
        } else {
            r = enqueue_persistent(c);
            c->st.pipeline = KSCHED_PIPE_PERSISTENT;
            if (r == 1 && c->xchg_run && !c->comm)
                r = fail(c, KSCHED_E_INVALID, "node-sharded exchange: the persistent pipeline does not fit this "
                                              "configuration and no RCCL communicator is set");
            if (r == 1) {  // not eligible: the stream pipeline
                c->xchg_run = false;
                r = enqueue_batched(c);
                c->st.pipeline = c->B > 64 || c->o.commit_impl == KSCHED_COMMIT_SEQUENTIAL ? KSCHED_PIPE_STREAM_SEQ
                                                                                          : KSCHED_PIPE_STREAM;
            }
        }
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->running = r == KSCHED_OK;
    // the call's commits move every allocatable by at most the sum of the staged requests: keep the
    // FAST53 bound true of the state the NEXT call starts from
    if (r == KSCHED_OK) c->max_abs_alloc = sat_add(c->max_abs_alloc, c->sum_abs_req);
    // (a rolled-back gang leaves no final placements for ksched_explain_batch to rebuild a pod's state from)
    // (and the explain calls know no spread, extended-resource or affinity reason)
    c->explain_valid = r == KSCHED_OK && run == kRunPlain;
    return r;
}

extern "C" {

int ksched_abi_version(void) { return KSCHED_ABI_VERSION; }

int ksched_default_opts(ksched_opts *o) {
    if (!o) return KSCHED_E_INVALID;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(ksched_opts);
    o->mode = KSCHED_MODE_AUTO;
    o->priority = KSCHED_PRIORITY_RESOURCE;
    o->domain = KSCHED_DOMAIN_ALL;
    o->device = -1;
    o->nranks = 1;
    return KSCHED_OK;
}

int ksched_create(const ksched_opts *opts, ksched_ctx **out) {
    if (!opts || !out || opts->struct_size != (int32_t)sizeof(ksched_opts)) return KSCHED_E_INVALID;
    *out = nullptr;
    if (opts->priority < 0 || opts->priority > 1 || opts->domain < 0 || opts->domain > 1 || opts->mode < 0 ||
        opts->mode > 2 || opts->nranks < 1 || opts->rank < 0 || opts->rank >= opts->nranks)
        return KSCHED_E_INVALID;
    if (opts->topk != 0 && opts->topk != 4 && opts->topk != 8 && opts->topk != 16) return KSCHED_E_INVALID;
    ksched_ctx *c = new (std::nothrow) ksched_ctx();
    if (!c) return KSCHED_E_NOMEM;
    c->o = *opts;
    c->K = opts->topk ? opts->topk : 16;
    if (opts->chunk_topk != 0 && opts->chunk_topk != 2 && opts->chunk_topk != 4 && opts->chunk_topk != 8 &&
        opts->chunk_topk != 16) { delete c; return KSCHED_E_INVALID; }
    c->KC = std::min(c->K, opts->chunk_topk ? opts->chunk_topk : 4);
    c->B = opts->batch > 0 ? opts->batch : std::min(128, 8 * c->K);
    if (c->B > 128) { delete c; return KSCHED_E_INVALID; }
    if (opts->commit_impl < 0 || opts->commit_impl > 3) { delete c; return KSCHED_E_INVALID; }
    if (opts->pipeline < 0 || opts->pipeline > 1 || opts->pipe_wgs < 0) { delete c; return KSCHED_E_INVALID; }
    read_env(&c->diag);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { delete c; return KSCHED_E_DEVICE; }
    if (opts->device >= 0) {
        if (opts->device >= ndev || hipSetDevice(opts->device) != hipSuccess) { delete c; return KSCHED_E_DEVICE; }
        c->dev = opts->device;
    } else {
        hipGetDevice(&c->dev);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->dev) == hipSuccess) c->cus = prop.multiProcessorCount;
    bool ev_ok = true;
    for (int i = 0; i < 4; ++i)
        ev_ok = ev_ok && hipEventCreateWithFlags(&c->ev_commit[i], hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&c->ev_scored[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 3; ++i) ev_ok = ev_ok && hipEventCreateWithFlags(&c->ev_pipe[i], hipEventDisableTiming) == hipSuccess;
    if (!ev_ok || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        c->d->cursor.reserve(sizeof(Ctl)) != hipSuccess ||
        c->d->err.reserve(sizeof(int32_t)) != hipSuccess ||
        hipHostMalloc((void **)&c->h_cursor, sizeof(Ctl)) != hipSuccess) {
        ksched_destroy(c);
        return KSCHED_E_DEVICE;
    }
    if (hipMemsetAsync(c->d->err, 0, sizeof(int32_t), c->stream) != hipSuccess ||  // error word read by every sync
        hipStreamSynchronize(c->stream) != hipSuccess) {
        ksched_destroy(c);
        return KSCHED_E_DEVICE;
    }
    *out = c;
    return KSCHED_OK;
}

int ksched_destroy(ksched_ctx *c) {
    if (!c) return KSCHED_OK;
    hipSetDevice(c->dev);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->stream2) hipStreamSynchronize(c->stream2);
    if (c->comm) ncclCommDestroy(c->comm);
    if (c->h_cursor) hipHostFree(c->h_cursor);
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    for (int i = 0; i < 4; ++i) {
        if (c->ev_commit[i]) hipEventDestroy(c->ev_commit[i]);
        if (c->ev_scored[i]) hipEventDestroy(c->ev_scored[i]);
    }
    for (int i = 0; i < 3; ++i) if (c->ev_pipe[i]) hipEventDestroy(c->ev_pipe[i]);
    c->d.reset();  // every device buffer but the receive ring
    rx_unmap_peers(c);
    c->lg.reset();
    rx_free(c);
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->stream2) hipStreamDestroy(c->stream2);
    delete c;
    return KSCHED_OK;
}

const char *ksched_last_error(const ksched_ctx *c) { return c ? c->err.c_str() : "null context"; }

int ksched_run(ksched_ctx *c) {
    if (!c) return KSCHED_E_INVALID;
    return run_impl(c, kRunPlain);
}

static int sync_impl(ksched_ctx *c) {
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->running) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->st.device_ms = ms;
        c->running = false;
        for (const auto &t : c->timed) {
            float km = 0.f;
            HIPCHK(c, hipEventElapsedTime(&km, c->ev_pool[(size_t)t.e0], c->ev_pool[(size_t)t.e1]));
            c->st.kernel_ms[t.fam] += km;
            c->st.kernel_launches[t.fam] += 1;
            c->st.kernel_pairs[t.fam] += t.pairs;
        }
        c->timed.clear();
    }
    if (c->persist_stats && c->d->trace && c->diag.trace) {
        print_persist_trace(c);
        print_wg_busy(c);
    }
    if (c->persist_stats && c->d->xdbg && c->xchg_run) {
        if (!c->diag.xchg_dump.empty()) dump_xchg(c);
        ++c->xdbg_calls;
    }
    if (c->persist_stats && c->d->trace_wg && c->prog_G > 0 && !c->diag.trace_wg.empty()) dump_trace_wg(c);
    if (c->persist_stats) {
        const Ctl *h = reinterpret_cast<const Ctl *>(c->h_cursor);
        c->st.batches = h->stats[0];
        c->st.truncations = h->stats[1];
        c->st.placed = h->stats[2];
        c->st.rescues = h->stats[4];
        c->st.pair_evals = (h->stats[0] + h->stats[3]) * c->persist_B * c->n_local;
        c->persist_stats = false;
        if (c->d->dbg) HIPCHK(c, hipMemcpy(c->commit_dbg, c->d->dbg, sizeof(c->commit_dbg), hipMemcpyDeviceToHost));
        if (c->d_prog) {  // the score workgroups' exact / scanned row counts (progress words 4, 5)
            std::vector<uint64_t> w((size_t)kProgWords * c->prog_G);
            HIPCHK(c, hipMemcpy(w.data(), c->d_prog, w.size() * 8, hipMemcpyDeviceToHost));
            for (int i = 0; i < 5; ++i) c->seed_stats[i] = 0;
            for (int g = 0; g < c->prog_G; ++g) {
                c->st.exact_rows += (int64_t)w[(size_t)kProgWords * g + 4];
                c->st.scan_rows += (int64_t)w[(size_t)kProgWords * g + 5];
            }
            if (c->seed_counted) {  // ... and the seeded scan's counters behind the progress words
                std::vector<uint64_t> sw((size_t)kSeedWords * c->prog_G);
                HIPCHK(c, hipMemcpy(sw.data(), c->d_prog + prog_seed_off(c->prog_G, c->prog_B, kCommitWGs), sw.size() * 8,
                                    hipMemcpyDeviceToHost));
                for (int g = 0; g < c->prog_G; ++g) {
                    const uint64_t sc = sw[(size_t)kSeedWords * g], sr = sw[(size_t)kSeedWords * g + 1];
                    c->seed_stats[0] += (int64_t)(sc & 0x1fffff);
                    c->seed_stats[1] += (int64_t)(sr & 0xffffffffffull);
                    c->seed_stats[2] += (int64_t)(sr >> 40);
                    c->seed_stats[3] += (int64_t)((sc >> 21) & 0x1fffff);
                    c->seed_stats[4] += (int64_t)(sc >> 42);
                }
            }
        }
    }
    int32_t e = 0;
    HIPCHK(c, hipMemcpy(&e, c->d->err, sizeof(e), hipMemcpyDeviceToHost));
    if (c->xchg_run) xchg_end_call(c, e != 0);
    return decode_device_error(c, e);
}

int ksched_sync(ksched_ctx *c) {
    if (!c) return KSCHED_E_INVALID;
    const int r = sync_impl(c);
    // a failed call left the node state partly committed: no FailedScheduling replay from it (callers
    // restore_state / load_nodes before retrying)
    if (r != KSCHED_OK) c->explain_valid = false;
    return r;
}

int ksched_get_stats(const ksched_ctx *c, ksched_stats *out) {
    if (!c || !out) return KSCHED_E_INVALID;
    *out = c->st;
    return KSCHED_OK;
}

int ksched_get_commit_stamps(const ksched_ctx *c, int32_t n, int64_t *out) {
    if (!c || !out || n < 0 || n > kCommitDbgWords) return KSCHED_E_INVALID;
    for (int i = 0; i < n; ++i) out[i] = c->commit_dbg[i];
    return KSCHED_OK;
}

int ksched_get_seed_stats(const ksched_ctx *c, int64_t *out) {
    if (!c || !out) return KSCHED_E_INVALID;
    for (int i = 0; i < 5; ++i) out[i] = c->seed_stats[i];
    return KSCHED_OK;
}

int ksched_set_timeout(ksched_ctx *c, int32_t persist_ms) {
    if (!c || persist_ms < 0) return KSCHED_E_INVALID;
    c->diag.persist_timeout_ms = persist_ms;
    return KSCHED_OK;
}

int ksched_set_timing(ksched_ctx *c, int32_t timing, int32_t every) {
    if (!c || every < 0) return KSCHED_E_INVALID;
    c->o.timing = timing ? 1 : 0;
    if (every > 0) c->o.timing_every = every;
    return KSCHED_OK;
}

int ksched_schedule(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                    const uint64_t *sel, int32_t *oi, double *os, int32_t *of) {
    int r = ksched_upload_pods(c, p, rc, rm, rp, sel);
    if (r != KSCHED_OK) return r;
    if ((r = ksched_run(c)) != KSCHED_OK) { ksched_sync(c); return r; }
    if ((r = ksched_sync(c)) != KSCHED_OK) return r;
    return ksched_download_results(c, p, oi, os, of);
}

}  // extern "C"
