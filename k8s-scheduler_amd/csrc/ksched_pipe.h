// ksched_pipe.h -- the interface of the persistent pipeline (ksched_pipe.hip): batched mode as
// ONE kernel, k_pipe, whose workgroups take roles -- kCommitWGs commit workgroups that alternate batches, G score
// and M merger workgroups -- joined by device counters in Ctl instead of launches and stream events.  Here: its
// arguments and launcher, what its commit (ksched_commit.h's COH paths) shares with the other roles (the tagged export
// records, the rescue request), progress words, bounded waits, trace and jitter hooks, the R > 1 exchange rings.
#pragma once

#include "ksched_kernels.h"

namespace ksched {

// The persistent pipeline's export records: 96 B, six 16-byte chunks, each led by the exporting batch's tag (batch
// + 1; the ring is zeroed before every launch, so 0 is never live): {tag, idx, cur0} {tag, cur1, cur2.lo} {tag,
// cur2.hi, sb0} {tag, sb1, sb2.lo} {tag, sb2.hi, labels} {tag, price, -, -}.  A consumer that polls the records
// themselves knows every chunk it holds is the batch's (MI355X_MICROARCH R2: a 16-byte sc1 access is untorn) with
// no drained flag in front of them -- the commit(b - 1) -> commit(b) hand-off reads export(b - 1) in the same
// round of loads as the hand-off record.  The score workgroups' export apply reads the first three (idx, cur).
constexpr uint32_t kXRecPipe = 96;
constexpr size_t xbuf_bytes_pipe(int B) { return 16 + (size_t)2 * B * kXRecPipe; }
__device__ __forceinline__ int64_t w64(uint32_t lo, uint32_t hi) { return (int64_t)(((uint64_t)hi << 32) | lo); }

// entry i of the array at (wave-uniform) e: one buffer resource for the wave, the lane's record by offset (a
// per-lane base would make the resource divergent, which the compiler serialises lane by lane).  Persistent
// layout; true when every chunk carries `tag` (callers that validated a header pass any tag and ignore it).
__device__ __forceinline__ bool load_xrec_pipe(const XRec *e, int i, uint32_t tag, XRec *o) {
    const __amdgpu_buffer_rsrc_t r = coh_rsrc(e);
    const uint32_t off = (uint32_t)i * kXRecPipe;
    u32x4 c[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = ld_coh16(r, off + 16u * k);
    o->idx = (int32_t)c[0].y; o->pad = 0;
    o->cur[0] = w64(c[0].z, c[0].w); o->cur[1] = w64(c[1].y, c[1].z); o->cur[2] = w64(c[1].w, c[2].y);
    o->sb[0] = w64(c[2].z, c[2].w); o->sb[1] = w64(c[3].y, c[3].z); o->sb[2] = w64(c[3].w, c[4].y);
    o->labels = (uint64_t)w64(c[4].z, c[4].w);
    o->price = __uint_as_float(c[5].y); o->pad2 = 0; o->pad3 = 0;
    return (c[0].x == tag) & (c[1].x == tag) & (c[2].x == tag) & (c[3].x == tag) & (c[4].x == tag) & (c[5].x == tag);
}

// COH: the persistent layout; else the stream pipeline's plain records (commit_spc_batch serves both)
template <bool COH>
__device__ __forceinline__ XRec load_xrec(const XRec *e, int i) {
    if constexpr (!COH) {
        return e[i];
    } else {
        XRec o;
        (void)load_xrec_pipe(e, i, 0u, &o);
        return o;
    }
}

// tag: the persistent layout's chunk tag (the exporting batch + 1); unused by the stream pipeline's plain records
template <bool COH>
__device__ __forceinline__ void store_xrec(XRec *e, int i, const XRec &o, uint32_t tag) {
    if constexpr (!COH) {
        e[i] = o;
    } else {
        const __amdgpu_buffer_rsrc_t r = coh_rsrc(e);
        const uint32_t b = (uint32_t)i * kXRecPipe;
        auto lo = [](int64_t v) { return (uint32_t)(uint64_t)v; };
        auto hi = [](int64_t v) { return (uint32_t)((uint64_t)v >> 32); };
        st_coh16(r, b, u32x4{tag, (uint32_t)o.idx, lo(o.cur[0]), hi(o.cur[0])});
        st_coh16(r, b + 16, u32x4{tag, lo(o.cur[1]), hi(o.cur[1]), lo(o.cur[2])});
        st_coh16(r, b + 32, u32x4{tag, hi(o.cur[2]), lo(o.sb[0]), hi(o.sb[0])});
        st_coh16(r, b + 48, u32x4{tag, lo(o.sb[1]), hi(o.sb[1]), lo(o.sb[2])});
        st_coh16(r, b + 64, u32x4{tag, hi(o.sb[2]), lo((int64_t)o.labels), hi((int64_t)o.labels)});
        st_coh16(r, b + 80, u32x4{tag, __float_as_uint(o.price), 0u, 0u});
    }
}

// The rescue request the commit writes (PersistArgs::rescue; sc1 stores, then Ctl::rescue_req) and the merger
// slots' results after it: {rc, rm, rp, sel, nT} and the touched set's node indices, then Rec res[B].
constexpr int kRescueMaxT = 256;  // >= the persistent commit's touched slots (spc_slots<true>() + 1)
struct alignas(16) RescueReq {
    int64_t rc, rm, rp;
    uint64_t sel;
    int64_t nT;
    int64_t pad;
    int64_t ti[kRescueMaxT];
};
constexpr size_t kRescueResOff = (sizeof(RescueReq) + 127) / 128 * 128;
constexpr size_t rescue_bytes(int B) { return kRescueResOff + (size_t)B * sizeof(Rec); }

// A commit workgroup's private control state (LDS): the commit workgroups are the only writers of the plans,
// the cursor, the stats and the export once their kernel runs, so each reads its own copies (handed over by
// Ctl::hrec) instead of loading them back from HBM -- every global load of the commit's serial chain costs ~1-2 us.
struct PersistLocal {
    int64_t plan[kPlanRing];
    int64_t cursor;
    int64_t stats[5];  // as Ctl::stats; [4] = rescues
    int32_t xcount;   // entries of the previous batch's export
    int32_t xcount2;  // entries of the export of the batch before it (both are inherited: lag kPipeLag)
    int64_t rseq;     // rescue requests issued this call
    int32_t rescue_credit;  // the rescue bucket, in quarter rescues (CommitArgs::rescue_rate)
};

// KSCHED_XCHG_DUMP's list sums: (key, idx | valid) words of a pod's merged list as written / as the commit loaded
// them, [cap][B][2] u64 after the hashes and the messages
__device__ __forceinline__ uint64_t dbg_mix(uint64_t w0, uint64_t w1, int q) {
    return (w0 * 0x9e3779b97f4a7c15ull + w1) * (uint64_t)(2 * q + 1);
}
__host__ __device__ inline size_t xdbg_sums_off(int64_t cap, int B, int R, int K) {
    return (size_t)cap * B * (R + 1) + ((size_t)16 * B * (K * 14 + 2) + 1) / 2;
}
// ... then per active batch the commit's summary [cap][8] u64 (ksched_commit.h)
__host__ __device__ inline size_t xdbg_commit_off(int64_t cap, int B, int R, int K) {
    return xdbg_sums_off(cap, B, R, K) + (size_t)cap * B * 2;
}

// every replica of Ctl::committed (the persistent pipeline's end and error paths; lanes 0..7)
__device__ __forceinline__ void publish_committed_all(Ctl *ctl, unsigned long long v) {
    const int l = threadIdx.x & 63;
    if (l == 0) __hip_atomic_store(&ctl->committed, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (l < kCtlReplicas) __hip_atomic_store(&ctl->committed_x[l].v, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One rank's arguments of k_pipe.
struct PersistArgs {
    NodeRec *nodes;
    int64_t n_local;
    PodArgs pods;
    Ctl *ctl;
    int32_t B, G, rows_per_wg;
    int32_t M;              // merger workgroups (after the G score workgroups): kPipeMergeSlots pod slots each
    Cand *part;             // [kPipeLag][B][G][KC], entry 0's pad = the list's predicate count
    char *lring;            // 4 x {Rec [B][K]; int64 fc[B]}
    int64_t lists_bytes;
    char *xring;            // 4 XBufs + the permanently empty one (slot 4)
    int64_t xbuf_bytes;
    OutArgs out;
    int32_t *err;           // device error word (kErrWait* .. kErrLdsCanary)
    int64_t timeout_ticks;
    int32_t no_screen;      // diagnostics (KSCHED_NO_SCREEN): the exact scan in every batch
    int32_t no_pairs;       // diagnostics (KSCHED_NO_PAIRS): the screened scan's exact phase by rows, never by pairs
    int32_t screen_ok;      // the screened scan's reciprocals fit in a score workgroup's LDS
    int32_t screen_h;       // ... and so do pass 1's per-pair records (KC = 8 kernels); KC <= 4 kernels: a wave's rows fit
                            // one 64-bit mask (the seeded scan, which keeps no records)
    // optional (KSCHED_PERSIST_TRACE): wall-clock stamps per batch, [trace_cap][kTraceCols]
    uint64_t *trace;
    int64_t trace_cap;
    // optional (KSCHED_TRACE_WG=<path>): per batch and score workgroup {scan start, arrival} as the low and
    // high 32 bits of the 100 MHz wall clock, [trace_cap][G]
    uint64_t *trace_wg;
    // optional (KSCHED_XCHG_DUMP=<path>, R > 1): per active batch a and pod m, [R + 1] hashes of the messages the
    // merger received from each rank, then of the one it sent: [(a * B + m) * (R + 1) + r]
    uint64_t *xdbg;
    int64_t xdbg_cap;       // active batches it holds
    int64_t *cdbg;  // KSCHED_COMMIT_STAMPS: commit phase cycle sums (CommitArgs::dbg), else null
    int64_t *mdbg;  // KSCHED_MERGE_STAMPS: merge phase cycle sums (MergeArgs::dbg), else null
    // node-sharded (R > 1, one process per GPU): this rank owns global nodes [node_offset, +n_local);
    // merger m of every rank writes pod m's list into EVERY rank's receive ring (rx_peer[r], slot
    // (active batch % 4, source rank, pod) of xchg_stride bytes) as tagged 8-byte granules (gran_enc),
    // then gathers the R lists of pod m from its own ring and rank-merges them (ksched_pipe.hip merge_role)
    int64_t node_offset;
    int32_t R, rank;
    uint32_t epoch0;        // granule tag of this call's active batch a is epoch0 + a (a >= 1)
    int64_t xchg_stride;    // bytes per pod message in a ring
    char *rx_peer[8];       // every rank's receive ring, mapped into this process (rx_peer[rank] = own)
    // progress words, kProgWords per workgroup ([G] score, [B] merger, [kCommitWGs] commit): {batch << 8 | phase,
    // hw id << 32 | low word of the last value a wait saw, busy-time sums}; read by the host when a wait timed out
    // (and by the phase trace)
    uint64_t *prog;
    char *rescue;           // this rank's RescueReq + Rec res[B] (null: exhausted lists truncate their batch)
    int32_t poison_lds;     // diagnostics (KSCHED_POISON): bytes of dynamic LDS every workgroup fills with 0xff first
    uint32_t lds_fill;      // diagnostics (KSCHED_LDS_FILL): the fill pattern (KSCHED_POISON: 0xffffffff)
    int32_t lds_fill_role;  // roles filled: 1 commit, 2 score, 4 merge (KSCHED_LDS_ROLE, default all)
    int32_t lds_fill_lo, lds_fill_hi;  // byte range filled (KSCHED_LDS_LO / KSCHED_LDS_HI)
    uint32_t jitter;        // diagnostics (KSCHED_JITTER): seed of the random delays at the protocol points, 0 = off
    int32_t rescue_max;     // rescues per batch before an exhausted list truncates it (KSCHED_RESCUE_MAX)
    int32_t rescue_cap;     // the rescue bucket's capacity in rescues (KSCHED_RESCUE_CAP, default rescue_max)
    int32_t rescue_low;     // rescues per batch while the bucket is below half full (KSCHED_RESCUE_LOW)
    int32_t rescue_look;    // KSCHED_RESCUE_LOOK (default 0): the commit's look-ahead over the batch's exhausted lists
    int32_t rescue_rate;    // the commit workgroup's rescue bucket refill per batch, quarter rescues (KSCHED_RESCUE_RATE)
    int32_t touch_screen;   // the commit's touched-node screen (KSCHED_NO_TOUCH_SCREEN=1: every key exact)
    // the merger slots' keys of their pod against the entries of export(b - 2), which commit(b) inherits:
    // [4 batches][B] summaries {sum of predicate deltas, best key, best idx | entry << 32, -} then [4][B][64] keys
    char *inh;
    int32_t early_inh;      // the commit loads those keys before its merges' wait when Ctl::inh_done shows them
                            // (KSCHED_NO_EARLY_INH=1: always after the wait)
    int32_t no_seed;        // diagnostics (KSCHED_NO_SEED): the seeded scan's bound from all rows in every batch
    int32_t no_fold_mask;   // diagnostics (KSCHED_NO_FOLD_MASK): the screened commit folds every wave and column
};
constexpr size_t inh_bytes(int B) { return (size_t)4 * B * 32 + (size_t)4 * B * 64 * 8; }
// progress phases (PersistArgs::prog); kProgWords 8-byte words per workgroup
constexpr int kProgWords = 6;  // 0 phase, 1 where/seen, 2 heartbeat, 3 busy, 4 rows scored exactly, 5 rows scanned
// Behind the progress words of every workgroup: the seeded scan's counters, two words per score workgroup, written by
// the screened KC <= 4 kernels only (the layout the other kernels and the host's per-call path see is unchanged) --
// 0: scans seeded from a mask | seeded from all rows after an unscreened batch << 21 | ... because the mask passed
// the cap << 42; 1: seed rows | scans whose bound was 0 ("everything passes") for some active pod << 40
constexpr int kSeedWords = 2;
__host__ __device__ inline size_t prog_seed_off(int G, int B, int commit_wgs) { return (size_t)(G + B + commit_wgs) * kProgWords; }
enum : int { kProgWaitCommit = 1, kProgScan = 2, kProgArrived = 3, kProgWaitArrive = 4, kProgMerged = 5,
             kProgWaitMerged = 6, kProgCommitted = 7, kProgIdle = 8, kProgRescue = 9, kProgWaitRescue = 10,
             kProgTimedOut = 0x80 };
__device__ __forceinline__ uint32_t hw_where() {
    uint32_t xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    // xcc[3:0] | se[15:13] | cu[11:8] of HW_ID
    return (xcc & 0xf) << 8 | ((hw >> 13) & 7) << 4 | ((hw >> 8) & 0xf);
}
__device__ __forceinline__ void prog_at(const PersistArgs &P, int slot, int64_t b, int phase, uint64_t seen) {
    if (!P.prog) return;
    __hip_atomic_store(P.prog + kProgWords * slot, (uint64_t)b << 8 | (uint64_t)phase, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(P.prog + kProgWords * slot + 1, (uint64_t)hw_where() << 32 | (seen & 0xffffffffull),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// busy-time sums of a workgroup (KSCHED_PERSIST_TRACE calls only: P.trace set): word 2 += scan ticks, word 3
// += ticks from its wait's end to its arrival (word 2 is the heartbeat of a long wait otherwise)
__device__ __forceinline__ void prog_add(const PersistArgs &P, int slot, uint64_t scan, uint64_t busy) {
    if (!P.prog || !P.trace) return;
    P.prog[kProgWords * slot + 2] += scan;
    P.prog[kProgWords * slot + 3] += busy;
}
// Atomic read of a control word at the coherence point: an RMW that adds a zero the compiler cannot see
// (an idempotent RMW it would turn back into a plain atomic load, which may be served by a cached line).
__device__ __forceinline__ uint64_t ld_rmw(const void *p) {
    uint64_t zero = 0;
    asm volatile("" : "+v"(zero));
    return __hip_atomic_fetch_add(reinterpret_cast<uint64_t *>(const_cast<void *>(p)), zero, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
}
// Bounded wait for *p >= v (one lane).  Polls are relaxed agent-scope (sc1) loads with s_sleep; every 1024th
// poll reads the counter with an atomic RMW instead (performed at the coherence point, never served from a
// cached line), so a poll can not stay behind the counter for longer than ~1024 sleeps; each such read
// also stores the poll count to *heartbeat (a stuck wait shows whether it still runs).  A wait that only the
// RMW read satisfied is counted in *rmw_hits.  false: timed out (*seen = the last value read).
__device__ __forceinline__ bool poll_ge(const unsigned long long *p, unsigned long long v, int64_t limit,
                                        unsigned long long *rmw_hits, unsigned long long *seen,
                                        uint64_t *heartbeat = nullptr) {
    unsigned long long x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (x >= v) { *seen = x; return true; }
    const uint64_t t0 = wall_clock64();
    for (int it = 1;; ++it) {
        __builtin_amdgcn_s_sleep(1);
        if ((it & 1023) == 0) {
            if (heartbeat) __hip_atomic_store(heartbeat, (uint64_t)it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            x = (unsigned long long)ld_rmw(p);
            if (x >= v) {
                if (rmw_hits) __hip_atomic_fetch_add(rmw_hits, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *seen = x;
                return true;
            }
            if ((int64_t)(wall_clock64() - t0) > limit) { *seen = x; return false; }
        } else {
            x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (x >= v) { *seen = x; return true; }
        }
    }
}
// The exchange's 8-byte granules carry one 32-bit word and the writer's tag in EACH 32-bit half: {tag16 | word
// bits 0..15} low, {tag16 | word bits 16..31} high, tag16 = (tag & 0x7fff) | 0x8000 (never 0: a zeroed ring holds no
// live granule).  A reader accepts the granule only when both halves carry the tag, so a granule read half old and
// half new (an 8-byte access split into two 4-byte ones -- seen on uncached rings) is never
// taken for the new one.  Tags 32768 apart would alias: every call zeroes the message and rescue areas before its
// rank barrier (ksched_xchg.hip rx_zero_regions), within a call a region is rewritten every 4 active batches, and
// consecutive calls' barrier tags never differ by a multiple of 2^15.
__device__ __forceinline__ uint32_t gran_tag(uint32_t tag) { return (tag & 0x7fffu) | 0x8000u; }
__device__ __forceinline__ uint64_t gran_enc(uint32_t word, uint32_t t16) {
    return ((uint64_t)((t16 << 16) | (word >> 16)) << 32) | (uint64_t)((t16 << 16) | (word & 0xffffu));
}
__device__ __forceinline__ bool gran_dec(uint64_t v, uint32_t t16, uint32_t *word) {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    *word = (lo & 0xffffu) | (hi << 16);
    return ((lo >> 16) == t16) & ((hi >> 16) == t16);
}

constexpr int kMaxXchgRanks = 8;
// receive ring: [4 active-batch slots][R source ranks][B pods] messages, then R barrier granules, then the
// rescue area: [2 request parities][R source ranks] one Rec as 14 tagged granules (128 bytes each)
constexpr size_t xchg_stride_bytes(int K) { return ((size_t)msg_words(K) * 8 + 63) / 64 * 64; }
constexpr int kXchgRescueWords = (int)(sizeof(Rec) / 4);  // 14
constexpr size_t kXchgRescueRec = 128;
__host__ __device__ constexpr size_t xchg_rescue_off(int R, int B, size_t stride) { return (size_t)4 * R * B * stride + 64 * (size_t)R; }
constexpr size_t xchg_ring_bytes(int R, int B, int K) {
    return xchg_rescue_off(R, B, xchg_stride_bytes(K)) + 2 * (size_t)R * kXchgRescueRec;
}
// all ranks meet on the device and agree on the minimum of a small value (tag: this call's epoch0)
hipError_t launch_xchg_min(const PersistArgs &a, int32_t mine, int32_t *out, hipStream_t s);
// trace columns: score start (WG 0 past its wait), last arrival, last merge done, commit start, commit end
// trace row: 0-15 stamps (col 13: exact rows), 16 the commit's counters, 17 its rescue waits; with
// KSCHED_COMMIT_STAMPS 18-21 its prologue / guess / evaluate / check cycles, 22-23 prologue marks (lists hashed, all
// waves past), 24 before the wait, 25 entry -> past the wait, 26 the inherited keys loaded early (0: after the wait),
// 27 P1 done, 29 the check step's rescans, 30 the lists hashed; 33-36 the check step's split in cycles (the fold of
// the confirmed columns, the probe of a pod resolved exactly, the commit of that pod, of it the wait for a listed
// record's state; builds with -DKSCHED_COMMIT_SPLIT=1 only).  An earlier check split had columns 26-28 and 30; P1's
// stamps took 26, 27 and 30 since, so the split moved to 33-36; 38-39 (the same builds) the check's t* fold over the
// waves' partial bests and its rescue leg (look-ahead, rescue, re-key).  Free (no writer): 28, 31-32, 40-48.
constexpr int kTraceCols = 54;  // + 37: score WG 0 behind the bound's barrier (every wave's pass 1 / seed pass done);
                                // 49-53: the commit's rounds
// KSCHED_JITTER (race hunting): at one in four (workgroup, batch, site) triples, sleep the wave for up to ~50 us,
// chosen by a hash of the seed -- a protocol that depends on timing then fails often instead of rarely
__device__ __forceinline__ void jitter_at(uint32_t seed, int64_t b, int site) {
    if (!seed) return;
    uint32_t h = seed ^ (uint32_t)((uint64_t)b * 0x9E3779B1u) ^ ((uint32_t)site * 0x85EBCA77u) ^ (blockIdx.x * 0xC2B2AE3Du);
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    if ((h & 3) != 0) return;
    const int n = (int)((h >> 8) & 255);
    for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(8);
}
__device__ __forceinline__ void trace_at(const PersistArgs &P, int64_t b, int col) {
    if (P.trace && b < P.trace_cap) P.trace[b * kTraceCols + col] = wall_clock64();
}
// k_pipe: ONE kernel of kCommitWGs + G + M workgroups x kPipeThreads per rank: first the commit workgroups,
// then G score workgroups, then M merger workgroups (kPipeMergeSlots pods each).
constexpr int kPipeThreads = 768;
constexpr int kPipeWaves = kPipeThreads / 64;
constexpr int kPipeScoreWaves = kPipeWaves;  // a score workgroup scores with all its waves
constexpr int kPipeMergeThreads = 256;       // one pod merge: one thread per score workgroup's list
constexpr int kPipeMergeSlots = kPipeThreads / kPipeMergeThreads;  // pods a merger workgroup merges at once
struct PipeInfo {
    size_t lds;         // dynamic LDS per workgroup (max of the commit's and a score workgroup's layout)
    size_t static_lds;
    int vgprs;
    size_t spill;       // private (scratch) bytes per thread
    int occ;            // workgroups per CU the occupancy query admits at that LDS (1: one per CU)
};
// One launch of k_pipe: the grids of R ranks (R = 1: a single rank) back to back, rank r's workgroups
// [base[r], base[r + 1]).  R > 1 only for ranks of ONE process sharing ONE device (ksched_xchg_join_local):
// their persistent kernels must be resident at once, which one cooperative launch guarantees and separate
// launches do not.
constexpr int kMaxLocalRanks = 8;  // PipeLaunch: 8 x 344-byte PersistArgs = 2.8 KB of kernel arguments
struct PipeLaunch {
    PersistArgs P[kMaxLocalRanks];
    int32_t R;
    int32_t base[kMaxLocalRanks + 1];
};
// launch: 0 = query PipeInfo only (L.P[0]), 1 = cooperative launch (the runtime checks the grid against the
// occupancy query, so every workgroup of every rank in L is resident at once).
// hipErrorNotSupported: no instantiation for (KC, K) -- the caller runs the stream pipeline.
hipError_t pipe_part_price(int KC, int K, bool lab, bool f53, const PipeLaunch &L, int launch, PipeInfo *info,
                           hipStream_t s);
hipError_t pipe_part_res_all(int KC, int K, bool lab, bool f53, const PipeLaunch &L, int launch, PipeInfo *info,
                             hipStream_t s);
hipError_t pipe_part_res_feas(int KC, int K, bool lab, bool f53, const PipeLaunch &L, int launch, PipeInfo *info,
                              hipStream_t s);
inline hipError_t launch_pipe(int KC, int K, int prio, int dom, bool lab, bool f53, const PipeLaunch &a, int launch,
                              PipeInfo *info, hipStream_t s) {
    if (prio == kPrioPrice) return pipe_part_price(KC, K, lab, false, a, launch, info, s);
    if (dom == kDomFeasible) return pipe_part_res_feas(KC, K, lab, f53, a, launch, info, s);
    return pipe_part_res_all(KC, K, lab, f53, a, launch, info, s);
}

// ---- register-only helpers of the score role (k_pipe; here so that the self-test unit can run them alone) ----------
// OR over the wave's lanes (DPP butterfly; every lane ends with the result)
template <int S>
__device__ __forceinline__ uint64_t or_stage(uint64_t v) {
    return v | (((uint64_t)wpartner<S>((uint32_t)(v >> 32)) << 32) | wpartner<S>((uint32_t)v));
}
__device__ __forceinline__ uint64_t wave_or_u64(uint64_t v) {
    v = or_stage<0>(v); v = or_stage<1>(v); v = or_stage<2>(v);
    v = or_stage<3>(v); v = or_stage<4>(v); v = or_stage<5>(v);
    return v;
}

// Pass 1's lower bounds of one step of kSPU rows into the wave's KC slots.  When kSPU is a multiple of KC,
// row u of the step goes to slot u % KC, which keeps the MAXIMUM of its rows (one v_max per pair instead of
// an insertion into a sorted list): the KC slots of a wave, and of the 12 waves, are lower bounds of keys of
// DISTINCT rows, so the KC-th largest of them is at most the KC-th largest key of the workgroup -- a valid
// L, at most slightly weaker than the KC-th largest of all the rows' bounds (tests/diag/screen_sim.py: c4 exact
// rows +4 %).  Otherwise a sorted top-KC insertion.
template <int KC, int SPU>
__device__ __forceinline__ void bound_slots(uint32_t (&t)[KC], const uint32_t (&xs)[SPU]) {
    if constexpr (SPU % KC == 0) {
#pragma unroll
        for (int u = 0; u < SPU; ++u) t[u % KC] = t[u % KC] > xs[u] ? t[u % KC] : xs[u];
    } else {
#pragma unroll
        for (int u = 0; u < SPU; ++u) {
            uint32_t xv = xs[u];
#pragma unroll
            for (int q = 0; q < KC; ++q) {
                const uint32_t hi = t[q] > xv ? t[q] : xv;
                xv = t[q] > xv ? xv : t[q];
                t[q] = hi;
            }
        }
    }
}

// One lower bound into a sorted (descending) top-KC list
template <int KC>
__device__ __forceinline__ void bound_insert(uint32_t (&t)[KC], uint32_t xv) {
#pragma unroll
    for (int q = 0; q < KC; ++q) {
        const uint32_t hi = t[q] > xv ? t[q] : xv;
        xv = t[q] > xv ? xv : t[q];
        t[q] = hi;
    }
}

// descending order of KC values (once per batch, before the cross-wave merge)
template <int KC>
__device__ __forceinline__ void sort_desc_u32(uint32_t (&t)[KC]) {
#pragma unroll
    for (int i = 1; i < KC; ++i) {
#pragma unroll
        for (int j = i; j >= 1; --j) {
            const uint32_t a = t[j - 1], c = t[j];
            t[j - 1] = a > c ? a : c;
            t[j] = a > c ? c : a;
        }
    }
}

// t (sorted descending) <- the KC largest of t and u (both sorted descending): the element-wise max of t
// and reversed u holds them as a bitonic sequence, which half-cleaners sort
template <int KC>
__device__ __forceinline__ void topk_merge_u32(uint32_t (&t)[KC], const uint32_t (&u)[KC]) {
    uint32_t v[KC];
#pragma unroll
    for (int q = 0; q < KC; ++q) v[q] = t[q] > u[KC - 1 - q] ? t[q] : u[KC - 1 - q];
#pragma unroll
    for (int d = KC / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int i = 0; i < KC; ++i) {
            if ((i & d) == 0) {
                const uint32_t a = v[i], b = v[i + d];
                v[i] = a > b ? a : b;
                v[i + d] = a > b ? b : a;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < KC; ++q) t[q] = v[q];
}

}  // namespace ksched
