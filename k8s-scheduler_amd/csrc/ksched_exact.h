// ksched_exact.h -- exact mode (ksched_exact.hip).  First, in plain C++ (ksched_full.h reads it without a HIP compiler):
// the kinds of k_exact, what each carries, and the constants of the constraints.  Then, for a HIP compiler only, the
// arguments of k_exact / k_exact1 and the launchers.  ksched_ctx.h includes it beside ksched_kernels.h, so the host units
// keep one include and no other device unit depends on it.
#pragma once

#include <stdint.h>

namespace ksched {

// Which kind of k_exact a launch runs.  The value travels from the C entry point (ksched_constraints.hip) through
// run_impl and enqueue_exact to the kernel's template parameter; every kind but kRunPlain is the multi-slot kernel
// whatever opts.mode, under the geometry and launch rule of a plain exact run.  No other pairing is instantiated
// (a composed kind with a constraint switched off costs 7 to 14 % over the kind without it).
enum ExactRun { kRunPlain = 0, kRunGang = 1, kRunSpread = 2, kRunExt = 3, kRunAll = 4, kRunAffinity = 5, kRunFull = 6,
                kRunFullWhy = 7 };

// What a kind carries: the one table that the kernel's constexpr flags, the launcher's checks, enqueue_exact's fields
// and the host's check-and-pack (ksched_full.h) all read.
//   gang    the staged gang ends, all-or-nothing rollback
//   spread  the staged spread words and the context's spread table
//   ext     the staged requests and words and the context's extended-resource table
//   aff     the staged affinity words and the context's affinity table
//   undo    a rejected gang puts back the affinity words it ORed into (the undo log in d->aundo)
//   why     the reason code of every node for each pod that fits nowhere, at its turn (the why_* buffers)
//   optional  a composed kind: a call switches a constraint it does not use off by uniform run-time values -- gangs of
//             one; sp_S == 0 with every sp_word -1; n_ext == 0 with every ext_word 0; af_dom null with every af_word 0 --
//             and the kernel is not given that table.  A single kind's constraint is always on.
struct ExactKind {
    bool gang, spread, ext, aff, undo, why, optional;
};
constexpr ExactKind exact_kind(ExactRun run) {
    switch (run) {  //                   gang   spread ext    aff    undo   why    optional
        case kRunGang:     return {true,  false, false, false, false, false, false};  // ksched_schedule_gangs
        case kRunSpread:   return {false, true,  false, false, false, false, false};  // ksched_schedule_spread
        case kRunExt:      return {false, false, true,  false, false, false, false};  // ksched_schedule_ext
        case kRunAll:      return {true,  true,  true,  false, false, false, true};   // ksched_schedule_constrained
        case kRunAffinity: return {false, false, false, true,  false, false, false};  // ksched_schedule_affinity
        case kRunFull:     return {true,  true,  true,  true,  true,  false, true};   // ksched_schedule_full
        case kRunFullWhy:  return {true,  true,  true,  true,  true,  true,  true};   // ksched_schedule_full_why
        default:           return {false, false, false, false, false, false, false};  // kRunPlain (ksched_run)
    }
}

constexpr int kNumWhyReasons = 14;      // KSCHED_NUM_REASONS_FULL: ksched_rank_full's codes
constexpr int kGangMax = 1024;          // KSCHED_GANG_MAX: the LDS log of one gang's outcomes
constexpr int32_t kGangRejected = -3;   // KSCHED_GANG_REJECTED
constexpr int kSpreadMaxDomains = 1024; // KSCHED_SPREAD_MAX_DOMAINS
constexpr int kSpreadMaxGroups = 64;    // KSCHED_SPREAD_MAX_GROUPS
constexpr int kSpreadMaxCells = 4096;   // KSCHED_SPREAD_MAX_CELLS: the LDS table of every workgroup, 16 KiB
constexpr int kExtMax = 4;              // KSCHED_EXT_MAX: columns of the dynamic LDS table, kExtMax * 256 * 8 slots * 8 B = 64 KiB

constexpr int kAffMaxGroups = 64;       // KSCHED_AFF_MAX_GROUPS: one bit of a 64-bit word per group
constexpr int kAffWords = 4;            // ExactArgs::af_pod: words per pod

}  // namespace ksched

#ifdef __HIPCC__
#include "ksched_device.h"

namespace ksched {

struct ExactArgs {
    NodeRec *nodes;
    int64_t n;
    int32_t G;        // workgroups (all co-resident)
    int32_t per_wg;   // nodes per workgroup
    PodArgs pods;
    OutArgs out;
    uint64_t *slots;  // [2][G][4] granules {epoch:32 | value:32}; zeroed before every launch
    int32_t *err;     // device error word (kErrExactExchange)
    int64_t timeout_ticks;
    const int32_t *perm;  // k_exact1: slot -> node (best-price: nodes by price asc, index asc); null: slot = node
    // k_exact<GANG> (ksched_schedule_gangs): per pod, 0 or -- at the last member of its gang -- the gang's size
    // (<= kGangMax) | the members it needs << 16 (both fit 15 bits: kGangMax < 2^15, asserted where the host packs
    // them); the kernel reads it with the pod's request
    const int32_t *gang_end;
    int32_t *gang_placed;     // out: members bound per gang, 0 for a rejected one (may be null)
    // k_exact<SPREAD> (ksched_schedule_spread): the context's spread table and the per-pod word
    const int32_t *sp_dom;    // [n] node -> topology domain in [0, sp_D), or -1: the node does not carry the key
    int32_t *sp_counts;       // [sp_S][sp_D] matching pods bound per (group, domain): read at entry, written at exit
    const int32_t *sp_skew;   // [sp_S] the groups' maximum skew
    int32_t sp_D, sp_S;       // sp_S * sp_D <= kSpreadMaxCells (kRunAll: sp_S == 0 -- no table, every sp_word is -1)
    const int32_t *sp_word;   // per pod: -1 (no group), or group << 1 | enforce; the kernel reads it with the request
    // k_exact<EXT> (ksched_schedule_ext): the context's extended-resource table and the staged requests
    int64_t *ext;             // [n_ext][n] allocatable per (resource, node): read at entry, written at exit
    const int64_t *ext_req;   // [p][kExtMax] requests, pod-major (columns at and beyond n_ext: 0)
    const int32_t *ext_word;  // per pod: bit r set where ext_req[i][r] != 0; the kernel reads it with the request
    int32_t n_ext;            // 1..kExtMax (kRunAll: 0 -- no table, every ext_word is 0)
    // k_exact<AFF> (ksched_schedule_affinity): the context's affinity table and the staged pod words
    const int32_t *af_dom;    // [n] node -> zone domain in [0, af_D), or -1: the node does not carry the zone key
    uint64_t *af_member;      // [n] groups with a pod bound on the node: read at entry, written at exit
    uint64_t *af_anti_host;   // [n] groups the node's bound pods refuse at host scope: read at entry, written at exit
    uint64_t *af_anti_zone;   // [n] the same at zone scope: ORed into by the winner's owner lane only
    uint64_t *af_zone;        // [af_D][2] per domain {zone_member, zone_anti}: read at entry, written at exit
    uint64_t *af_any;         // out: [2] {any_host, any_zone} after the call's last pod
    uint64_t af_any_host, af_any_zone;  // the OR of every af_member / of every zone_member before the first pod
    int32_t af_D;             // 0..kSpreadMaxDomains (0: no zone key, every af_dom is -1)
    const int32_t *af_word;   // per pod: 0 (no group, no term), or 1 | zone scope of its affinity term << 1; the kernel
                              // reads it with the request
    const uint64_t *af_pod;   // [p][kAffWords] member, anti_host, anti_zone, the affinity term's group bit (0: none)
    // k_exact<kRunFull> (ksched_schedule_full): every field above (sp_S == 0, n_ext == 0 as in kRunAll; af_dom null --
    // no affinity table, every af_word is 0) and the rejected gang's undo log of the affinity words, device memory that
    // every thread reads back only where it wrote itself
    uint64_t *af_undo_slot;   // [kGangMax][3] per member: its winner's node_member, node_anti_host and (where the member
                              // has an anti_zone word) node_anti_zone before the commit -- the winner's owner lane
    uint64_t *af_undo_zone;   // [G][kGangMax][2] per workgroup and member: {zone_member, zone_anti} of the winner's domain
                              // before the commit -- thread 0 of the workgroup
    // k_exact<kRunFullWhy> (ksched_schedule_full_why): every field above, and what the NO_FIT pods are told.  The r-th
    // NO_FIT pod of the call (in pod order, never rolled back) owns row r of each buffer while r < why_rows (the bytes:
    // r < why_node_rows <= why_rows); the host clears all of them before the launch and reads them after the stream sync
    int32_t *why_pod;         // [why_rows] the pod's index (workgroup 0, thread 0)
    unsigned long long *why_counts;  // [why_rows][kNumWhyReasons] nodes per reason code: every wave adds its own, atomically
    uint8_t *why_reason;      // [why_node_rows][n] every node's code, written by the thread that owns the node's slot
    int64_t why_rows, why_node_rows;
    int64_t *why_nofit;       // out: the call's NO_FIT pods, recorded or not (workgroup 0, thread 0, at exit)
};
constexpr int kExactBlock = 256;
constexpr int kExact1Block = 1024;  // k_exact1: the whole node set in one workgroup

// host-side launchers (ksched_exact.hip).  fast53: every allocatable and request magnitude stays
// below 2^52 for the whole call (host-checked), enabling (double)(a-r) == (double)a - (double)r.
// One launch of k_exact<run>: the fields of every constraint exact_kind(run) carries must be set, a table's "off" form
// accepted only where the kind is optional (hipErrorInvalidValue otherwise).  Dynamic LDS: ext, a.n_ext * block * npt *
// 8 bytes; aff, block * npt * 20 bytes (two 8-byte words and the domain of every slot) where the table is given; the
// kinds with both may pass 64 KiB, so the launcher raises the kernel's limit first.  (A constrained kind never runs
// k_exact1: the one-workgroup kernel knows no gang log and no spread, extended-resource or affinity table.)
hipError_t launch_exact(ExactRun run, int npt, int prio, int dom, bool lab, bool fast53, const ExactArgs &a, int block,
                        bool cooperative, hipStream_t s);
// exact mode on one workgroup of bs threads, npt node slots each: bs 1024 with npt 1-4 (resource) or 1-6, 8, 12, 16
// (best-price); best-price also (512, 10) and (256, 20)
hipError_t launch_exact1(int npt, int bs, int prio, int dom, bool lab, bool f53, const ExactArgs &a, hipStream_t s);

}  // namespace ksched
#endif  // __HIPCC__
