// ksched_dryrun.h -- ksched_rank_full / ksched_explain_full: the dry runs under the spread, extended-resource and
// affinity tables.  First the host side: which constraints a call switches on, the order of its checks and the per-pod
// packing, through the single calls' own checkers (ksched_spread.h, ksched_ext.h, ksched_affinity.h) -- plain C++ with
// no device call, so every check runs before anything is allocated or staged (and the unit can be compiled on its own:
// tests/diag/dryrun_check_main.cpp).  Then, for a HIP compiler only, the kernels of ksched_dryrun.hip as the
// host sees them: the geometry, the workspace layout and the launchers.  The rules are include/ksched.h's.  Dry run:
// nothing here writes a node row or a table.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"
#include "ksched_affinity.h"
#include "ksched_ext.h"
#include "ksched_spread.h"

namespace ksched {

// One pod as the kernels read it, wave-uniform (pod-major: a pod's 112 bytes come with a few scalar loads).
struct alignas(16) DryPod {
    int64_t rc, rm, rp;
    uint64_t sel;
    uint64_t mem, anti_h, anti_z;  // the pod's groups; the groups its anti-affinity terms name, per scope
    uint64_t abit;                 // its affinity term's group bit; 0: no term, or the term is waived
    int64_t er[KSCHED_EXT_MAX];    // its extended-resource requests (0: not checked; columns from n_ext on are 0)
    int32_t sgroup;                // the spread group it ENFORCES, -1: none (a pod that only counts reads no count)
    int32_t flags;                 // kDryAffZone | kDryAff
    int32_t pad[2];
};
static_assert(sizeof(DryPod) == 112, "DryPod layout");
constexpr int32_t kDryAffZone = 1;  // the affinity term is of zone scope
constexpr int32_t kDryAff = 2;      // some affinity word of the pod is not zero: the node and zone words are read

// The call's arguments behind k and the outputs, as include/ksched.h names them (ksched_explain_full: m == 1, every
// given array one element long).
struct DryCall {
    int64_t m;
    const int64_t *rc, *rm, *rp;
    const uint64_t *sel;
    const int32_t *spread_group;
    const uint8_t *spread_enforce;
    const int64_t *req_ext;
    const uint64_t *member, *anti_host, *anti_zone;
    const int32_t *aff_group;
    const uint8_t *aff_zone;
};

// What the context holds when the call arrives: the loaded tables' sizes (0 / false: none) and the affinity table's
// current any words, which decide every pod's waiver.
struct DryState {
    bool use_labels;
    int32_t spread_S, ext_R;
    bool aff_valid;
    uint64_t any_host, any_zone;
};

struct DryPacked {
    bool spread = false, ext = false, aff = false;  // the tables the kernels are given
    std::vector<DryPod> pods;
};

// KSCHED_OK with *out packed, or the code and *why.  The order is ksched_schedule_full's: m and the requests' shape
// (KSCHED_E_INVALID), a constraint that is on without its table (KSCHED_E_STATE), then every array, constraint by
// constraint (KSCHED_E_INVALID).  No array is read before m is known to be in range.  May throw std::bad_alloc.
inline int dry_check_pack(const DryCall &a, const DryState &st, DryPacked *out, const char **why) {
    *why = nullptr;
    if (a.m < 0 || a.m >= ((int64_t)1 << 30)) { *why = "m must be in [0, 2^30)"; return KSCHED_E_INVALID; }
    if (a.m > 0 && (!a.rc || !a.rm || !a.rp)) { *why = "the requests must be given"; return KSCHED_E_INVALID; }
    if (st.use_labels && a.m > 0 && !a.sel) { *why = "use_labels needs selectors"; return KSCHED_E_INVALID; }
    out->spread = a.spread_group != nullptr;
    out->ext = a.req_ext != nullptr;
    out->aff = affinity_on(a.member, a.anti_host, a.anti_zone, a.aff_group, a.aff_zone);
    if (out->spread && st.spread_S == 0) { *why = "no spread table (ksched_load_spread after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->ext && st.ext_R == 0) { *why = "no extended-resource table (ksched_load_ext after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->aff && !st.aff_valid) { *why = "no affinity table (ksched_load_affinity after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    std::vector<int32_t> swords, ewords, awords;
    std::vector<int64_t> reqs;
    std::vector<uint64_t> apods;
    if (out->spread) *why = spread_pack_words(a.m, st.spread_S, a.spread_group, a.spread_enforce, &swords);
    if (!*why && out->ext) *why = ext_pack_pods(a.m, st.ext_R, a.req_ext, &reqs, &ewords);
    if (!*why && out->aff)
        *why = aff_pack_pods(a.m, a.member, a.anti_host, a.anti_zone, a.aff_group, a.aff_zone, &awords, &apods);
    if (*why) return KSCHED_E_INVALID;
    out->pods.assign((size_t)a.m, DryPod{});
    for (int64_t i = 0; i < a.m; ++i) {
        DryPod &p = out->pods[(size_t)i];
        p.rc = a.rc[i]; p.rm = a.rm[i]; p.rp = a.rp[i];
        p.sel = a.sel ? a.sel[i] : 0;
        p.sgroup = -1;
        if (out->spread && swords[(size_t)i] >= 0 && (swords[(size_t)i] & 1)) p.sgroup = swords[(size_t)i] >> 1;
        if (out->ext)
            for (int r = 0; r < KSCHED_EXT_MAX; ++r) p.er[r] = reqs[(size_t)i * KSCHED_EXT_MAX + (size_t)r];
        if (out->aff && awords[(size_t)i] != 0) {
            const uint64_t *w = apods.data() + (size_t)i * kAffPodWords;
            p.mem = w[0]; p.anti_h = w[1]; p.anti_z = w[2]; p.abit = w[3];
            const bool zone = (awords[(size_t)i] & 2) != 0;
            p.flags = kDryAff | (zone ? kDryAffZone : 0);
            // waived: no pod of the group is bound anywhere in scope and the pod is in the group itself
            if ((p.abit & (zone ? st.any_zone : st.any_host)) == 0 && (p.abit & p.mem) != 0) p.abit = 0;
        }
    }
    return KSCHED_OK;
}

// ksched_explain_full's scalars as a call of one pod.  A constraint is on where the pod uses it: spread_group >= 0,
// req_ext given, an affinity word or an affinity group.  The scalars' own range errors come first.
struct DryOne {
    int64_t rc, rm, rp;
    uint64_t sel, member, anti_host, anti_zone;
    int32_t spread_group, aff_group;
    uint8_t spread_enforce, aff_zone;
    DryCall call(const int64_t *req_ext) const {
        const bool sp = spread_group >= 0;
        const bool af = member != 0 || anti_host != 0 || anti_zone != 0 || aff_group >= 0;
        return DryCall{1, &rc, &rm, &rp, &sel, sp ? &spread_group : nullptr, sp ? &spread_enforce : nullptr, req_ext,
                       af ? &member : nullptr, af ? &anti_host : nullptr, af ? &anti_zone : nullptr,
                       af ? &aff_group : nullptr, af ? &aff_zone : nullptr};
    }
};
inline const char *dry_check_one(int32_t spread_group, int32_t aff_group) {
    if (spread_group < -1) return "a spread group outside [-1, n_groups)";
    if (aff_group < -1 || aff_group >= KSCHED_AFF_MAX_GROUPS) return "an affinity group outside [-1, KSCHED_AFF_MAX_GROUPS)";
    return nullptr;
}

}  // namespace ksched

#ifdef __HIPCC__
#include "ksched_rank.h"

namespace ksched {

constexpr int kNumReasonsFull = 14;  // KSCHED_NUM_REASONS_FULL
constexpr int kDryHist = 16;         // histogram fields kept per list: the 14 codes and two that stay zero
// The scan's workgroup, spans, chunks and list steps are ksched_rank.h's (kRankWaves, kRankThreads, kRankSpanMin,
// kRankGridWGs, kRankChunk, kRankInsertMax); the tile is its own.
constexpr int kDryTile = 4;          // pods a scan wave carries (the register report)
constexpr int kDryExplainThreads = 1024;  // k_dry_explain's workgroup: its waves' counts meet in LDS
constexpr int kDryFlush = 255;       // steps a lane's 8-bit histogram fields hold before they are widened and reduced

// The tables as they stand, read only.  A null sp_dom / ext / af_dom: that constraint is off, nothing of it is read.
struct DryTables {
    const int32_t *sp_dom, *sp_cnt, *sp_skew;  // node -> domain, [S][D] counts, [S] skews
    int32_t sp_D, sp_S;
    int32_t *sp_min;                           // [S] each group's minimum count: written by k_dry_min, then read
    const int64_t *ext;                        // [n_ext][n_local]
    int32_t n_ext;
    const int32_t *af_dom;                     // node -> zone domain
    const uint64_t *af_mem, *af_anti_h;        // node_member, node_anti_host
    const uint64_t *af_zone;                   // [af_D][2] {zone_member, zone_anti}
    int32_t af_D;
};

struct DryArgs {
    const NodeRec *nodes;  // read only
    int64_t n_local, node_offset;
    DryTables t;
    const DryPod *pods;    // the chunk's pods (device)
    int32_t m;             // pods in the chunk (<= kRankChunk)
    int32_t spans;         // node spans (scan grid x)
    int64_t span_rows;     // rows per span, a multiple of kRankThreads
    Cand *part;            // [m][spans][64], best first, idx = kNoIdx past the end
    int32_t *part_hist;    // [m][spans][kDryHist] nodes of the span per reason code
    int32_t k;             // entries wanted (1..64)
    int32_t *out_idx;      // [m][k]
    double *out_score;     // [m][k]
    uint8_t *out_reason;   // [m][k]
    int32_t *out_count;    // [m]
    int32_t *out_feasible; // [m]
    int64_t *out_hist;     // [m][kNumReasonsFull]
};

// rank_geometry (ksched_rank.h) at this unit's tile: spans * m <= kRankGridWGs * kDryTile lists of 1 KiB.
inline void dry_geometry(int64_t n, int64_t m, int32_t *spans, int64_t *span_rows) {
    rank_geometry(n, m, spans, span_rows, kDryTile);
}

// every group's minimum count into t.sp_min (nothing where spread is off): one small launch, no copy to the host
hipError_t launch_dry_min(const DryTables &t, hipStream_t s);
// k_dry_scan then k_dry_merge on s: two ordinary launches, no waits on the device (t.sp_min is ready in stream order)
hipError_t launch_dry_rank(int prio, int dom, bool lab, bool fast53, const DryArgs &a, hipStream_t s);
// one pod against every row: reason[j] (may be null) and counts[kNumReasonsFull] (zeroed by the caller)
hipError_t launch_dry_explain(const NodeRec *nodes, int64_t n, const DryTables &t, const DryPod &pod, bool use_labels,
                              uint8_t *reason, unsigned long long *counts, hipStream_t s);

}  // namespace ksched
#endif  // __HIPCC__
