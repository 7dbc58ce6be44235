// ksched_reason.h -- the ONE device function that gives the FailedScheduling code of a (pod, node) pair under
// ksched_schedule_full's constraints, and the two values it reads.  Shared by the dry runs (ksched_dryrun.hip: the scan
// ranks by it, the merge labels the ranked entries with it, the explain kernel is nothing else) and by
// k_exact<kRunFullWhy> (ksched_exact.hip: the reasons a pod that fits nowhere saw at its turn), so what a pod is told
// at its turn and what a dry run tells it cannot disagree about a state they both see.  Device units only.
#pragma once

#include <hip/hip_runtime.h>

#include "ksched_dryrun.h"  // KSCHED_EXT_MAX and the reason codes (ksched.h), kDryAff / kDryAffZone

namespace ksched {

// A pod as a wave carries it: DryPod with the spread group resolved against the table.
struct PodU {
    int64_t rc, rm, rp;
    uint64_t sel, mem, anti_h, anti_z, abit;
    int64_t er[KSCHED_EXT_MAX];
    int32_t srow;   // the enforced group's row of the counts, -1: none
    int64_t slim;   // ... the largest count an eligible domain may hold: max_skew + minimum - 1
    int32_t flags;
};

// What a lane holds of its node beside the NodeRec's fields.
struct RowX {
    int32_t sd;                   // spread domain (-1 also where spread is off)
    int64_t ext[KSCHED_EXT_MAX];  // extended columns (0 where not loaded: only non-zero requests read them)
    int32_t ad;                   // affinity zone domain
    uint64_t nm, na;              // node_member, node_anti_host
};

// The first failing check of pod u on a node, in include/ksched.h's order: cpu, memory, pods, labels, the extended
// columns (zero requests skipped), the spread key, the spread skew, the pod's affinity term, its own anti-affinity
// terms, the bound pods' anti-affinity.  0: eligible(i, j) of ksched_schedule_full.  cnt: the [S][D] counts, zone: the
// per-domain {zone_member, zone_anti} pairs -- in LDS (the dry scan, k_exact) or in global memory.
template <bool LAB>
__device__ __forceinline__ int dry_reason(const PodU &u, int64_t a0, int64_t a1, int64_t a2, uint64_t lab,
                                          const RowX &x, const int32_t *cnt, const uint64_t *zone) {
    int c = a0 < u.rc ? 1 : a1 < u.rm ? 2 : a2 < u.rp ? 3 : (LAB && (lab & u.sel) != u.sel) ? 4 : 0;
    if (c == 0) {
#pragma unroll
        for (int r = KSCHED_EXT_MAX - 1; r >= 0; --r)  // (downwards: the lowest failing column is the one that stays)
            if (u.er[r] != 0 && u.er[r] > x.ext[r]) c = KSCHED_REASON_EXT0 + r;
    }
    if (c == 0 && u.srow >= 0) {  // (the first clause is per lane, the second wave-uniform)
        if (x.sd < 0) c = KSCHED_REASON_SPREAD_NO_KEY;
        else if ((int64_t)cnt[u.srow + x.sd] > u.slim) c = KSCHED_REASON_SPREAD_SKEW;
    }
    if (c == 0 && (u.flags & kDryAff)) {
        uint64_t zm = 0, za = 0;
        if (x.ad >= 0) { zm = zone[2 * x.ad]; za = zone[2 * x.ad + 1]; }  // a node without the key violates no zone term
        if ((((u.flags & kDryAffZone) ? zm : x.nm) & u.abit) != u.abit) c = KSCHED_REASON_AFFINITY;
        else if (((x.nm & u.anti_h) | (zm & u.anti_z)) != 0) c = KSCHED_REASON_ANTI_AFFINITY;
        else if (((x.na | za) & u.mem) != 0) c = KSCHED_REASON_EXISTING_ANTI_AFFINITY;
    }
    return c;
}

}  // namespace ksched
