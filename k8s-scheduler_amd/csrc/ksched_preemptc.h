// ksched_preemptc.h -- ksched_load_bound_constrained / ksched_preempt_constrained: preemption under the extended
// columns and the spread table.  First the host side: the argument checks in include/ksched.h's order, the packing of
// the bound-pod table's two extra columns and of the pods' constraint words -- plain C++ with no device call, so every
// check runs before anything is allocated or staged (and the unit can be compiled on its own:
// tests/diag/preemptc_check_main.cpp).  Then, for a HIP compiler only, the kernels of ksched_preemptc.hip as the host
// sees them: the table's wrapper, the geometry and the launchers.  Dry run: nothing here writes a node row or a table.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"
#include "ksched_ext.h"
#include "ksched_spread.h"

namespace ksched {

// ---- ksched_load_bound_constrained ------------------------------------------------------------------------------------
struct PcBound {
    int64_t nb;
    const int32_t *node_idx;
    const int64_t *cpu, *mem;
    const int32_t *prio;
    int32_t n_ext;
    const int64_t *bound_ext;      // [n_ext][nb]
    const uint64_t *bound_spread;  // [nb], or NULL: zeros
};

// nullptr: valid; otherwise why not (KSCHED_E_INVALID).  ksched_load_bound's cases first (the arrays, the node indices,
// the segment bound), then the extra columns'.  No array is read before nb and n_ext say how long it is.  May throw
// std::bad_alloc.
inline const char *pc_check_bound(const PcBound &b, int64_t n_local) {
    if (b.nb < 0 || b.nb >= 0x7fffffff) return "nb must be in [0, 2^31 - 1)";
    if (b.nb > 0 && (!b.node_idx || !b.cpu || !b.mem || !b.prio)) return "node_idx, cpu, mem and prio must be given";
    if (b.n_ext < 0 || b.n_ext > KSCHED_EXT_MAX) return "n_ext must be in 0..KSCHED_EXT_MAX";
    if (b.n_ext > 0 && !b.bound_ext) return "bound_ext must be given with n_ext > 0";
    if (b.n_ext == 0 && b.bound_ext) return "bound_ext must be NULL with n_ext == 0";
    std::vector<int32_t> seg((size_t)(n_local > 0 ? n_local : 0), 0);
    for (int64_t t = 0; t < b.nb; ++t) {
        if (b.node_idx[t] < 0 || b.node_idx[t] >= n_local) return "node index out of range";
        if (++seg[(size_t)b.node_idx[t]] > KSCHED_BOUND_MAX_PER_NODE) return "more than KSCHED_BOUND_MAX_PER_NODE pods on one node";
    }
    for (int64_t e = 0; e < (int64_t)b.n_ext * b.nb; ++e)
        if (b.bound_ext[e] < 0) return "a negative extended-resource amount";
    return nullptr;
}

// The table's two extra columns, laid out like the others (ksched_preempt.h: BoundTable): entry e holds table pod
// tidx[e]'s amounts and mask, padding (tidx -1) amount 0 and mask 0.  ext: [n_ext][entries]; *mask_or: every mask ORed.
inline void pc_pack_columns(const std::vector<int32_t> &tidx, const PcBound &b, std::vector<int64_t> *ext,
                            std::vector<uint64_t> *mask, uint64_t *mask_or) {
    const size_t entries = tidx.size();
    ext->assign((size_t)b.n_ext * entries, 0);
    mask->assign(entries, 0);
    *mask_or = 0;
    for (size_t e = 0; e < entries; ++e) {
        const int32_t t = tidx[e];
        if (t < 0) continue;
        for (int32_t r = 0; r < b.n_ext; ++r) (*ext)[(size_t)r * entries + e] = b.bound_ext[(int64_t)r * b.nb + t];
        if (b.bound_spread) { (*mask)[e] = b.bound_spread[t]; *mask_or |= b.bound_spread[t]; }
    }
}

// ---- ksched_preempt_constrained ---------------------------------------------------------------------------------------
struct PcCall {
    int64_t m;
    const int64_t *rc, *rm, *rp;
    const uint64_t *sel;
    const int32_t *prio;
    const int32_t *spread_group;
    const uint8_t *spread_enforce;
    const int64_t *req_ext;
    int32_t vcap;
};

// What the context holds when the call arrives (0 / false: none).
struct PcState {
    bool nodes_loaded, use_labels;
    int32_t nranks;
    bool bound_valid;
    int32_t bound_R;          // the bound table's n_ext
    uint64_t bound_mask_or;   // every mask of the bound table ORed
    int32_t spread_S, ext_R;  // the loaded tables' sizes
};

struct PcPacked {
    bool spread = false, ext = false;  // the tables the kernels are given
    std::vector<int64_t> er;           // [m][KSCHED_EXT_MAX] requests, pod-major (columns from n_ext on: 0)
    std::vector<int32_t> sg;           // [m] the spread group the pod ENFORCES, -1: none (a pod that only counts reads no count)
};

// KSCHED_OK with *out packed, or the code and *why.  Every KSCHED_E_INVALID case that can be decided comes before every
// KSCHED_E_STATE case: ksched_preempt's argument rules, m's range, the rank count, then the pod arrays of each constraint
// that is on -- against its table where one is loaded (without one there is no array length or group count to check
// against: that call ends in KSCHED_E_STATE below).  May throw std::bad_alloc.
inline int pc_check_pack(const PcCall &a, const PcState &st, PcPacked *out, const char **why) {
    *why = nullptr;
    if (a.vcap < 1 || a.vcap > KSCHED_BOUND_MAX_PER_NODE) { *why = "vcap must be in 1..KSCHED_BOUND_MAX_PER_NODE"; return KSCHED_E_INVALID; }
    if (a.m < 0 || a.m >= ((int64_t)1 << 30)) { *why = "m must be in [0, 2^30)"; return KSCHED_E_INVALID; }
    if (a.m > 0 && (!a.rc || !a.rm || !a.rp || !a.prio)) { *why = "the requests and priorities must be given"; return KSCHED_E_INVALID; }
    if (st.use_labels && a.m > 0 && !a.sel) { *why = "use_labels needs selectors"; return KSCHED_E_INVALID; }
    if (st.nranks > 1) { *why = "single-GPU (the tables are: there is no shard merge)"; return KSCHED_E_INVALID; }
    out->spread = a.spread_group != nullptr;
    out->ext = a.req_ext != nullptr;
    std::vector<int32_t> swords, ewords;
    if (out->spread) {
        if (st.spread_S > 0) *why = spread_pack_words(a.m, st.spread_S, a.spread_group, a.spread_enforce, &swords);
        else
            for (int64_t i = 0; i < a.m && !*why; ++i)
                if (a.spread_group[i] < -1) *why = "a spread group outside [-1, n_groups)";
    }
    if (!*why && out->ext && st.ext_R > 0) *why = ext_pack_pods(a.m, st.ext_R, a.req_ext, &out->er, &ewords);
    if (*why) return KSCHED_E_INVALID;
    if (!st.nodes_loaded) { *why = "before load_nodes"; return KSCHED_E_STATE; }
    if (!st.bound_valid) { *why = "no bound-pod table (ksched_load_bound or ksched_load_bound_constrained after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->spread && st.spread_S == 0) { *why = "no spread table (ksched_load_spread after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->ext && st.ext_R == 0) { *why = "no extended-resource table (ksched_load_ext after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->ext && st.bound_R != st.ext_R) { *why = "the bound-pod table's n_ext is not the extended-resource table's"; return KSCHED_E_STATE; }
    if (out->spread && st.spread_S < 64 && (st.bound_mask_or >> st.spread_S) != 0) { *why = "a bound pod's mask names a group the spread table does not hold"; return KSCHED_E_STATE; }
    if (!out->ext) out->er.assign((size_t)a.m * KSCHED_EXT_MAX, 0);
    out->sg.assign((size_t)a.m, -1);
    if (out->spread)
        for (int64_t i = 0; i < a.m; ++i)
            if (swords[(size_t)i] >= 0 && (swords[(size_t)i] & 1)) out->sg[(size_t)i] = swords[(size_t)i] >> 1;
    return KSCHED_OK;
}

}  // namespace ksched

#ifdef __HIPCC__
#include "ksched_preempt.h"

namespace ksched {

// Pods a scan wave carries.  Beside k_preempt_scan's 13 registers a pod keeps two per extended column in use and two
// for the spread clause (DESIGN.md section 4.6.1 has the compiler's resource report for every instantiation).
constexpr int kPreemptCTile = 4;
constexpr int kPreemptCMinWords = 4;  // per spread group: {minimum, second minimum, domains at the minimum, 0}

// ksched_preempt's arguments (a: the bound-pod table, the chunk's pods, the workspace and the outputs, exactly as
// k_preempt_scan reads them) and what the constraints add.  A column or table that the call does not use is never read.
struct PreemptCArgs {
    PreemptArgs a;
    // the bound-pod table's extra columns, entry for entry beside a.tb's (slot-major; padding: amount 0, mask 0)
    const int64_t *bext;    // [n_ext][entries]
    int64_t entries;
    const uint64_t *bmask;  // [entries] bit s: the pod is counted in group s
    // the pods' constraint words (device)
    const int64_t *er;      // [m][KSCHED_EXT_MAX]
    const int32_t *sg;      // [m] enforced group, -1: none
    // the tables as they stand, read only
    const int64_t *ext;     // [n_ext][n_local]
    int32_t n_ext;          // 0: extended resources off
    const int32_t *sp_dom, *sp_cnt, *sp_skew;  // node -> domain, [S][D] counts, [S] skews; sp_dom null: spread off
    int32_t sp_D, sp_S;
    int32_t *sp_min;        // [S][kPreemptCMinWords]: written by k_preemptc_min, then read
};

// preempt_geometry (ksched_preempt.h) at this unit's tile: spans * m <= kPreemptGridWGs * kPreemptCTile.
inline void preemptc_geometry(int64_t n, int64_t m, int32_t *spans, int64_t *span_rows) {
    preempt_geometry(n, m, spans, span_rows, kPreemptCTile);
}

// every group's minimum, second minimum and domains at the minimum into sp_min (nothing where spread is off): one small
// launch from the counts as they stand, no copy to the host
hipError_t launch_preemptc_min(const PreemptCArgs &a, hipStream_t s);
// k_preemptc_scan then k_preemptc_pick on s: two ordinary launches, no waits on the device (sp_min is ready in stream order)
hipError_t launch_preemptc(bool lab, const PreemptCArgs &a, hipStream_t s);

}  // namespace ksched
#endif  // __HIPCC__
