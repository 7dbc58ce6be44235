// ksched_full.h -- host side of ksched_schedule_full: which constraints the call switches on, the order of its checks
// and the per-pod packing of all four, through the single calls' own checkers and packers (ksched_gang.h,
// ksched_spread.h, ksched_ext.h, ksched_affinity.h).  Plain C++ with no device call, so every check runs before anything
// is allocated or staged (and the unit can be compiled on its own: tests/diag/full_check_main.cpp).  The rules are
// include/ksched.h's.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"
#include "ksched_affinity.h"
#include "ksched_ext.h"
#include "ksched_gang.h"
#include "ksched_spread.h"

namespace ksched {

// The call's arguments behind the pods' requests, as include/ksched.h names them.
struct FullArgs {
    int64_t p, n_gangs;
    const int64_t *gang_off;
    const int32_t *gang_min;
    const int32_t *spread_group;
    const uint8_t *spread_enforce;
    const int64_t *req_ext;
    const uint64_t *member, *anti_host, *anti_zone;
    const int32_t *aff_group;
    const uint8_t *aff_zone;
};

// What the call stages: a word per pod for every constraint, on or off (off: gangs of one, no group, no request, no
// affinity word), and the requests and affinity words where their constraint is on.
struct FullPacked {
    bool spread = false, ext = false, aff = false;  // the tables the kernel is given
    size_t n_gangs = 0;                             // the kernel's gangs: the caller's, or one per pod
    std::vector<int32_t> gend, swords, ewords, awords;
    std::vector<int64_t> reqs;
    std::vector<uint64_t> apods;
};

// Affinity is on when at least one of its five pointers is given.
inline bool full_affinity_on(const FullArgs &a) {
    return a.member || a.anti_host || a.anti_zone || a.aff_group || a.aff_zone;
}

// KSCHED_OK with *out packed, or the code and *why.  The order: p and the gang arguments' shape (KSCHED_E_INVALID), a
// constraint that is on without its table (KSCHED_E_STATE; spread_S, ext_R: the loaded tables' sizes, 0: none), then
// every array, constraint by constraint (KSCHED_E_INVALID).  No array is read before p is known to be in range.  May
// throw std::bad_alloc.
inline int full_check_pack(const FullArgs &a, int32_t spread_S, int32_t ext_R, bool aff_valid, FullPacked *out,
                           const char **why) {
    *why = nullptr;
    if (a.p < 0 || a.p >= ((int64_t)1 << 30)) { *why = "p must be in [0, 2^30)"; return KSCHED_E_INVALID; }
    if (!a.gang_off && a.n_gangs != 0) { *why = "n_gangs must be 0 without gang_off"; return KSCHED_E_INVALID; }
    out->spread = a.spread_group != nullptr;
    out->ext = a.req_ext != nullptr;
    out->aff = full_affinity_on(a);
    if (out->spread && spread_S == 0) { *why = "no spread table (ksched_load_spread after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->ext && ext_R == 0) { *why = "no extended-resource table (ksched_load_ext after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->aff && !aff_valid) { *why = "no affinity table (ksched_load_affinity after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (a.gang_off) *why = gang_check(a.p, a.n_gangs, a.gang_off, a.gang_min);
    if (!*why && out->spread) *why = spread_pack_words(a.p, spread_S, a.spread_group, a.spread_enforce, &out->swords);
    if (!*why && out->ext) *why = ext_pack_pods(a.p, ext_R, a.req_ext, &out->reqs, &out->ewords);
    if (!*why && out->aff)
        *why = aff_pack_pods(a.p, a.member, a.anti_host, a.anti_zone, a.aff_group, a.aff_zone, &out->awords, &out->apods);
    if (*why) return KSCHED_E_INVALID;
    if (a.gang_off) gang_pack_ends(a.p, a.n_gangs, a.gang_off, a.gang_min, &out->gend);
    else gang_pack_singles(a.p, &out->gend);
    if (!out->spread) out->swords.assign((size_t)a.p, -1);
    if (!out->ext) { out->ewords.assign((size_t)a.p, 0); out->reqs.clear(); }
    if (!out->aff) { out->awords.assign((size_t)a.p, 0); out->apods.clear(); }
    out->n_gangs = a.gang_off ? (size_t)a.n_gangs : (size_t)a.p;
    return KSCHED_OK;
}

}  // namespace ksched
