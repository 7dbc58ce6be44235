// ksched_full.h -- host side of the constrained schedule calls (ksched_schedule_gangs / _spread / _ext / _constrained /
// _affinity / _full / _full_why): for a kind of k_exact (exact_kind, ksched_exact.h), which constraints the call
// switches on, the order of its checks and the per-pod packing, through the constraints' own checkers and packers
// (ksched_gang.h, ksched_spread.h, ksched_ext.h, ksched_affinity.h).  Plain C++ with no device call, so every check
// runs before anything is allocated or staged (and the unit can be compiled on its own:
// tests/diag/full_check_main.cpp, kind_check_main.cpp).  The rules are include/ksched.h's.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"
#include "ksched_affinity.h"
#include "ksched_exact.h"
#include "ksched_ext.h"
#include "ksched_gang.h"
#include "ksched_spread.h"

namespace ksched {

// The call's arguments behind the pods' requests, as include/ksched.h names them (a single call leaves the others null).
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

// What the call stages: for every constraint its kind carries, a word per pod, on or off (off: gangs of one, no group,
// no request, no affinity word), and the requests and affinity words where the constraint is on.  Nothing for a
// constraint the kind does not carry.
struct FullPacked {
    bool spread = false, ext = false, aff = false;  // the tables the kernel is given
    size_t n_gangs = 0;                             // the kernel's gangs: the caller's, or one per pod
    std::vector<int32_t> gend, swords, ewords, awords;
    std::vector<int64_t> reqs;
    std::vector<uint64_t> apods;
};

// KSCHED_OK with *out packed, or the code and *why.  A single kind's constraint is on whatever its pointers are; an
// optional kind's where its argument is given.  The order: for an optional kind p and the gang arguments' shape
// (KSCHED_E_INVALID; a single kind's checker refuses its own p); a constraint that is on without its table
// (KSCHED_E_STATE; spread_S, ext_R: the loaded tables' sizes, 0: none); then every array, constraint by constraint
// (KSCHED_E_INVALID).  No array is read before p is known to be in range.  May throw std::bad_alloc.
inline int full_check_pack(ExactKind k, const FullArgs &a, int32_t spread_S, int32_t ext_R, bool aff_valid,
                           FullPacked *out, const char **why) {
    *why = nullptr;
    if (k.optional) {
        if (a.p < 0 || a.p >= ((int64_t)1 << 30)) { *why = "p must be in [0, 2^30)"; return KSCHED_E_INVALID; }
        if (!a.gang_off && a.n_gangs != 0) { *why = "n_gangs must be 0 without gang_off"; return KSCHED_E_INVALID; }
    }
    const bool gangs = k.gang && (!k.optional || a.gang_off);
    out->spread = k.spread && (!k.optional || a.spread_group);
    out->ext = k.ext && (!k.optional || a.req_ext);
    out->aff = k.aff && (!k.optional || affinity_on(a.member, a.anti_host, a.anti_zone, a.aff_group, a.aff_zone));
    if (out->spread && spread_S == 0) { *why = "no spread table (ksched_load_spread after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->ext && ext_R == 0) { *why = "no extended-resource table (ksched_load_ext after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (out->aff && !aff_valid) { *why = "no affinity table (ksched_load_affinity after every ksched_load_nodes)"; return KSCHED_E_STATE; }
    if (gangs) *why = gang_check(a.p, a.n_gangs, a.gang_off, a.gang_min);
    if (!*why && out->spread) *why = spread_pack_words(a.p, spread_S, a.spread_group, a.spread_enforce, &out->swords);
    if (!*why && out->ext) *why = ext_pack_pods(a.p, ext_R, a.req_ext, &out->reqs, &out->ewords);
    if (!*why && out->aff)
        *why = aff_pack_pods(a.p, a.member, a.anti_host, a.anti_zone, a.aff_group, a.aff_zone, &out->awords, &out->apods);
    if (*why) return KSCHED_E_INVALID;
    if (gangs) gang_pack_ends(a.p, a.n_gangs, a.gang_off, a.gang_min, &out->gend);
    else if (k.gang) gang_pack_singles(a.p, &out->gend);
    if (k.spread && !out->spread) out->swords.assign((size_t)a.p, -1);
    if (k.ext && !out->ext) { out->ewords.assign((size_t)a.p, 0); out->reqs.clear(); }
    if (k.aff && !out->aff) { out->awords.assign((size_t)a.p, 0); out->apods.clear(); }
    if (k.gang) out->n_gangs = gangs ? (size_t)a.n_gangs : (size_t)a.p;
    return KSCHED_OK;
}

}  // namespace ksched
