// ksched_affinity.h -- host side of ksched_load_affinity / ksched_schedule_affinity: the table check, the derivation of
// the zone and `any` words, and the per-pod packing, plain C++ with no device call, so every check runs before anything
// is allocated or staged (and the unit can be compiled on its own: tests/diag/affinity_check_main.cpp).  The rules are
// include/ksched.h's.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"

namespace ksched {

// The table's arguments.  nullptr: valid; otherwise why not (KSCHED_E_INVALID).  node_domain may be null only where
// there is nothing to read it for (no zone key, or no node).
inline const char *aff_check_table(int64_t n_local, int32_t n_domains, const int32_t *node_domain) {
    if (n_domains < 0 || n_domains > KSCHED_SPREAD_MAX_DOMAINS) return "n_domains must be in 0..KSCHED_SPREAD_MAX_DOMAINS";
    if (!node_domain) return n_domains > 0 && n_local > 0 ? "node_domain must be given where n_domains > 0" : nullptr;
    std::vector<uint8_t> carried((size_t)n_domains, 0);
    for (int64_t j = 0; j < n_local; ++j) {
        if (node_domain[j] < -1 || node_domain[j] >= n_domains) return "a node domain outside [-1, n_domains)";
        if (node_domain[j] >= 0) carried[(size_t)node_domain[j]] = 1;
    }
    for (int32_t d = 0; d < n_domains; ++d)
        if (!carried[(size_t)d]) return "a domain that no node carries (compact the domain ids)";
    return nullptr;
}

// What the library derives from a checked table: per domain {zone_member, zone_anti} side by side (the layout of
// ExactArgs::af_zone), and the OR of every node_member / of every zone_member.  A null mask array is all zero.
struct AffDerived {
    std::vector<uint64_t> zone;  // [n_domains][2]
    uint64_t any_host = 0, any_zone = 0;
};
inline void aff_derive(int64_t n_local, int32_t n_domains, const int32_t *node_domain, const uint64_t *node_member,
                       const uint64_t *node_anti_zone, AffDerived *out) {
    out->zone.assign((size_t)n_domains * 2, 0);
    out->any_host = out->any_zone = 0;
    for (int64_t j = 0; j < n_local; ++j) {
        const uint64_t m = node_member ? node_member[j] : 0;
        out->any_host |= m;
        const int32_t d = node_domain ? node_domain[j] : -1;
        if (d < 0) continue;  // (the bits of a node without the key act on nothing)
        out->zone[(size_t)d * 2] |= m;
        out->zone[(size_t)d * 2 + 1] |= node_anti_zone ? node_anti_zone[j] : 0;
        out->any_zone |= m;
    }
}

constexpr int kAffPodWords = 4;  // ExactArgs::af_pod: member, anti_host, anti_zone, the affinity term's group bit

// Where affinity is optional (the composed schedule calls, the dry runs) it is on when at least one of its five
// pointers is given.
inline bool affinity_on(const uint64_t *member, const uint64_t *anti_host, const uint64_t *anti_zone,
                        const int32_t *aff_group, const uint8_t *aff_zone) {
    return member || anti_host || anti_zone || aff_group || aff_zone;
}

// The pods' arguments, and for each pod ExactArgs::af_word -- 0 where the pod has no group and no term, else 1 | (its
// affinity term is of zone scope) << 1 -- and its kAffPodWords words of ExactArgs::af_pod.  Any array may be null:
// zeros, or -1 for aff_group.
inline const char *aff_pack_pods(int64_t p, const uint64_t *member, const uint64_t *anti_host, const uint64_t *anti_zone,
                                 const int32_t *aff_group, const uint8_t *aff_zone, std::vector<int32_t> *words,
                                 std::vector<uint64_t> *pods) {
    if (p < 0 || p >= ((int64_t)1 << 30)) return "p must be in [0, 2^30)";
    if (aff_group)
        for (int64_t i = 0; i < p; ++i)
            if (aff_group[i] < -1 || aff_group[i] >= KSCHED_AFF_MAX_GROUPS) return "an affinity group outside [-1, KSCHED_AFF_MAX_GROUPS)";
    words->assign((size_t)p, 0);
    pods->assign((size_t)p * kAffPodWords, 0);
    for (int64_t i = 0; i < p; ++i) {
        uint64_t *w = pods->data() + (size_t)i * kAffPodWords;
        w[0] = member ? member[i] : 0;
        w[1] = anti_host ? anti_host[i] : 0;
        w[2] = anti_zone ? anti_zone[i] : 0;
        const int32_t a = aff_group ? aff_group[i] : -1;
        w[3] = a >= 0 ? (uint64_t)1 << a : 0;
        if ((w[0] | w[1] | w[2] | w[3]) != 0) (*words)[(size_t)i] = 1 | ((a >= 0 && aff_zone && aff_zone[i] != 0) ? 2 : 0);
    }
    return nullptr;
}

}  // namespace ksched
