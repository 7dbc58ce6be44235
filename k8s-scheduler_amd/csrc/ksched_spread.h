// ksched_spread.h -- host side of ksched_load_spread / ksched_schedule_spread: the argument checks and the per-pod
// word, plain C++ with no device call, so every check runs before anything is allocated or staged (and the unit can
// be compiled on its own).  The rules are include/ksched.h's.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"

namespace ksched {

// The table's arguments.  nullptr: valid; otherwise why not (KSCHED_E_INVALID).
inline const char *spread_check_table(int64_t n_local, int32_t n_domains, const int32_t *node_domain, int32_t n_groups,
                                      const int32_t *max_skew, const int32_t *counts) {
    if (n_domains < 1 || n_domains > KSCHED_SPREAD_MAX_DOMAINS) return "n_domains must be in 1..KSCHED_SPREAD_MAX_DOMAINS";
    if (n_groups < 1 || n_groups > KSCHED_SPREAD_MAX_GROUPS) return "n_groups must be in 1..KSCHED_SPREAD_MAX_GROUPS";
    if ((int64_t)n_domains * n_groups > KSCHED_SPREAD_MAX_CELLS) return "n_groups * n_domains exceeds KSCHED_SPREAD_MAX_CELLS";
    if (!max_skew || (n_local > 0 && !node_domain)) return "node_domain and max_skew must be given";
    std::vector<uint8_t> carried((size_t)n_domains, 0);
    for (int64_t j = 0; j < n_local; ++j) {
        if (node_domain[j] < -1 || node_domain[j] >= n_domains) return "a node domain outside [-1, n_domains)";
        if (node_domain[j] >= 0) carried[(size_t)node_domain[j]] = 1;
    }
    for (int32_t d = 0; d < n_domains; ++d)
        if (!carried[(size_t)d]) return "a domain that no node carries (compact the domain ids)";
    for (int32_t s = 0; s < n_groups; ++s)
        if (max_skew[s] < 1) return "max_skew must be at least 1";
    if (counts)
        for (int64_t e = 0; e < (int64_t)n_groups * n_domains; ++e)
            if (counts[e] < 0 || counts[e] > (1 << 30)) return "a count outside [0, 2^30]";
    return nullptr;
}

// The pods' arguments, and ExactArgs::sp_word for each pod: -1 (no group), or group << 1 | enforce.
inline const char *spread_pack_words(int64_t p, int32_t n_groups, const int32_t *spread_group, const uint8_t *spread_enforce,
                                     std::vector<int32_t> *words) {
    if (p < 0 || p >= ((int64_t)1 << 30)) return "p must be in [0, 2^30)";
    if (p > 0 && !spread_group) return "spread_group must be given";
    for (int64_t i = 0; i < p; ++i)
        if (spread_group[i] < -1 || spread_group[i] >= n_groups) return "a spread group outside [-1, n_groups)";
    words->resize((size_t)p);
    for (int64_t i = 0; i < p; ++i) {
        const int32_t s = spread_group[i];
        (*words)[(size_t)i] = s < 0 ? -1 : (s << 1 | ((spread_enforce ? spread_enforce[i] != 0 : true) ? 1 : 0));
    }
    return nullptr;
}

}  // namespace ksched
