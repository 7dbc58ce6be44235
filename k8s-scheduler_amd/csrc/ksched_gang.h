// ksched_gang.h -- host side of ksched_schedule_gangs / ksched_schedule_constrained: the checks of the gang offsets and
// minima and the per-pod word, plain C++ with no device call, so every check runs before anything is allocated or
// staged (and the unit can be compiled on its own).  The rules are include/ksched.h's.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"

namespace ksched {

static_assert(KSCHED_GANG_MAX < (1 << 15), "ExactArgs::gang_end packs size and minimum into 16 bits each");

// The gangs' arguments.  nullptr: valid; otherwise why not (KSCHED_E_INVALID).  Every offset and minimum is checked
// before anything is written or allocated: each offset above its predecessor and at most p (so every gang's pods lie
// in [0, p)), each gang within the cap.
inline const char *gang_check(int64_t p, int64_t n_gangs, const int64_t *gang_off, const int32_t *gang_min) {
    if (p < 0 || n_gangs < 0 || n_gangs > p || !gang_off || gang_off[0] != 0 || gang_off[n_gangs] != p)
        return "gang_off must run from 0 to p over n_gangs <= p gangs";
    for (int64_t g = 0; g < n_gangs; ++g) {
        if (gang_off[g + 1] <= gang_off[g] || gang_off[g + 1] > p) return "gang_off must be strictly increasing and end at p";
        const int64_t size = gang_off[g + 1] - gang_off[g];
        if (size > KSCHED_GANG_MAX) return "a gang has more than KSCHED_GANG_MAX members";
        if (gang_min && (gang_min[g] < 1 || gang_min[g] > size)) return "gang_min must be in 1..size";
    }
    return nullptr;
}

// ExactArgs::gang_end for each pod of gangs that passed gang_check, so the kernel reads a gang's end with its last
// member's request: 0, or size | minimum << 16 (gang_min == nullptr: every member is required).
inline void gang_pack_ends(int64_t p, int64_t n_gangs, const int64_t *gang_off, const int32_t *gang_min,
                           std::vector<int32_t> *gend) {
    gend->assign((size_t)p, 0);
    for (int64_t g = 0; g < n_gangs; ++g) {
        const int32_t size = (int32_t)(gang_off[g + 1] - gang_off[g]);
        (*gend)[(size_t)gang_off[g + 1] - 1] = size | (gang_min ? gang_min[g] : size) << 16;
    }
}

// The same for pods that come in no gangs (ksched_schedule_constrained without gang_off): every pod is a gang of one.
inline void gang_pack_singles(int64_t p, std::vector<int32_t> *gend) { gend->assign((size_t)p, 1 | 1 << 16); }

}  // namespace ksched
