// ksched_ext.h -- host side of ksched_load_ext / ksched_schedule_ext: the argument checks and the per-pod staging,
// plain C++ with no device call, so every check runs before anything is allocated or staged (and the unit can be
// compiled on its own).  The rules are include/ksched.h's.
#pragma once

#include <cstdint>
#include <vector>

#include "ksched.h"

namespace ksched {

// The table's arguments.  nullptr: valid; otherwise why not (KSCHED_E_INVALID).
inline const char *ext_check_table(int32_t n_ext, const int64_t *node_ext) {
    if (n_ext < 1 || n_ext > KSCHED_EXT_MAX) return "n_ext must be in 1..KSCHED_EXT_MAX";
    if (!node_ext) return "node_ext must be given";
    return nullptr;
}

// The pods' arguments, and what the kernel reads per pod: reqs[i * KSCHED_EXT_MAX + r], pod-major with a fixed stride
// (columns at and beyond n_ext are zero) so that one uniform load brings every column, and words[i], bit r set where
// the request for column r is not zero.  req_ext == nullptr: every request is zero.
inline const char *ext_pack_pods(int64_t p, int32_t n_ext, const int64_t *req_ext, std::vector<int64_t> *reqs,
                                 std::vector<int32_t> *words) {
    if (n_ext < 1 || n_ext > KSCHED_EXT_MAX) return "n_ext must be in 1..KSCHED_EXT_MAX";
    if (p < 0 || p >= ((int64_t)1 << 30)) return "p must be in [0, 2^30)";
    if (req_ext)
        for (int64_t e = 0; e < (int64_t)n_ext * p; ++e)
            if (req_ext[e] < 0) return "a negative extended-resource request";
    reqs->assign((size_t)p * KSCHED_EXT_MAX, 0);
    words->assign((size_t)p, 0);
    if (req_ext)
        for (int32_t r = 0; r < n_ext; ++r)
            for (int64_t i = 0; i < p; ++i) {
                const int64_t v = req_ext[(int64_t)r * p + i];
                (*reqs)[(size_t)i * KSCHED_EXT_MAX + (size_t)r] = v;
                if (v != 0) (*words)[(size_t)i] |= 1 << r;
            }
    return nullptr;
}

}  // namespace ksched
