// ksched_why.h -- host side of ksched_schedule_full_why beside ksched_full.h: the checks of the arguments the call adds
// to ksched_schedule_full's (they run after full_check_pack, in include/ksched.h's order) and the layout of the one
// device buffer its rows live in.  Plain C++ with no device call, so every check runs before anything is allocated or
// staged (and the unit can be compiled on its own: tests/diag/why_check_main.cpp).  The rules are include/ksched.h's.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ksched.h"

namespace ksched {

// The arguments behind out_gang_placed, as include/ksched.h names them, and the context's node count.
struct WhyArgs {
    int64_t why_rows;
    const int32_t *out_why_pod;
    const int64_t *out_why_counts;
    int64_t node_rows;
    const uint8_t *out_why_reason;
    int64_t n_local;
};

// nullptr, or why the call is KSCHED_E_INVALID.  No pointer is dereferenced.
inline const char *why_check(const WhyArgs &a) {
    if (a.why_rows < 0 || a.node_rows < 0) return "why_rows and node_rows must not be negative";
    if (a.node_rows > a.why_rows) return "node_rows must not exceed why_rows";
    if (a.why_rows >= ((int64_t)1 << 30)) return "why_rows must be below 2^30";
    if (a.why_rows > 0 && (!a.out_why_pod || !a.out_why_counts)) return "out_why_pod and out_why_counts must be given with why_rows > 0";
    if (a.node_rows > 0 && !a.out_why_reason) return "out_why_reason must be given with node_rows > 0";
    // (node_rows < 2^30 and n_local < 2^31: the product cannot wrap)
    if (a.node_rows > 0 && a.n_local > 0 && a.node_rows * a.n_local > (int64_t)KSCHED_WHY_MAX_NODE_BYTES)
        return "node_rows * n_local above KSCHED_WHY_MAX_NODE_BYTES";
    return nullptr;
}

// The device buffer: the counts first (8-byte words), the total behind them, then the pods, then the bytes.
// why_rows * (4 + 8 * KSCHED_NUM_REASONS_FULL) bytes and the node bytes, beside one word and the alignment.
struct WhyLayout {
    size_t o_counts, o_nofit, o_pod, o_reason, total;
};
inline WhyLayout why_layout(int64_t why_rows, int64_t node_rows, int64_t n_local) {
    WhyLayout l;
    l.o_counts = 0;
    l.o_nofit = (size_t)why_rows * KSCHED_NUM_REASONS_FULL * sizeof(int64_t);
    l.o_pod = l.o_nofit + sizeof(int64_t);
    l.o_reason = l.o_pod + ((size_t)why_rows * sizeof(int32_t) + 7) / 8 * 8;
    l.total = l.o_reason + (size_t)node_rows * (size_t)(n_local > 0 ? n_local : 0);
    return l;
}

}  // namespace ksched
