// why_check_main.cpp -- csrc/ksched_why.h beside csrc/ksched_full.h on their own, for a CPU sanitizer run of
// ksched_schedule_full_why's checks: ksched_schedule_full's come first, in that header's order, then the call's own --
// the two caps, the output pointers they require and the bound on the per-node bytes -- and the layout of the rows'
// device buffer (no device call, no library):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ik8s-scheduler_amd/csrc
//       tests/diag/why_check_main.cpp -o why_check; ./why_check
// Every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ksched_full.h"
#include "ksched_why.h"

using namespace ksched;

static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

// a heap copy of exactly the vector's length (ASan's redzones sit right behind it); an empty vector is a null pointer
template <class T>
struct Exact {
    T *p = nullptr;
    explicit Exact(const std::vector<T> &v) {
        if (v.empty()) return;
        p = (T *)std::malloc(v.size() * sizeof(T));
        std::memcpy(p, v.data(), v.size() * sizeof(T));
    }
    ~Exact() { std::free(p); }
};

// One call: ksched_schedule_full's arrays by value (empty: NULL), the loaded tables, and the new arguments; the output
// buffers are allocated at exactly the sizes the arguments promise (a flag leaves one out).
struct Call {
    int64_t p = 0, n_gangs = 0, n_local = 4;
    std::vector<int64_t> gang_off;
    std::vector<int32_t> gang_min, group;
    std::vector<uint8_t> enforce;
    std::vector<int64_t> req;
    std::vector<uint64_t> member;
    std::vector<int32_t> aff_group;
    int32_t S = 2, R = 2;
    bool aff_valid = true;
    int64_t why_rows = 0, node_rows = 0;
    bool no_pod = false, no_counts = false, no_reason = false;
};

static const char *why;

// the code ksched_schedule_full_why returns before it touches the device: full_check_pack, then why_check
static int run(const Call &c) {
    Exact<int64_t> off(c.gang_off), req(c.req);
    Exact<int32_t> gmin(c.gang_min), group(c.group), ag(c.aff_group);
    Exact<uint8_t> enf(c.enforce);
    Exact<uint64_t> mem(c.member);
    const FullArgs a{c.p, c.n_gangs, off.p, gmin.p, group.p, enf.p, req.p, mem.p, nullptr, nullptr, ag.p, nullptr};
    FullPacked k;
    why = nullptr;
    if (const int code = full_check_pack(exact_kind(kRunFullWhy), a, c.S, c.R, c.aff_valid, &k, &why)) return code;
    const bool rows = c.why_rows > 0 && c.why_rows < 4096, nodes = c.node_rows > 0 && c.node_rows < 4096;
    Exact<int32_t> wp(std::vector<int32_t>(rows && !c.no_pod ? (size_t)c.why_rows : 0));
    Exact<int64_t> wc(std::vector<int64_t>(rows && !c.no_counts ? (size_t)c.why_rows * KSCHED_NUM_REASONS_FULL : 0));
    Exact<uint8_t> wr(std::vector<uint8_t>(nodes && !c.no_reason ? (size_t)(c.node_rows * c.n_local) : 0));
    // (beyond 4096 rows no buffer is allocated here: a stand-in address the check must never read through)
    static int32_t far_pod; static int64_t far_counts; static uint8_t far_reason;
    const int32_t *pp = rows ? wp.p : (c.why_rows > 0 && !c.no_pod ? &far_pod : nullptr);
    const int64_t *pc = rows ? wc.p : (c.why_rows > 0 && !c.no_counts ? &far_counts : nullptr);
    const uint8_t *pr = nodes ? wr.p : (c.node_rows > 0 && !c.no_reason ? &far_reason : nullptr);
    why = why_check(WhyArgs{c.why_rows, pp, pc, c.node_rows, pr, c.n_local});
    return why ? KSCHED_E_INVALID : KSCHED_OK;
}

// three pods in two gangs, every constraint on
static Call all_on() {
    Call c;
    c.p = 3; c.n_gangs = 2;
    c.gang_off = {0, 2, 3}; c.gang_min = {2, 1};
    c.group = {0, 1, -1}; c.enforce = {1, 0, 1};
    c.req = {1, 0, 2, 0, 0, 3};
    c.member = {1, 2, 0}; c.aff_group = {0, -1, 63};
    c.why_rows = 3; c.node_rows = 2;
    return c;
}

int main() {
    {   // accepted shapes
        Call c = all_on();
        expect(run(c) == KSCHED_OK, "rows and node rows");
        c.node_rows = 0; c.no_reason = true;
        expect(run(c) == KSCHED_OK, "node_rows 0 with a NULL byte buffer");
        c.why_rows = 0; c.no_pod = c.no_counts = true;
        expect(run(c) == KSCHED_OK, "why_rows 0: only the total is produced, every buffer may be NULL");
        c = all_on(); c.why_rows = 1; c.node_rows = 1;
        expect(run(c) == KSCHED_OK, "fewer rows than pods");
        c = all_on(); c.why_rows = c.node_rows = 7;
        expect(run(c) == KSCHED_OK, "more rows than pods");
        c = all_on(); c.n_local = 0; c.node_rows = 0; c.no_reason = true;
        expect(run(c) == KSCHED_OK, "no nodes");
        Call off;
        off.p = 2; off.S = 0; off.R = 0; off.aff_valid = false; off.why_rows = 2;
        expect(run(off) == KSCHED_OK, "every constraint off, no table loaded");
    }
    {   // the call's own cases
        Call c = all_on(); c.why_rows = -1; c.node_rows = -1;
        expect(run(c) == KSCHED_E_INVALID, "why_rows < 0");
        c = all_on(); c.node_rows = -1;
        expect(run(c) == KSCHED_E_INVALID, "node_rows < 0");
        c = all_on(); c.node_rows = 4;
        expect(run(c) == KSCHED_E_INVALID, "node_rows > why_rows");
        c = all_on(); c.why_rows = (int64_t)1 << 30; c.node_rows = 0;
        expect(run(c) == KSCHED_E_INVALID, "why_rows = 2^30");
        c.why_rows = ((int64_t)1 << 30) - 1;
        expect(run(c) == KSCHED_OK, "why_rows = 2^30 - 1");
        c = all_on(); c.no_pod = true;
        expect(run(c) == KSCHED_E_INVALID, "a NULL out_why_pod with why_rows > 0");
        c = all_on(); c.no_counts = true;
        expect(run(c) == KSCHED_E_INVALID, "a NULL out_why_counts with why_rows > 0");
        c = all_on(); c.no_reason = true;
        expect(run(c) == KSCHED_E_INVALID, "a NULL out_why_reason with node_rows > 0");
        // the bound on the per-node bytes: 2^28 exactly is allowed, one row more is not
        c = all_on(); c.n_local = (int64_t)1 << 16; c.why_rows = c.node_rows = (int64_t)1 << 12;
        expect(run(c) == KSCHED_OK, "node_rows * n_local == KSCHED_WHY_MAX_NODE_BYTES");
        c.why_rows = c.node_rows = ((int64_t)1 << 12) + 1;
        expect(run(c) == KSCHED_E_INVALID, "node_rows * n_local above KSCHED_WHY_MAX_NODE_BYTES");
        c.n_local = ((int64_t)1 << 31) - 1; c.why_rows = c.node_rows = ((int64_t)1 << 30) - 1;
        expect(run(c) == KSCHED_E_INVALID, "the largest product: no wrap");
    }
    {   // ksched_schedule_full's cases come first: a call wrong in both ways reports that call's code
        Call c = all_on(); c.why_rows = -1; c.S = 0;
        expect(run(c) == KSCHED_E_STATE, "spread on without a table, before the negative cap");
        c = all_on(); c.why_rows = -1; c.p = -1;
        expect(run(c) == KSCHED_E_INVALID && why && std::strstr(why, "p must be"), "p < 0 first");
        c = all_on(); c.node_rows = 9; c.aff_group = {0, 64, 63};
        expect(run(c) == KSCHED_E_INVALID && why && std::strstr(why, "affinity group"), "an affinity group of 64 first");
        c = all_on(); c.node_rows = 9; c.gang_off = {0, 0, 3};
        expect(run(c) == KSCHED_E_INVALID && why && !std::strstr(why, "node_rows"), "a repeated offset first");
        c = all_on(); c.node_rows = 9;
        expect(run(c) == KSCHED_E_INVALID && why && std::strstr(why, "node_rows"), "then the call's own");
    }
    {   // the layout: 8-byte words first, nothing overlaps, the size the header states
        const WhyLayout l = why_layout(3, 2, 5);
        expect(l.o_counts == 0 && l.o_nofit == 3 * 14 * 8 && l.o_pod == l.o_nofit + 8, "counts, then the total, then the pods");
        expect(l.o_reason == l.o_pod + 16 && l.o_reason % 8 == 0 && l.total == l.o_reason + 10, "the bytes behind the padded pods");
        const WhyLayout z = why_layout(0, 0, 5);
        expect(z.o_nofit == 0 && z.o_pod == 8 && z.total == 8, "no rows: the total alone");
        const WhyLayout e = why_layout(4, 4, 0);
        expect(e.total == e.o_reason, "no nodes: no bytes");
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("why_check: all checks passed\n");
    return 0;
}
