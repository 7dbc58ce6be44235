// full_check_main.cpp -- csrc/ksched_full.h on its own, for a CPU sanitizer run of ksched_schedule_full's host side: which
// constraints a call switches on, the order of its checks, every invalid case of the four calls through it, and the
// packing (no device call, no library):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ik8s-scheduler_amd/csrc
//       tests/diag/full_check_main.cpp -o full_check; ./full_check
// Every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ksched_full.h"

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

// One call: the arrays by value (empty: NULL), the loaded tables' sizes.
struct Call {
    int64_t p = 0, n_gangs = 0;
    std::vector<int64_t> off;
    std::vector<int32_t> gmin, group;
    std::vector<uint8_t> enforce;
    std::vector<int64_t> req;
    std::vector<uint64_t> member, anti_host, anti_zone;
    std::vector<int32_t> aff_group;
    std::vector<uint8_t> aff_zone;
    int32_t S = 2, R = 2;
    bool aff_table = true;
};

static FullPacked packed;
static const char *why;

static int run(const Call &c) {
    Exact<int64_t> off(c.off), req(c.req);
    Exact<int32_t> gmin(c.gmin), group(c.group), ag(c.aff_group);
    Exact<uint8_t> enf(c.enforce), az(c.aff_zone);
    Exact<uint64_t> m(c.member), ah(c.anti_host), anz(c.anti_zone);
    const FullArgs a{c.p, c.n_gangs, off.p, gmin.p, group.p, enf.p, req.p, m.p, ah.p, anz.p, ag.p, az.p};
    packed = FullPacked{};
    return full_check_pack(exact_kind(kRunFull), a, c.S, c.R, c.aff_table, &packed, &why);
}

// three pods, every constraint on: gangs {p0, p1}, {p2}; two groups, two columns
static Call all_on() {
    Call c;
    c.p = 3; c.n_gangs = 2;
    c.off = {0, 2, 3}; c.gmin = {2, 1};
    c.group = {0, 1, -1}; c.enforce = {1, 0, 1};
    c.req = {1, 0, 2, 0, 0, 3};
    c.member = {1, 2, 0}; c.anti_host = {1, 0, 0}; c.anti_zone = {0, 2, 0};
    c.aff_group = {0, -1, 63}; c.aff_zone = {1, 0, 0};
    return c;
}

int main() {
    // ---- every constraint on: the words of the four packers, side by side
    Call c = all_on();
    expect(run(c) == KSCHED_OK && why == nullptr, "all on");
    expect(packed.spread && packed.ext && packed.aff && packed.n_gangs == 2, "all on: every table, the caller's gangs");
    expect(packed.gend == std::vector<int32_t>({0, 2 | 2 << 16, 1 | 1 << 16}), "all on: gang ends");
    expect(packed.swords == std::vector<int32_t>({1, 2, -1}), "all on: spread words");
    expect(packed.ewords == std::vector<int32_t>({1, 0, 3}) && packed.reqs.size() == 3 * KSCHED_EXT_MAX, "all on: ext words");
    expect(packed.awords == std::vector<int32_t>({3, 1, 1}) && packed.apods.size() == 12 &&
               packed.apods[2 * 4 + 3] == (uint64_t)1 << 63, "all on: affinity words");
    // ---- everything off: words that say so, no table named, one gang per pod
    Call none;
    none.p = 3; none.S = none.R = 0; none.aff_table = false;
    expect(run(none) == KSCHED_OK, "all off, no table loaded");
    expect(!packed.spread && !packed.ext && !packed.aff && packed.n_gangs == 3, "all off: no table, gangs of one");
    expect(packed.gend == std::vector<int32_t>(3, 1 | 1 << 16) && packed.swords == std::vector<int32_t>(3, -1) &&
               packed.ewords == std::vector<int32_t>(3, 0) && packed.awords == std::vector<int32_t>(3, 0) &&
               packed.reqs.empty() && packed.apods.empty(), "all off: the words");
    none.p = 0;
    expect(run(none) == KSCHED_OK && packed.gend.empty() && packed.n_gangs == 0, "no pods");
    // ---- affinity is on by any one of its five pointers; the others mean zeros (-1 for aff_group)
    for (int k = 0; k < 5; ++k) {
        Call one;
        one.p = 2; one.S = one.R = 0;
        if (k == 0) one.member = {4, 0};
        if (k == 1) one.anti_host = {4, 0};
        if (k == 2) one.anti_zone = {4, 0};
        if (k == 3) one.aff_group = {2, -1};
        if (k == 4) one.aff_zone = {1, 1};
        expect(run(one) == KSCHED_OK && packed.aff && !packed.spread && !packed.ext, "one affinity pointer switches affinity on");
        // (a scope without a term is no word)
        expect(packed.awords == (k == 4 ? std::vector<int32_t>({0, 0}) : std::vector<int32_t>({1, 0})), "... its words");
        one.aff_table = false;
        expect(run(one) == KSCHED_E_STATE, "... and needs the table");
    }
    // ---- the order: p, the gang arguments' shape, the tables, then the arrays
    // p outside [0, 2^30) is refused before any array is read: one-element arrays
    for (int64_t p : {(int64_t)-1, (int64_t)1 << 30, INT64_MAX, INT64_MIN}) {
        Call bad;
        bad.p = p; bad.n_gangs = 1;
        bad.off = {0}; bad.gmin = {1}; bad.group = {0}; bad.enforce = {1}; bad.req = {1}; bad.member = {1};
        bad.aff_group = {0}; bad.aff_zone = {1};
        bad.S = bad.R = 0; bad.aff_table = false;  // (before the tables too)
        expect(run(bad) == KSCHED_E_INVALID, "p out of range");
    }
    c = all_on(); c.off.clear(); c.gmin.clear(); c.n_gangs = 1; c.S = 0;
    expect(run(c) == KSCHED_E_INVALID, "gang_off NULL with n_gangs 1 (before the missing spread table)");
    c.n_gangs = -1;
    expect(run(c) == KSCHED_E_INVALID, "gang_off NULL with n_gangs -1");
    c = all_on(); c.S = 0; c.group[0] = 7;
    expect(run(c) == KSCHED_E_STATE, "spread on without a table (before its bad group)");
    c = all_on(); c.R = 0; c.req[0] = -1;
    expect(run(c) == KSCHED_E_STATE, "ext on without a table (before its bad request)");
    c = all_on(); c.aff_table = false; c.aff_group[0] = 64;
    expect(run(c) == KSCHED_E_STATE, "affinity on without a table (before its bad group)");
    c = all_on(); c.S = 0; c.R = 0; c.aff_table = false; c.group.clear(); c.enforce.clear(); c.req.clear();
    c.member.clear(); c.anti_host.clear(); c.anti_zone.clear(); c.aff_group.clear(); c.aff_zone.clear();
    expect(run(c) == KSCHED_OK && packed.n_gangs == 2, "gangs alone need no table");
    // ---- every invalid case of the four calls, each with the three other constraints valid beside it
    c = all_on(); c.off[0] = 1;
    expect(run(c) == KSCHED_E_INVALID, "a first offset of 1");
    c = all_on(); c.off[2] = 2;
    expect(run(c) == KSCHED_E_INVALID, "a last offset short of p");
    c = all_on(); c.off[1] = 0;
    expect(run(c) == KSCHED_E_INVALID, "an offset that repeats");
    c = all_on(); c.off[1] = (int64_t)1 << 40;
    expect(run(c) == KSCHED_E_INVALID, "an offset above p");
    c = all_on(); c.off[1] = -5;
    expect(run(c) == KSCHED_E_INVALID, "a negative offset");
    c = all_on(); c.n_gangs = 4;
    expect(run(c) == KSCHED_E_INVALID, "n_gangs above p (refused before gang_off[n_gangs] is read)");
    c = all_on(); c.gmin[0] = 0;
    expect(run(c) == KSCHED_E_INVALID, "a minimum of 0");
    c = all_on(); c.gmin[0] = 3;
    expect(run(c) == KSCHED_E_INVALID, "a minimum of size + 1");
    c = all_on(); c.gmin.clear();
    expect(run(c) == KSCHED_OK && packed.gend[1] == (2 | 2 << 16), "gang_min NULL: every member");
    {
        Call big;
        big.p = KSCHED_GANG_MAX + 1; big.n_gangs = 1; big.off = {0, KSCHED_GANG_MAX + 1};
        expect(run(big) == KSCHED_E_INVALID, "a gang above the cap");
        big.p = KSCHED_GANG_MAX; big.off = {0, KSCHED_GANG_MAX};
        expect(run(big) == KSCHED_OK && packed.gend.back() == (KSCHED_GANG_MAX | KSCHED_GANG_MAX << 16), "a gang at the cap");
    }
    c = all_on(); c.group[1] = 2;
    expect(run(c) == KSCHED_E_INVALID, "a spread group of S");
    c = all_on(); c.group[2] = -2;
    expect(run(c) == KSCHED_E_INVALID, "a spread group of -2");
    c = all_on(); c.enforce.clear();
    expect(run(c) == KSCHED_OK && packed.swords == std::vector<int32_t>({1, 3, -1}), "spread_enforce NULL: every pod enforces");
    c = all_on(); c.req[4] = -1;
    expect(run(c) == KSCHED_E_INVALID, "a request of -1");
    c = all_on(); c.req[5] = INT64_MIN;
    expect(run(c) == KSCHED_E_INVALID, "a request of INT64_MIN");
    c = all_on(); c.aff_group[1] = 64;
    expect(run(c) == KSCHED_E_INVALID, "an affinity group of 64");
    c = all_on(); c.aff_group[2] = -2;
    expect(run(c) == KSCHED_E_INVALID, "an affinity group of -2");
    c = all_on(); c.aff_group[0] = INT32_MIN;
    expect(run(c) == KSCHED_E_INVALID, "an affinity group of INT32_MIN");
    // the first invalid constraint in the order gangs, spread, ext, affinity names the reason
    c = all_on(); c.gmin[0] = 0; c.aff_group[1] = 64;
    expect(run(c) == KSCHED_E_INVALID && why && std::strstr(why, "gang"), "gangs before affinity");
    c = all_on(); c.req[4] = -1; c.aff_group[1] = 64;
    expect(run(c) == KSCHED_E_INVALID && why && !std::strstr(why, "affinity"), "ext before affinity");
    // ---- the worked example of include/ksched.h
    Call w;
    w.p = 6; w.n_gangs = 3; w.off = {0, 3, 5, 6}; w.S = 1; w.R = 1;
    w.group = {0, 0, 0, 0, 0, 0}; w.enforce = {0, 0, 0, 0, 0, 1}; w.req = {1, 1, 1, 1, 1, 0};
    w.member = {1, 1, 1, 1, 1, 0}; w.anti_host = {1, 1, 1, 1, 1, 0};
    w.aff_group = {0, 0, 0, 0, 0, -1}; w.aff_zone = {1, 1, 1, 1, 1, 0};
    expect(run(w) == KSCHED_OK, "the worked example");
    expect(packed.gend == std::vector<int32_t>({0, 0, 3 | 3 << 16, 0, 2 | 2 << 16, 1 | 1 << 16}) &&
               packed.swords == std::vector<int32_t>({0, 0, 0, 0, 0, 1}) &&
               packed.ewords == std::vector<int32_t>({1, 1, 1, 1, 1, 0}) &&
               packed.awords == std::vector<int32_t>({3, 3, 3, 3, 3, 0}), "... its words");
    std::printf(failures ? "%d expectation(s) failed\n" : "every expectation met\n", failures);
    return failures != 0;
}
