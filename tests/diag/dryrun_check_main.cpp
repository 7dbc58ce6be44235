// dryrun_check_main.cpp -- csrc/ksched_dryrun.h's host side on its own, for a CPU sanitizer run of ksched_rank_full's and
// ksched_explain_full's checks: which constraints a call switches on, the order of the checks, every invalid case of the
// single calls through it, the packing and the waiver (no device call, no library):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ik8s-scheduler_amd/csrc
//       tests/diag/dryrun_check_main.cpp -o dryrun_check; ./dryrun_check
// Every array is allocated at exactly the length its case states, so a read beyond what the arguments allow is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ksched_dryrun.h"

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

// One call: the arrays by value (empty: NULL), and what the context holds.
struct Call {
    int64_t m = 0;
    std::vector<int64_t> rc, rm, rp;
    std::vector<uint64_t> sel;
    std::vector<int32_t> group;
    std::vector<uint8_t> enforce;
    std::vector<int64_t> req;
    std::vector<uint64_t> member, anti_host, anti_zone;
    std::vector<int32_t> aff_group;
    std::vector<uint8_t> aff_zone;
    DryState st{false, 2, 2, true, 0, 0};
};

static DryPacked packed;
static const char *why;

static int run(const Call &c) {
    Exact<int64_t> rc(c.rc), rm(c.rm), rp(c.rp), req(c.req);
    Exact<int32_t> group(c.group), ag(c.aff_group);
    Exact<uint8_t> enf(c.enforce), az(c.aff_zone);
    Exact<uint64_t> sel(c.sel), m(c.member), ah(c.anti_host), anz(c.anti_zone);
    const DryCall a{c.m, rc.p, rm.p, rp.p, sel.p, group.p, enf.p, req.p, m.p, ah.p, anz.p, ag.p, az.p};
    packed = DryPacked{};
    return dry_check_pack(a, c.st, &packed, &why);
}

// three pods, every constraint on: two groups, two columns
static Call all_on() {
    Call c;
    c.m = 3;
    c.rc = {100, 200, 300}; c.rm = {1, 2, 3}; c.rp = {1, 1, 2};
    c.group = {0, 1, -1}; c.enforce = {1, 0, 1};
    c.req = {1, 0, 2, 0, 0, 3};
    c.member = {1, 2, 0}; c.anti_host = {1, 0, 0}; c.anti_zone = {0, 2, 0};
    c.aff_group = {0, -1, 63}; c.aff_zone = {1, 0, 0};
    return c;
}

int main() {
    {   // the packing: group only where the pod enforces, requests pod-major, the affinity words, the scope
        Call c = all_on();
        c.st.any_host = 1; c.st.any_zone = 1;
        expect(run(c) == KSCHED_OK && packed.spread && packed.ext && packed.aff, "all on");
        const DryPod &a = packed.pods[0], &b = packed.pods[1], &d = packed.pods[2];
        expect(a.rc == 100 && b.rm == 2 && d.rp == 2 && a.sel == 0, "requests");
        expect(a.sgroup == 0 && b.sgroup == -1 && d.sgroup == -1, "a pod that only counts enforces nothing");
        expect(a.er[0] == 1 && a.er[1] == 0 && b.er[0] == 0 && b.er[1] == 0 && d.er[0] == 2 && d.er[1] == 3 && d.er[2] == 0 &&
                   d.er[3] == 0, "extended requests, pod-major");
        expect(a.mem == 1 && a.anti_h == 1 && a.anti_z == 0 && a.abit == 1 && a.flags == (kDryAff | kDryAffZone), "pod 0 words");
        expect(b.mem == 2 && b.anti_z == 2 && b.abit == 0 && b.flags == kDryAff, "pod 1 words");
        expect(d.mem == 0 && d.abit == (uint64_t)1 << 63 && d.flags == kDryAff, "pod 2: a term without membership");
    }
    {   // the waiver: the group is nowhere in scope and the pod is in it -- per scope, from the current any words
        Call c = all_on();
        expect(run(c) == KSCHED_OK && packed.pods[0].abit == 0, "waived: zone scope, any_zone has no bit 0");
        expect(packed.pods[2].abit == (uint64_t)1 << 63, "not waived: the pod is not in its term's group");
        c.st.any_host = 1;  // (pod 0's term is of zone scope: any_host does not matter)
        expect(run(c) == KSCHED_OK && packed.pods[0].abit == 0, "waived by scope");
        c.st.any_zone = 1;
        expect(run(c) == KSCHED_OK && packed.pods[0].abit == 1, "not waived: the group is in some zone");
        c.aff_zone = {0, 0, 0}; c.st.any_host = 0;
        expect(run(c) == KSCHED_OK && packed.pods[0].abit == 0 && packed.pods[0].flags == kDryAff, "waived at host scope");
    }
    {   // off: nothing is read, nothing is needed
        Call c;
        c.m = 2; c.rc = {1, 2}; c.rm = {3, 4}; c.rp = {1, 1};
        c.st = DryState{false, 0, 0, false, 0, 0};
        expect(run(c) == KSCHED_OK && !packed.spread && !packed.ext && !packed.aff, "all off without tables");
        expect(packed.pods[1].sgroup == -1 && packed.pods[1].flags == 0 && packed.pods[1].er[0] == 0, "off: no words");
        c.m = 0; c.rc.clear(); c.rm.clear(); c.rp.clear();
        expect(run(c) == KSCHED_OK && packed.pods.empty(), "no pods");
    }
    {   // one affinity pointer switches affinity on; the others mean zeros and no group
        Call c = all_on();
        c.member.clear(); c.anti_host.clear(); c.anti_zone.clear(); c.aff_group.clear();
        expect(run(c) == KSCHED_OK && packed.aff && packed.pods[0].flags == 0, "aff_zone alone: on, and no pod has a word");
    }
    {   // a constraint that is on without its table: KSCHED_E_STATE, before any array is looked at
        Call c = all_on();
        c.st.spread_S = 0; c.group = {7, 7, 7};
        expect(run(c) == KSCHED_E_STATE, "spread on without a table");
        c = all_on(); c.st.ext_R = 0; c.req = {-1, 0, 2, 0, 0, 3};
        expect(run(c) == KSCHED_E_STATE, "ext on without a table");
        c = all_on(); c.st.aff_valid = false;
        expect(run(c) == KSCHED_E_STATE, "affinity on without a table");
    }
    {   // the single calls' argument rules
        Call c = all_on(); c.group = {0, 2, -1};
        expect(run(c) == KSCHED_E_INVALID, "a spread group outside [-1, S)");
        c = all_on(); c.group = {0, -2, -1};
        expect(run(c) == KSCHED_E_INVALID, "a spread group below -1");
        c = all_on(); c.req = {1, 0, 2, 0, -1, 3};
        expect(run(c) == KSCHED_E_INVALID, "a negative extended-resource request");
        c = all_on(); c.aff_group = {0, 64, 63};
        expect(run(c) == KSCHED_E_INVALID, "an affinity group of 64");
        c = all_on(); c.aff_group = {0, -2, 63};
        expect(run(c) == KSCHED_E_INVALID, "an affinity group below -1");
        c = all_on(); c.m = -1;
        expect(run(c) == KSCHED_E_INVALID, "m < 0");
        c = all_on(); c.m = (int64_t)1 << 30;
        expect(run(c) == KSCHED_E_INVALID, "m = 2^30: refused before any array is read");
        c = all_on(); c.rm.clear();
        expect(run(c) == KSCHED_E_INVALID, "a NULL request array");
        c = all_on(); c.st.use_labels = true;
        expect(run(c) == KSCHED_E_INVALID, "use_labels without selectors");
        c.sel = {1, 2, 4};
        expect(run(c) == KSCHED_OK && packed.pods[2].sel == 4, "selectors");
    }
    {   // ksched_explain_full's scalars: a constraint is on where the pod uses it
        expect(dry_check_one(-1, -1) == nullptr && dry_check_one(63, 63) == nullptr, "scalars in range");
        expect(dry_check_one(-2, -1) != nullptr && dry_check_one(0, 64) != nullptr && dry_check_one(0, -2) != nullptr, "scalars out of range");
        const DryState none{false, 0, 0, false, 0, 0}, all{false, 2, 2, true, 0, 0};
        DryOne one{100, 1, 1, 0, 0, 0, 0, -1, -1, 1, 0};
        expect(dry_check_pack(one.call(nullptr), none, &packed, &why) == KSCHED_OK && !packed.spread && !packed.ext && !packed.aff,
               "a plain pod needs no table");
        one.spread_group = 1;
        expect(dry_check_pack(one.call(nullptr), none, &packed, &why) == KSCHED_E_STATE, "a group needs the spread table");
        expect(dry_check_pack(one.call(nullptr), all, &packed, &why) == KSCHED_OK && packed.pods[0].sgroup == 1, "enforcing");
        one.spread_enforce = 0;
        expect(dry_check_pack(one.call(nullptr), all, &packed, &why) == KSCHED_OK && packed.spread && packed.pods[0].sgroup == -1,
               "only counting");
        one.spread_group = 2;
        expect(dry_check_pack(one.call(nullptr), all, &packed, &why) == KSCHED_E_INVALID, "a group beyond the table");
        one.spread_group = -1; one.aff_group = 5;
        expect(dry_check_pack(one.call(nullptr), none, &packed, &why) == KSCHED_E_STATE, "a term needs the affinity table");
        expect(dry_check_pack(one.call(nullptr), all, &packed, &why) == KSCHED_OK && packed.pods[0].abit == 32, "the term's bit");
        one.aff_group = -1; one.anti_zone = 4;
        expect(dry_check_pack(one.call(nullptr), all, &packed, &why) == KSCHED_OK && packed.aff && packed.pods[0].anti_z == 4, "a word alone");
        one.anti_zone = 0;
        Exact<int64_t> req(std::vector<int64_t>{0, 7});
        expect(dry_check_pack(one.call(req.p), none, &packed, &why) == KSCHED_E_STATE, "requests need the ext table");
        expect(dry_check_pack(one.call(req.p), all, &packed, &why) == KSCHED_OK && packed.pods[0].er[1] == 7 && !packed.aff, "requests");
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("dryrun_check: all checks passed\n");
    return 0;
}
